#!/usr/bin/env python3
"""Golden data of the edge-based recursion skip (--rskip 2) FROM THE REFERENCE ITSELF.

  tests/golden/rskip_edge_golden.npz           ce<D>/<WxH>/<content>   the bit plane of the reference's own computeEdge (an exported function of
                                                                       oracle/_ref/libx265_ref{8,10}.so, called through ctypes) on the planes of
                                                                       tests/test_rskip_edge.py: no angle plane, bcalcTheta false, white pixel 1, the output plane zeroed
                                                                       first as Frame::create does -- what FrameEncoder::compressFrame asks for under --rskip 2.  This
                                                                       script ASSERTS that the built library's host model (x265amd_rskip_edge_model) gives the same planes
                                                                       before it stores anything.
  tests/golden/encoder_rskip_edge_golden.json  stream md5 + length and the md5 of every reconstructed picture of oracle/_ref/x265_ref{8,10} for the command lines of
                                               tests/test_encoder_rskip_edge.py, in the record layout of encoder_aq_edge_golden.json; and per case the stream md5 of three
                                               more reference encodes of the same clip (--rskip 1; --rskip 2 with threshold 100; with threshold 0), which this script
                                               ASSERTS all differ from the case's stream: the case then cannot be met without the edge decision, with it always taken or
                                               with it never taken.

Reads only oracle/_ref (oracle/build_ref.sh) and the built library's host code; the outputs are committed.  Usage: make_rskip_edge_golden.py [planes] [encoder]
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hevc_testlib as T
import test_rskip_edge as RE
import test_encoder_rskip_edge as EE

SYMBOL = {8: "_ZN4x26511computeEdgeEPhS0_S0_liibh", 10: "_ZN4x26511computeEdgeEPtS0_S0_liibt"}


def compute_edge_bits(depth, ref):
    """the reference's computeEdge(edgeBitPic, refPic, NULL, stride, height, width, false, 1) on a zeroed plane"""
    lib = C.CDLL(os.path.join(T.REF_DIR, "libx265_ref%d.so" % depth))
    fn = getattr(lib, SYMBOL[depth])
    fn.restype = C.c_bool
    h, w = ref.shape
    stride = w + 3
    r = np.zeros((h, stride), ref.dtype); r[:, :w] = ref
    e = np.zeros((h, stride), ref.dtype)
    assert fn(T._ptr(e), T._ptr(r), None, C.c_long(stride), C.c_int(h), C.c_int(w), C.c_bool(False), C.c_uint8(1) if depth == 8 else C.c_uint16(1))
    assert not e[:, w:].any() and e.max() <= 1
    return e[:, :w].astype(np.uint8)


def make_planes():
    out = {}
    for depth in (8, 10):
        for w, h in RE.SIZES:
            for name in RE.CONTENTS:
                src = RE.plane(name, w, h, depth)
                bits = compute_edge_bits(depth, src)
                got, counts = RE.model(depth, src, stride_extra=3)
                assert np.array_equal(got, bits), (depth, w, h, name, np.argwhere(got != bits)[:8])
                assert np.array_equal(counts, RE.block_counts(bits)), (depth, w, h, name)
                out["ce%d/%dx%d/%s" % (depth, w, h, name)] = bits
        print("depth %d: x265amd_rskip_edge_model = the reference's computeEdge on %d planes" % (depth, len(RE.SIZES) * len(RE.CONTENTS)))
    np.savez_compressed(RE.GOLD_PATH, **out)
    print("wrote rskip_edge_golden.npz with", len(out), "planes,", os.path.getsize(RE.GOLD_PATH), "bytes")


def reference_encode(d, depth, cli, out_name, recon=None):
    exe = os.path.join(T.REF_DIR, "x265_ref%d" % depth)
    cmd = [exe, "--input", "clip.y4m", "-o", out_name] + (["--recon", recon] if recon else []) + cli
    r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=7200)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(d, out_name), "rb").read()


def make_encoder():
    out = {}
    for tag, ((w, h), nframes, depth, _, cli) in EE.CASES.items():
        with tempfile.TemporaryDirectory() as d:
            EE.write_y4m(os.path.join(d, "clip.y4m"), EE.case_frames(tag), w, h, depth)
            t0 = time.time()
            stream = reference_encode(d, depth, cli + T.PRESET_CLI, "out.hevc", "rec.yuv")
            seconds = round(time.time() - t0, 1)
            fsz = w * h * 3 // 2 * (2 if depth == 10 else 1)
            rec = np.fromfile(os.path.join(d, "rec.yuv"), np.uint8)
            assert len(rec) == fsz * nframes
            others = {}
            for name in sorted(EE.OTHERS):
                other = reference_encode(d, depth, EE.other_cli(cli, name) + T.PRESET_CLI, name + ".hevc")
                assert other != stream, "%s: the reference's stream under %s is the case's own: pick another threshold or clip" % (tag, " ".join(EE.OTHERS[name]))
                others[name] = hashlib.md5(other).hexdigest()
            out[tag] = {"stream_md5": hashlib.md5(stream).hexdigest(), "stream_bytes": len(stream),
                        "recon_md5": [hashlib.md5(rec[k * fsz:(k + 1) * fsz].tobytes()).hexdigest() for k in range(nframes)],
                        "other_stream_md5": others, "reference_command_line": " ".join(cli + T.PRESET_CLI), "reference_seconds": seconds}
            print(tag, out[tag])
    with open(EE.GOLD_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["planes", "encoder"]
    if "planes" in what:
        make_planes()
    if "encoder" in what:
        make_encoder()
