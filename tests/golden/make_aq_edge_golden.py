#!/usr/bin/env python3
"""Golden data of the edge-based adaptive quantisation modes (--aq-mode 4 / 5) FROM THE REFERENCE ITSELF.

  tests/golden/aq_edge_golden.npz           ce<D>/<plane>/{edge,theta}     the reference's own computeEdge (an exported function of oracle/_ref/libx265_ref{8,10}.so, called
                                                                            through ctypes) on the planes of tests/test_aq_edge.py: plane_direct
                                            pic<D>/<WxH>/{edge,theta}      computeEdge on the Gaussian picture of test_aq_edge.picture (the Gaussian is integer arithmetic,
                                                                            made here in numpy), with the source copied in first as edgeFilter does;
                                            pic<D>/<WxH>/{density,angle,sums}  edgeDensityCu's sums over THOSE planes
                                            rc<D>/p<poc>/{energy,density,angle,sums}  per picture of the rate-control clip: acEnergyCu from the reference (librefprims), the
                                                                            edge arrays from the numpy model with the library's host angle function
                                            rc<D>/m<mode>/p<poc>/{qp_aq_offset,inv_qscale}  Lowres::qpAqOffset / invQscaleFactor of oracle/_ref/x265_rc_dump{8,10} encoding
                                                                            the clip with aq-mode=<mode>, cuTree off -- and this script ASSERTS that x265amd_aq_offsets_edge of
                                                                            the built library turns the model's arrays into exactly these doubles before it stores anything:
                                                                            the CPU-side proof of the border rules, the model and the host half against the real encoder
                                            near_pairs                      coprime gradient pairs whose angle lies within one float ulp of a whole degree
                                                                            (tests/native/aq_theta_check.cpp, mode `near`), for the device's angle test
                                            versions                        the C library and compiler the reference's values depend on (its atan2 is the C library's)
  tests/golden/encoder_aq_edge_golden.json  stream md5 + length and the md5 of every reconstructed picture of oracle/_ref/x265_ref{8,10} for the command lines of
                                            tests/test_encoder_aq_edge.py, in the record layout of encoder_cli_golden.json

Reads only oracle/_ref (oracle/build_ref.sh) and the built library's host code; the outputs are committed.  Usage: make_aq_edge_golden.py [planes] [encoder]
"""
import ctypes as C
import hashlib
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hevc_testlib as T
import ratecontrol_lib as RC
import test_aq_edge as AE
import test_encoder_aq_edge as EE

SYMBOL = {8: "_ZN4x26511computeEdgeEPhS0_S0_liibh", 10: "_ZN4x26511computeEdgeEPtS0_S0_liibt"}


def compute_edge(depth, ref, border):
    """the reference's computeEdge(edgePic, refPic, edgeTheta, stride, height, width, true, whitePixel); edgePic starts as `border`, edgeTheta as zeros (edgeFilter)"""
    lib = C.CDLL(os.path.join(T.REF_DIR, "libx265_ref%d.so" % depth))
    fn = getattr(lib, SYMBOL[depth])
    fn.restype = C.c_bool
    h, w = ref.shape
    stride = w + 3
    dt = ref.dtype
    r = np.zeros((h, stride), dt); r[:, :w] = ref
    e = np.zeros((h, stride), dt); e[:, :w] = border
    t = np.zeros((h, stride), dt)
    white = (1 << depth) - 1
    assert fn(T._ptr(e), T._ptr(r), T._ptr(t), C.c_long(stride), C.c_int(h), C.c_int(w), C.c_bool(True), C.c_uint8(white) if depth == 8 else C.c_uint16(white))
    assert not e[:, w:].any() and not t[:, w:].any()
    return e[:, :w].copy(), t[:, :w].copy()


def make_planes():
    out = {}
    out["versions"] = np.array("%s %s; gcc %s" % (platform.libc_ver() + (subprocess.run(["gcc", "-dumpfullversion"], capture_output=True, text=True).stdout.strip(),)))
    for depth in (8, 10):
        for name in AE.DIRECT:
            ref = AE.plane_direct(name, depth)
            out["ce%d/%s/edge" % (depth, name)], out["ce%d/%s/theta" % (depth, name)] = compute_edge(depth, ref, ref)
        for w, h in AE.PICTURES:
            src = AE.picture(w, h, depth)
            edge, theta = compute_edge(depth, AE.gaussian(src).astype(src.dtype), src)
            k = "pic%d/%dx%d/" % (depth, w, h)
            out[k + "edge"], out[k + "theta"] = edge, theta
            out[k + "density"], out[k + "angle"], out[k + "sums"] = AE.block_sums(edge.astype(np.int64), theta.astype(np.int64))
        # the rate-control clip
        w, h, n = AE.RC_CLIPS[depth]
        frames = AE.rc_frames(depth)
        avg = (((w // 2) + 7) >> 3) * (((h // 2) + 7) >> 3)
        ref = T.load_ref(depth)
        arrays = []
        for poc in range(n):
            flat, stride, cstride, org = AE.padded(frames[poc])
            energy, _ = T.aq_run_ref(ref, dict(pic=flat, stride=stride, cstride=cstride, org=org), w, h, 16)
            _, _, density, angle, sums = AE.model(depth, frames[poc][0])
            k = "rc%d/p%d/" % (depth, poc)
            out[k + "energy"], out[k + "density"], out[k + "angle"], out[k + "sums"] = energy, density, angle, sums
            arrays.append((energy, density, angle))
        for mode, opts in AE.RC_OPTS.items():
            with tempfile.TemporaryDirectory() as d:
                recs, _ = RC.reference_rc_records(frames, w, h, depth, AE.RC_PRESET, opts, os.path.join(d, "rc"))
            assert sorted(r["poc"] for r in recs) == list(range(n))
            for r in recs:
                energy, density, angle = arrays[r["poc"]]
                rc, a, t, f = AE.offsets_edge(depth, energy, density, angle, avg, mode)
                assert rc == 0 and len(a) == len(r["aq"]), (len(a), len(r["aq"]))
                same = a.view(np.uint64) == r["aq"].view(np.uint64)
                assert same.all(), (depth, mode, r["poc"], int((~same).sum()), a[~same][:4], r["aq"][~same][:4])
                assert np.array_equal(f, r["inv_qscale"]), (depth, mode, r["poc"])
                k = "rc%d/m%d/p%d/" % (depth, mode, r["poc"])
                out[k + "qp_aq_offset"], out[k + "inv_qscale"] = r["aq"], r["inv_qscale"]
            print("depth %d aq-mode %d: x265amd_aq_offsets_edge of the model's arrays = the reference encoder's doubles, %d pictures" % (depth, mode, len(recs)))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "aq_theta_check")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off", "-I", os.path.join(T.PKG_DIR, "csrc"), "-o", exe, AE.NATIVE])
        subprocess.check_call([exe, "10", "near", os.path.join(d, "near.bin")])
        near = np.fromfile(os.path.join(d, "near.bin"), np.int32).reshape(-1, 2)
    out["near_pairs"] = near[np.lexsort((near[:, 1], near[:, 0]))].astype(np.int16)
    np.savez_compressed(AE.GOLD_PATH, **out)
    print("wrote aq_edge_golden.npz with", len(out), "arrays,", len(near), "near pairs;", out["versions"])


def make_encoder():
    out = {}
    for tag, ((w, h), nframes, depth, _, cli) in EE.CASES.items():
        cli = cli + T.PRESET_CLI
        with tempfile.TemporaryDirectory() as d:
            EE.write_y4m(os.path.join(d, "clip.y4m"), EE.case_frames(tag), w, h, depth)
            exe = os.path.join(T.REF_DIR, "x265_ref%d" % depth)
            t0 = time.time()
            r = subprocess.run([exe, "--input", "clip.y4m", "-o", "out.hevc", "--recon", "rec.yuv"] + cli, cwd=d, capture_output=True, text=True, timeout=7200)
            assert r.returncode == 0, r.stderr[-2000:]
            fsz = w * h * 3 // 2 * (2 if depth == 10 else 1)
            rec = np.fromfile(os.path.join(d, "rec.yuv"), np.uint8)
            assert len(rec) == fsz * nframes
            stream = open(os.path.join(d, "out.hevc"), "rb").read()
            out[tag] = {"stream_md5": hashlib.md5(stream).hexdigest(), "stream_bytes": len(stream),
                        "recon_md5": [hashlib.md5(rec[k * fsz:(k + 1) * fsz].tobytes()).hexdigest() for k in range(nframes)],
                        "reference_command_line": " ".join(cli), "reference_seconds": round(time.time() - t0, 1)}
            if tag == "aq4_fade/":
                # the case is there for the weights: the reference must pick some (its log at --log-level full: "poc: N weights: [L0:R0 Y{scale/2^denom+offset}...")
                r = subprocess.run([exe, "--input", "clip.y4m", "-o", "out2.hevc", "--log-level", "full"] + cli, cwd=d, capture_output=True, text=True, timeout=7200)
                assert r.returncode == 0 and open(os.path.join(d, "out2.hevc"), "rb").read() == stream
                out[tag]["reference_weighted_pictures"] = sum(1 for l in r.stderr.splitlines() if "weights:" in l and "Y{" in l)
                assert out[tag]["reference_weighted_pictures"] > 0
            print(tag, out[tag])
    with open(EE.GOLD_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["planes", "encoder"]
    if "planes" in what:
        make_planes()
    if "encoder" in what:
        make_encoder()
