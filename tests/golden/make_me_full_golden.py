#!/usr/bin/env python3
"""Golden data of the exhaustive motion search (--me full) FROM THE REFERENCE ITSELF.

  tests/golden/me_full_golden.npz           [n,3] results (mvx, mvy, cost) of the reference's MotionEstimate::motionEstimate for method 5 (X265_FULL_SEARCH), both depths,
                                            for the job sets of tests/test_hip_me_full.py (ref_motion_estimate / ref_motion_estimate_c of oracle/_ref/librefprims{8,10}.so)
  tests/golden/encoder_me_full_golden.json  stream md5 + length and the md5 of every reconstructed picture of oracle/_ref/x265_ref{8,10} for the command lines of
                                            tests/test_encoder_me_full.py, in the record layout of encoder_cli_golden.json

Reads only oracle/_ref (oracle/build_ref.sh); the outputs are committed.  Usage: make_me_full_golden.py [me] [encoder]
"""
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
import test_hip_me_full as MF
import test_encoder_me_full as EF


def ref_mvcost(ref):
    import ctypes as C
    ref.lib.ref_mvcost_table.restype = C.POINTER(C.c_uint16)

    def table(qp):
        p = ref.lib.ref_mvcost_table(qp)
        return np.ctypeslib.as_array(C.cast(C.addressof(p.contents) - 2 * 65536, C.POINTER(C.c_uint16)), (2 * 65536 + 1,))
    return table


def make_me_full_golden():
    out = {}
    for depth in (8, 10):
        ref = T.load_ref(depth)
        for key, (planes, jobs, chroma) in MF.golden_sets(depth).items():
            t0 = time.time()
            out[key] = MF.cut(ref, planes, jobs, chroma)
            note = ""
            if "/ties/" in key:
                # the set is only worth its name if many jobs' areas hold the cheapest cost more than once (asserted by the test as well)
                tied = sum(1 for _, n, _ in MF.scan_minima(planes, jobs, ref_mvcost(ref)) if n >= 2)
                assert 3 * tied >= len(jobs), (key, tied, len(jobs))
                note = ", %d of %d jobs with tied minima" % (tied, len(jobs))
            print("%-24s %3d jobs %5.1f s%s" % (key, len(jobs), time.time() - t0, note))
    np.savez_compressed(MF.GOLD_PATH, **out)
    print("wrote me_full_golden.npz with", len(out), "arrays")


def make_encoder_me_full_golden():
    out = {}
    for tag, ((w, h), nframes, depth, cfg_id, cli) in EF.CASES.items():
        planes = T.survey_clip(w, h, depth, cfg_id, 0, nframes)
        cli = cli + T.PRESET_CLI
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "clip.y4m"), "wb") as f:
                f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 %s\n" % (w, h, b"C420p10" if depth == 10 else b"C420"))
                for fr in planes:
                    f.write(b"FRAME\n")
                    for pl in fr:
                        f.write(np.ascontiguousarray(pl).tobytes())
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
            print(tag, out[tag], r.stderr.strip().splitlines()[-1])
    with open(EF.GOLD_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["me", "encoder"]
    if "me" in what:
        make_me_full_golden()
    if "encoder" in what:
        make_encoder_me_full_golden()
