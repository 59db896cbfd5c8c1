#!/usr/bin/env python3
"""Golden data of the diamond, hexagon and star motion searches at ties and degenerate ranges FROM THE REFERENCE ITSELF.

  tests/golden/me_edges_golden.npz    [n,3] results (mvx, mvy, cost) of the reference's MotionEstimate::motionEstimate for methods 0, 1 and 3, both depths, for the
                                      job sets of tests/test_hip_me_edges.py (ref_motion_estimate / ref_motion_estimate_c of oracle/_ref/librefprims{8,10}.so)

Asserts what makes the sets worth their names (test_hip_me_edges.quality, with the reference's own price tables) and prints the counts reached; the test file's
docstring records them.  Reads only oracle/_ref (oracle/build_ref.sh); the output is committed.  Usage: make_me_edges_golden.py
"""
import io
import os
import sys
import time
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hevc_testlib as T
import test_hip_me_full as MF
import test_hip_me_edges as ME


def make_me_edges_golden():
    out = {}
    for depth in (8, 10):
        ref = T.load_ref(depth)
        mvcost = ME.lib_mvcost(ref)
        for key, (planes, jobs, chroma) in ME.golden_sets(depth).items():
            t0 = time.time()
            out[key] = MF.cut(ref, planes, jobs, chroma)
            note = ME.quality(key, planes, jobs, out[key], mvcost)
            print("%-32s %3d jobs %5.1f s%s" % (key, len(jobs), time.time() - t0, note))
        seen, sizes = ME.pairs_seen(depth)
        assert seen == {(m, s) for m in ME.METHODS for s in range(8)} and sizes == set(ME.SIZES)
    # np.savez_compressed's layout with a fixed member order and a fixed date: the same results give the same bytes
    with zipfile.ZipFile(ME.GOLD_PATH, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(out[k], np.int32), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print("wrote me_edges_golden.npz with", len(out), "arrays,", os.path.getsize(ME.GOLD_PATH), "bytes")


if __name__ == "__main__":
    make_me_edges_golden()
