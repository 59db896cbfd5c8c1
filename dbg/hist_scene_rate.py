#!/usr/bin/env python3
"""What the statistics pass of the histogram-based scene-cut detection costs.

  hist_scene_rate.py    x265amd_hist_scene_stats alone (its memset and two launches) on an 8-bit picture at 1920x1080 and at 3840x2160 (coded 1920x1088 and 3840x2160), once
                        with NOISE in all three planes (the bins spread: the common case) and once FLAT (every lane of every wave adds to one LDS bin: the contention
                        case): HIP events round a BATCH of 20 calls (one call is tens of microseconds, too short for an event pair), ms per call = batch / 20, median / min /
                        max of 10 batches after 3 warm-up batches, the picture re-uploaded never; next to it x265amd_aq_energy on the same picture in the same run, the
                        yardstick (a pass of integer work that reads the same three planes once)

Prints one JSON line.  Needs a GPU.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hevc_testlib as T
import test_hist_scenecut as HS

CALLS, BATCHES, WARMUP = 20, 10, 3


def main():
    import torch
    lib = T.load_hip(8).lib
    lib.x265amd_last_error.restype = C.c_char_p
    lib.x265amd_hist_scene_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_uint64, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p, C.c_uint64]
    out = {"depth": 8, "device": torch.cuda.get_device_name(0)}
    for w, h in ((1920, 1088), (3840, 2160)):
        for content in ("noise", "flat"):
            pl = HS.planes(content, w, h)
            pad = 64
            planes = [np.pad(p, pad if k == 0 else pad // 2, mode="edge") for k, p in enumerate(pl)]
            d = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes]
            d_half = torch.from_numpy(np.ascontiguousarray(HS.half_plane(pl[0]))).cuda()
            stride, cstride = planes[0].shape[1], planes[1].shape[1]
            addr = np.array([d[0].data_ptr() + pad * stride + pad, d[1].data_ptr() + (pad // 2) * cstride + pad // 2, d[2].data_ptr() + (pad // 2) * cstride + pad // 2], np.uint64)
            nb = ((w + 15) // 16) * ((h + 15) // 16)
            d_energy = torch.zeros(nb, dtype=torch.int32, device="cuda"); d_wp = torch.zeros(6, dtype=torch.int64, device="cuda")
            d_rec = torch.zeros(HS.record_bytes(h), dtype=torch.uint8, device="cuda")

            def energy():
                assert lib.x265amd_aq_energy(None, T._ptr(addr), C.c_int64(stride), C.c_int64(cstride), w, h, 16, C.c_void_p(d_energy.data_ptr()), C.c_void_p(d_wp.data_ptr())) == 0

            def stats():
                assert lib.x265amd_hist_scene_stats(None, T._ptr(addr), stride, cstride, d_half.data_ptr(), w // 2, w, h, d_rec.data_ptr(), 0) == 0, lib.x265amd_last_error()

            rec = {}
            for name, fn in (("aq_energy", energy), ("hist_scene_stats", stats)):
                ms = []
                for it in range(WARMUP + BATCHES):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(CALLS):
                        fn()
                    b.record()
                    torch.cuda.synchronize()
                    if it >= WARMUP:
                        ms.append(a.elapsed_time(b) / CALLS)
                rec[name] = {"calls_per_batch": CALLS, "batches": BATCHES, "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms)}
            got = HS.parse_record(d_rec.cpu().numpy(), h)
            rec["record_equals_model"] = bool(HS.same_record(got, HS.model(pl, want_quarter=False)[0]))
            rec["non_empty_bins"] = int(np.count_nonzero(got["counts"]))
            rec["bytes_read"] = (w // 2) * (h // 2) + w * h * 3 // 2          # the half-size plane, and the three source planes for the band variances
            out["%dx%d %s" % (w, h, content)] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
