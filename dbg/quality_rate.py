#!/usr/bin/env python3
"""What the quality metrics cost.

  quality_rate.py kernel    each device pass alone -- x265amd_picture_ssd (its memset and launch), x265amd_picture_ssim (both launches), x265amd_luma_level -- on a noise picture
                            at 1920x1080 (coded 1920x1088) and at 3840x2160, in both library depths: HIP events round a BATCH of 20 calls (one call is tens of microseconds,
                            too short for an event pair), ms per call = batch / 20, median / min / max of 10 batches after 3 warm-up batches.  Next to each time the bytes the
                            pass has to read (every sample of the planes it compares, once) and that figure over the time as a fraction of the HBM peak, 8 TB/s -- at these
                            sizes a picture fits the 256 MB of last-level cache, so the fraction says how far the pass is from the memory system's best, not where the bytes came from.
  quality_rate.py encoder   the bench's 1080p clip (tests/hevc_testlib.py: survey_clip cfg 2, 28 pictures) through the command line client with and without --psnr --ssim,
                            three runs each, alternating, on one build: frames per second of the whole program run (its start-up included), and that the two streams are equal.

Prints one JSON line per mode.  Needs a GPU.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hevc_testlib as T
import test_quality as Q
import test_hip_quality as HQ

CALLS, BATCHES, WARMUP = 20, 10, 3
HBM_PEAK = 8.0e12


def kernel():
    import torch
    out = {"device": torch.cuda.get_device_name(0), "calls_per_batch": CALLS, "batches": BATCHES}
    for depth in (8, 10):
        lib = HQ._lib(depth)
        bps = 2 if depth > 8 else 1
        for coded, org in (((1920, 1088), (1920, 1080)), ((3840, 2160), (3840, 2160))):
            src, rec = Q.planes(depth, "noise", coded)
            pad = 64
            sp = [np.pad(p, pad if k == 0 else pad // 2, mode="edge") for k, p in enumerate(src)]
            rp = [np.pad(p, pad if k == 0 else pad // 2, mode="edge") for k, p in enumerate(rec)]
            ds, dr = [HQ._to_device(np.ascontiguousarray(p)) for p in sp], [HQ._to_device(np.ascontiguousarray(p)) for p in rp]
            stride, cstride = sp[0].shape[1], sp[1].shape[1]
            offs = [pad * stride + pad, (pad // 2) * cstride + pad // 2, (pad // 2) * cstride + pad // 2]
            sa = np.array([t.data_ptr() + o * bps for t, o in zip(ds, offs)], np.uint64)
            ra = np.array([t.data_ptr() + o * bps for t, o in zip(dr, offs)], np.uint64)
            wb, hb, geo = Q.ssim_geometry(coded)
            d_ssd = torch.zeros(3, dtype=torch.int64, device="cuda")
            d_bands = torch.zeros(2 * len(geo), dtype=torch.int32, device="cuda")
            d_work = torch.zeros((hb - 1) * ((wb - 1 + 3) // 4), dtype=torch.float32, device="cuda")
            d_level = torch.zeros(2, dtype=torch.int64, device="cuda")

            def ssd():
                assert lib.x265amd_picture_ssd(None, T._ptr(sa), T._ptr(ra), stride, cstride, coded[0], coded[1], org[0], org[1], d_ssd.data_ptr()) == 0, lib.x265amd_last_error()

            def ssim():
                assert lib.x265amd_picture_ssim(None, int(sa[0]), int(ra[0]), stride, coded[0], coded[1], d_bands.data_ptr(), d_work.data_ptr(), 0) == 0, lib.x265amd_last_error()

            def level():
                assert lib.x265amd_luma_level(None, int(sa[0]), stride, org[0], org[1], d_level.data_ptr()) == 0, lib.x265amd_last_error()

            need = {"picture_ssd": 2 * (org[0] * coded[1] * 3 // 2) * bps, "picture_ssim": 2 * coded[0] * coded[1] * bps, "luma_level": org[0] * org[1] * bps}
            rec_out = {}
            for name, fn in (("picture_ssd", ssd), ("picture_ssim", ssim), ("luma_level", level)):
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
                med = float(np.median(ms))
                rec_out[name] = {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "bytes_read": need[name], "fraction_of_hbm_peak": need[name] / (med * 1e-3) / HBM_PEAK}
            # what was timed is what the tests hold against the models
            got_ssd = d_ssd.cpu().numpy().view(np.uint64)
            bands = d_bands.cpu().numpy().view(np.uint32).reshape(len(geo), 2)
            rec_out["records_equal_models"] = bool(np.array_equal(got_ssd, Q.model_ssd(depth, src, rec, coded, org)) and
                                                   np.array_equal(bands, Q.model_ssim(depth, src[0], rec[0], coded, want_blocks=False)[0]))
            out["%d-bit %dx%d" % (depth, coded[0], coded[1])] = rec_out
    print(json.dumps(out))


def encoder():
    import test_encoder_quality as EQ
    cli = os.path.join(T.PKG_DIR, "bin", "x265amd")
    frames = T.survey_clip(1920, 1080, 8, 2, 0, 28)
    out = {"pictures": len(frames), "runs": {"plain": [], "psnr_ssim": []}}
    with tempfile.TemporaryDirectory() as d:
        EQ.write_y4m(os.path.join(d, "clip.y4m"), frames, 1920, 1080, 8)
        md5 = {}
        for rep in range(3):
            for name, extra in (("plain", []), ("psnr_ssim", ["--psnr", "--ssim"])):
                t0 = time.perf_counter()
                r = subprocess.run([cli, "--input", os.path.join(d, "clip.y4m"), "-o", os.path.join(d, name + ".hevc"), "--preset", "medium", "--no-info"] + extra,
                                   capture_output=True, text=True, timeout=600)
                dt = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr[-2000:]
                out["runs"][name].append(len(frames) / dt)
                md5[name] = hashlib.md5(open(os.path.join(d, name + ".hevc"), "rb").read()).hexdigest()
                if extra:
                    out["summary"] = [l for l in r.stderr.splitlines() if l.startswith("encoded ")][-1]
        out["streams_equal"] = md5["plain"] == md5["psnr_ssim"]
    for name in ("plain", "psnr_ssim"):
        out[name + "_fps_median"] = float(np.median(out["runs"][name]))
    print(json.dumps(out))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    {"kernel": kernel, "encoder": encoder}[mode]()
