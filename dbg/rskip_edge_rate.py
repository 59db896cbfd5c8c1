#!/usr/bin/env python3
"""What the edge-based recursion skip costs.

  rskip_edge_rate.py kernel    x265amd_rskip_edge_counts alone (one launch) on a textured 8-bit picture at 1920x1080 and at 3840x2160: HIP events round a BATCH of 20
                               calls (one call is microseconds, too short for an event pair), ms per call = batch / 20, median / min / max of 10 batches after 3 warm-up
                               batches, the picture re-uploaded never; next to it x265amd_aq_energy on the same picture in the same run, the yardstick (a pass of
                               integer work of the same order that reads the same samples)
  rskip_edge_rate.py encoder   bin/x265amd --preset medium --rskip 2 against --rskip 1 on the same 1280x720 x 30 clip, the two lines ALTERNATING (1, 2, 1, 2, 1, 2):
                               wall-clock frames/s of both from the median of each line's second and third run (the first pays the code objects' load).  Under
                               --rskip 2 the device-run paths of the analysis (skip chain, fused search) are off: the line is slower, and by how much is what this shows

Prints one JSON line per leg.  Needs a GPU.
"""
import ctypes as C
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


CALLS, BATCHES, WARMUP = 20, 10, 3


def kernel_leg():
    import torch
    lib = T.load_hip(8).lib
    lib.x265amd_last_error.restype = C.c_char_p
    out = {"leg": "kernel", "depth": 8, "device": torch.cuda.get_device_name(0)}
    for w, h in ((1920, 1080), (3840, 2160)):
        frame = T.survey_clip(w, h, 8, 2, 0, 1)[0]
        pad = 64
        planes = [np.pad(pl, pad if k == 0 else pad // 2, mode="edge") for k, pl in enumerate(frame)]
        d = [torch.from_numpy(np.ascontiguousarray(pl)).cuda() for pl in planes]
        stride, cstride = planes[0].shape[1], planes[1].shape[1]
        addr = np.array([d[0].data_ptr() + pad * stride + pad, d[1].data_ptr() + (pad // 2) * cstride + pad // 2, d[2].data_ptr() + (pad // 2) * cstride + pad // 2], np.uint64)
        nb = ((w + 15) // 16) * ((h + 15) // 16)
        nb32 = ((w + 31) // 32) * ((h + 31) // 32)
        d_energy = torch.zeros(nb, dtype=torch.int32, device="cuda"); d_counts = torch.zeros(nb32, dtype=torch.int32, device="cuda")
        d_wp = torch.zeros(6, dtype=torch.int64, device="cuda")

        def energy():
            assert lib.x265amd_aq_energy(None, T._ptr(addr), C.c_int64(stride), C.c_int64(cstride), w, h, 16, C.c_void_p(d_energy.data_ptr()), C.c_void_p(d_wp.data_ptr())) == 0

        def counts():
            assert lib.x265amd_rskip_edge_counts(None, C.c_uint64(int(addr[0])), C.c_int64(stride), w, h, C.c_void_p(d_counts.data_ptr())) == 0, lib.x265amd_last_error()

        rec = {}
        for name, fn in (("aq_energy", energy), ("rskip_edge_counts", counts)):
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
        rec["rskip_edge_counts"]["source_bytes"] = w * h
        rec["rskip_edge_counts"]["source_gb_per_s_at_median"] = w * h / (rec["rskip_edge_counts"]["ms_median"] * 1e-3) / 1e9
        got = d_counts.cpu().numpy()
        rec["blocks_with_edges"] = int(np.count_nonzero(got)); rec["ones"] = int(got.astype(np.int64).sum())
        rec["blocks"] = nb32
        out["%dx%d" % (w, h)] = rec
    print(json.dumps(out))


def encoder_leg():
    w, h, n = 1280, 720, 30
    frames = T.survey_clip(w, h, 8, 2, 0, n)
    out = {"leg": "encoder", "size": [w, h], "frames": n}
    exe = os.path.join(ROOT, "x265-amod_amd", "bin", "x265amd")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "clip.y4m"), "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420\n" % (w, h))
            for fr in frames:
                f.write(b"FRAME\n")
                for pl in fr:
                    f.write(np.ascontiguousarray(pl).tobytes())
        runs = {"1": [], "2": []}
        says = {}
        for rep in range(3):
            for mode in ("1", "2"):
                cli = ["--preset", "medium", "--rskip", mode, "--no-info"]
                t0 = time.perf_counter()
                r = subprocess.run([exe, "--input", "clip.y4m", "-o", "m%s.hevc" % mode] + cli, cwd=d, capture_output=True, text=True, timeout=600)
                runs[mode].append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr[-2000:]
                line = [l for l in r.stderr.splitlines() if "encoded" in l]
                says[mode] = line[-1].strip() if line else ""
        for mode in ("1", "2"):
            out["rskip " + mode] = {"command_line": "--preset medium --rskip %s --no-info" % mode, "wall_s": runs[mode], "frames_per_s_wall": n / float(np.median(runs[mode][1:])),
                                      "says": says[mode], "stream_bytes": os.path.getsize(os.path.join(d, "m%s.hevc" % mode))}
    print(json.dumps(out))


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["kernel", "encoder"]:
        {"kernel": kernel_leg, "encoder": encoder_leg}[leg]()
