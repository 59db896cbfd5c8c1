#!/usr/bin/env python3
"""Rates of the low-pass transform (--lowpass-dct) -> profiles/lowpass_dct_rate.md.

  lowpass_dct_rate.py kernel     one x265amd_tu_chain launch of 4096 units (half 32x32, half 16x16 luma, the units of hevc_testlib.tu_cases repeated), every unit with
                                 X265AMD_TU_LOWPASS against every unit without; HIP events round single launches, median (min .. max) of 10 after 3 warm-ups, the two
                                 legs alternating; 8 and 10 bits
  lowpass_dct_rate.py encoder    bin/x265amd on the bench clip (survey_clip configuration 2, 1920x1080 x 24) with --preset medium, with and without --lowpass-dct, the
                                 two lines alternating five times, wall clock of the whole process

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

UNITS, LAUNCHES, WARMUP = 4096, 10, 3


def kernel_leg(depth):
    import torch
    L = T.load_hip(depth)
    pool = [c for c in T.tu_cases(depth, 31337, 400) if c["ttype"] == 0]
    big = {5: [c for c in pool if c["log2"] == 5][:16], 4: [c for c in pool if c["log2"] == 4][:16]}
    cases = [big[5 if i % 2 == 0 else 4][(i // 2) % 16] for i in range(UNITS)]
    dt = L.pixel
    isz = np.dtype(dt).itemsize
    per = 32 * 32 * (isz * 3 + 2 * 2)
    arena = np.zeros(UNITS * per, np.uint8)
    for i, c in enumerate(cases):
        N = 1 << c["log2"]
        arena[i * per:i * per + 1024 * isz].view(dt).reshape(32, 32)[:N, :N] = c["fenc"]
        arena[i * per + 1024 * isz:i * per + 2048 * isz].view(dt).reshape(32, 32)[:N, :N] = c["pred"]
    d_arena = torch.from_numpy(arena).cuda()
    a0 = d_arena.data_ptr()
    d_jobs = {}
    for flag in (0, 1):
        jobs = np.zeros(UNITS, T.TU_JOB_DT)
        for i, c in enumerate(cases):
            b = a0 + i * per
            jobs[i] = (b, b + 1024 * isz, b + 3072 * isz, b + 3072 * isz + 2048, b + 2048 * isz, 32, 32, 32, 32, c["log2"], 0, c["intra"], c["dir"], c["slice"], c["qp"], c["signhide"], flag)
        d_jobs[flag] = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(UNITS * T.TU_RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = {0: [], 1: []}
    sig = {}
    for it in range(WARMUP + LAUNCHES):
        for flag in (0, 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            assert L.lib.x265amd_tu_chain(None, C.c_void_p(d_jobs[flag].data_ptr()), UNITS, C.c_void_p(d_out.data_ptr())) == 0
            b.record()
            torch.cuda.synchronize()
            if it >= WARMUP:
                ms[flag].append(a.elapsed_time(b))
            sig[flag] = int(d_out.cpu().numpy().view(T.TU_RESULT_DT)["num_sig"].astype(np.int64).sum())
    out = {"leg": "kernel", "depth": depth, "device": torch.cuda.get_device_name(0), "units": UNITS, "launches": LAUNCHES}
    for flag, name in ((0, "standard"), (1, "lowpass")):
        out[name] = {"ms_median": float(np.median(ms[flag])), "ms_min": min(ms[flag]), "ms_max": max(ms[flag]), "levels": sig[flag]}
    out["lowpass_over_standard"] = out["lowpass"]["ms_median"] / out["standard"]["ms_median"]
    print(json.dumps(out), flush=True)


def encoder_leg():
    w, h, n = 1920, 1080, 24
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
        lines = {"plain": ["--preset", "medium", "--no-info"], "lowpass-dct": ["--preset", "medium", "--lowpass-dct", "--no-info"]}
        runs = {k: [] for k in lines}
        for rep in range(5):
            for k, cli in lines.items():
                t0 = time.perf_counter()
                r = subprocess.run([exe, "--input", "clip.y4m", "-o", k + ".hevc"] + cli, cwd=d, capture_output=True, text=True, timeout=600)
                runs[k].append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr[-2000:]
        for k in lines:
            out[k] = {"command_line": " ".join(lines[k]), "wall_s": runs[k], "frames_per_s_wall": n / float(np.median(runs[k][1:])),
                      "stream_bytes": os.path.getsize(os.path.join(d, k + ".hevc"))}
        out["lowpass_over_plain"] = out["lowpass-dct"]["frames_per_s_wall"] / out["plain"]["frames_per_s_wall"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["kernel", "encoder"]:
        if leg == "kernel":
            kernel_leg(8); kernel_leg(10)
        elif leg == "encoder":
            encoder_leg()
        else:
            raise SystemExit("lowpass_dct_rate.py [kernel] [encoder]")
