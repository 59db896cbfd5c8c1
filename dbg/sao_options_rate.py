#!/usr/bin/env python3
"""What the SAO options cost and save (results in profiles/sao_options_rate.md).

  sao_options_rate.py kernel [other_lib.so]   the statistics kernels alone on a textured 8-bit 1920x1080 picture: k_sao_stats in its default form (x265amd_sao_stats), with the
                                              non-deblock skips, without EO_2 / EO_3, with both (x265amd_sao_stats_opt), and k_sao_stats_pre (x265amd_sao_stats_pre).  HIP events
                                              round a BATCH of 20 calls (one call is too short for an event pair), ms per picture = batch / 20, median / min / max of 10
                                              batches after 3 warm-up batches, the legs alternating batch by batch.  With another build of the library named (the parent
                                              commit's) only ITS x265amd_sao_stats is timed, in a process of its own; run the two forms alternately to compare: the default
                                              form is meant not to move
  sao_options_rate.py encoder                 bin/x265amd on the bench clip (survey_clip configuration 2, 1920x1080 x 24) with --preset veryfast and --preset medium, each with
                                              and without --limit-sao, the two lines of a preset ALTERNATING five times: wall-clock frames/s from the median of each line's
                                              second to fifth run (the first pays the code objects' load; a process's start is inside every figure), next to the reference's
                                              published "10% speed benefits at faster presets" 

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
NON_DEBLOCK, EO01_ONLY = 1, 2


def kernel_leg(other=None):
    import torch
    lib = C.CDLL(other) if other else T.load_hip(8).lib
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    lib.x265amd_sao_stats.argtypes = [P, P, P, L, L, I, I, P, P]
    if not other:
        lib.x265amd_sao_stats_opt.argtypes = [P, P, P, L, L, I, I, P, P, I]
        lib.x265amd_sao_stats_pre.argtypes = [P, P, P, L, L, I, I, P, P]
    w, h = 1920, 1080
    coded_h = (h + 7) & ~7
    out = {"leg": "kernel", "depth": 8, "size": [w, coded_h], "device": torch.cuda.get_device_name(0), "calls_per_batch": CALLS, "batches": BATCHES}
    frames = T.survey_clip(w, h, 8, 2, 0, 2)
    pad = lambda pl, rows: np.ascontiguousarray(np.pad(pl, ((0, rows - pl.shape[0]), (0, 0)), mode="edge"))
    rec = [pad(pl, coded_h >> (k > 0)) for k, pl in enumerate(frames[0])]
    fenc = [pad(pl, coded_h >> (k > 0)) for k, pl in enumerate(frames[1])]          # the next picture as "source": differences of a few levels
    d_rec = [torch.from_numpy(p).cuda() for p in rec]; d_fenc = [torch.from_numpy(p).cuda() for p in fenc]
    t_rec = np.array([t.data_ptr() for t in d_rec], np.uint64); t_fenc = np.array([t.data_ptr() for t in d_fenc], np.uint64)
    n = ((w + 63) // 64) * ((coded_h + 63) // 64) * 3 * 5 * 32
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda"); org = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    args = (None, T._ptr(t_rec), T._ptr(t_fenc), w, w // 2, w, coded_h, cnt.data_ptr(), org.data_ptr())
    legs = [("k_sao_stats default", lambda: lib.x265amd_sao_stats(*args)),
            ("k_sao_stats non-deblock", lambda: lib.x265amd_sao_stats_opt(*args, NON_DEBLOCK)),
            ("k_sao_stats EO_0/1 only", lambda: lib.x265amd_sao_stats_opt(*args, EO01_ONLY)),
            ("k_sao_stats non-deblock + EO_0/1 only", lambda: lib.x265amd_sao_stats_opt(*args, NON_DEBLOCK | EO01_ONLY)),
            ("k_sao_stats_pre", lambda: lib.x265amd_sao_stats_pre(*args))]
    if other:
        legs = legs[:1]
        out["other_build"] = other
    ms = {name: [] for name, _ in legs}
    for it in range(WARMUP + BATCHES):
        for name, fn in legs:               # the legs alternate batch by batch
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                assert fn() == 0
            b.record()
            torch.cuda.synchronize()
            if it >= WARMUP:
                ms[name].append(a.elapsed_time(b) / CALLS)
    for name, _ in legs:
        out[name] = {"ms_median": float(np.median(ms[name])), "ms_min": min(ms[name]), "ms_max": max(ms[name])}
    # the bytes a picture's statistics have to read: the deblocked and the source picture once
    out["picture_bytes_read"] = 2 * (w * coded_h * 3 // 2)
    out["k_sao_stats default"]["gb_per_s_at_median"] = out["picture_bytes_read"] / (out["k_sao_stats default"]["ms_median"] * 1e-3) / 1e9
    print(json.dumps(out))


def encoder_leg():
    w, h, n = 1920, 1080, 24
    frames = T.survey_clip(w, h, 8, 2, 0, n)
    out = {"leg": "encoder", "size": [w, h], "frames": n, "reference_claim": "--limit-sao: 10% speed benefits at faster presets (BASELINE.md)"}
    exe = os.path.join(ROOT, "x265-amod_amd", "bin", "x265amd")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "clip.y4m"), "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420\n" % (w, h))
            for fr in frames:
                f.write(b"FRAME\n")
                for pl in fr:
                    f.write(np.ascontiguousarray(pl).tobytes())
        for preset in ("veryfast", "medium"):
            lines = {"plain": ["--preset", preset, "--no-info"], "limit-sao": ["--preset", preset, "--limit-sao", "--no-info"]}
            runs = {k: [] for k in lines}
            for rep in range(5):
                for k, cli in lines.items():
                    t0 = time.perf_counter()
                    r = subprocess.run([exe, "--input", "clip.y4m", "-o", k + ".hevc"] + cli, cwd=d, capture_output=True, text=True, timeout=600)
                    runs[k].append(time.perf_counter() - t0)
                    assert r.returncode == 0, r.stderr[-2000:]
            rec = {k: {"command_line": " ".join(lines[k]), "wall_s": runs[k], "frames_per_s_wall": n / float(np.median(runs[k][1:])),
                       "stream_bytes": os.path.getsize(os.path.join(d, k + ".hevc"))} for k in lines}
            rec["limit_sao_over_plain"] = rec["limit-sao"]["frames_per_s_wall"] / rec["plain"]["frames_per_s_wall"]
            out[preset] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    argv = sys.argv[1:] or ["kernel", "encoder"]
    i = 0
    while i < len(argv):
        if argv[i] == "kernel":
            other = argv[i + 1] if i + 1 < len(argv) and argv[i + 1].endswith(".so") else None
            kernel_leg(other)
            i += 2 if other else 1
        elif argv[i] == "encoder":
            encoder_leg(); i += 1
        else:
            raise SystemExit("sao_options_rate.py [kernel [other_lib.so]] [encoder]")
