#!/usr/bin/env python3
"""Rates of the exhaustive motion search (--me full), device against the reference on the host.

  me_full_rate.py kernel    one x265amd_me_search launch of about 2,000 FULL jobs (the random scene of the tests at 1920x1080, merange 57, 8-bit): HIP events, median of 10
                            after 3 warm-up launches; the same jobs through oracle/_ref's ref_motion_estimate_batch in 16 host processes; candidates/s of both, the share
                            of candidates whose block lies in the staged window, and a comparison of the results
  me_full_rate.py encoder   bin/x265amd --preset medium --me full on 416x240 x 30 against oracle/_ref/x265_ref8 with the same line: frames/s of both, streams compared

Prints one JSON line per leg.  Needs oracle/_ref (oracle/build_ref.sh) and a GPU.
"""
import ctypes as C
import json
import multiprocessing
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hevc_testlib as T

W, H, SEED, MOTION, NJOBS, HOST_PROCS = 1920, 1080, 1, (5, -3), 2000, 16


def scene():
    cur, ref, stride, origin = T.me_make_planes(8, SEED, width=W, height=H, motion=MOTION)
    jobs = T.me_jobs(SEED * 100 + 57, NJOBS, width=W, height=H, motion=MOTION, methods=(5,), submes=(2,), merange=57)
    return cur, ref, stride, origin, T.me_pack_jobs(jobs)


def _host_chunk(k):
    cur, ref, stride, origin, packed = scene()
    part = packed[k::HOST_PROCS]
    L = T.load_ref(8)
    t0 = time.perf_counter()
    out = T.me_run_host_batch(L, cur, ref, stride, origin, part)
    return k, time.perf_counter() - t0, out


def kernel_leg():
    cur, ref, stride, origin, packed = scene()
    area = (packed["mvmax"].astype(np.int64) - packed["mvmin"] + 1).prod(axis=1)
    # the host leg first, in processes forked before this one has touched the GPU
    t0 = time.perf_counter()
    with multiprocessing.get_context("fork").Pool(HOST_PROCS) as pool:
        parts = pool.map(_host_chunk, range(HOST_PROCS))
    host_wall = time.perf_counter() - t0
    want = np.zeros((len(packed), 3), np.int32)
    for k, _, out in parts:
        want[k::HOST_PROCS] = out
    host_busy = max(t for _, t, _ in parts)

    import torch
    me = T.HipME(8)
    groups, order = me.plan(packed)
    ordered = packed[order]
    # candidates whose block (with the 4 samples the dword reads add) lies inside the group's staged window
    inwin = 0
    for g in groups:
        for j in ordered[g["first_job"]:g["first_job"] + g["num_jobs"]]:
            xs = np.arange(j["mvmin"][0], j["mvmax"][0] + 1) + int(j["x"])
            ys = np.arange(j["mvmin"][1], j["mvmax"][1] + 1) + int(j["y"])
            okx = (xs >= g["win_x"]) & (xs + int(j["w"]) + 4 <= int(g["win_x"]) + int(g["win_w"]))
            oky = (ys >= g["win_y"]) & (ys + int(j["h"]) <= int(g["win_y"]) + int(g["win_h"]))
            inwin += int(okx.sum()) * int(oky.sum())
    d_cur, d_ref = me.upload(cur), me.upload(ref)
    d_groups, d_jobs = me.upload(groups), me.upload(ordered)
    d_out = torch.zeros(len(ordered) * 8, dtype=torch.uint8, device="cuda")
    d_reftab = me.upload(np.array([d_ref.data_ptr() + origin], np.uint64))

    def launch(flags):
        rc = me.lib.x265amd_me_search(me.ctx, C.c_void_p(0), C.c_void_p(d_cur.data_ptr() + origin), C.c_void_p(d_reftab.data_ptr()), C.c_int64(stride),
                                      C.c_void_p(d_groups.data_ptr()), len(groups), C.c_void_p(d_jobs.data_ptr()), C.c_void_p(d_out.data_ptr()), 192, 192, flags,
                                      C.c_void_p(0), C.c_int64(0))
        assert rc == 0, me.lib.x265amd_last_error()

    ms = []
    for it in range(13):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch(4)       # X265AMD_ME_FLAG_FULL
        b.record()
        torch.cuda.synchronize()
        if it >= 3:
            ms.append(a.elapsed_time(b))
    res = d_out.cpu().numpy().view(T.ME_RESULT_DT)
    got = np.zeros((len(packed), 3), np.int32)
    got[order, 0] = res["mv"][:, 0]; got[order, 1] = res["mv"][:, 1]; got[order, 2] = res["cost"]
    med = float(np.median(ms))
    print(json.dumps({"leg": "kernel", "jobs": len(packed), "groups": len(groups), "candidates": int(area.sum()), "lds_resident_share": inwin / float(area.sum()),
                      "device_ms_median": med, "device_ms_min": min(ms), "device_ms_max": max(ms), "device_candidates_per_s": float(area.sum()) / (med * 1e-3),
                      "host_processes": HOST_PROCS, "host_wall_s": host_wall, "host_slowest_process_s": host_busy, "host_candidates_per_s": float(area.sum()) / host_busy,
                      "results_equal": bool(np.array_equal(want, got))}))
    me.close()


def encoder_leg():
    w, h, n = 416, 240, 30
    frames = T.survey_clip(w, h, 8, 2, 0, n)
    cli = ["--preset", "medium", "--me", "full", "--no-info"]
    out = {"leg": "encoder", "command_line": " ".join(cli), "size": [w, h], "frames": n}
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "clip.y4m"), "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420\n" % (w, h))
            for fr in frames:
                f.write(b"FRAME\n")
                for pl in fr:
                    f.write(np.ascontiguousarray(pl).tobytes())
        streams = {}
        for name, exe in (("reference", os.path.join(T.REF_DIR, "x265_ref8")), ("device", os.path.join(ROOT, "x265-amod_amd", "bin", "x265amd"))):
            t0 = time.perf_counter()
            r = subprocess.run([exe, "--input", "clip.y4m", "-o", name + ".hevc"] + cli, cwd=d, capture_output=True, text=True, timeout=1500)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-2000:]
            streams[name] = open(os.path.join(d, name + ".hevc"), "rb").read()
            says = [l for l in r.stderr.splitlines() if "encoded" in l]
            out[name] = {"wall_s": dt, "frames_per_s_wall": n / dt, "says": says[-1].strip() if says else ""}
        out["streams_equal"] = streams["reference"] == streams["device"]
    print(json.dumps(out))


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["kernel", "encoder"]:
        {"kernel": kernel_leg, "encoder": encoder_leg}[leg]()
