"""--psnr / --ssim / measured light levels through the encoder, on the GPU: the command line program, the library's own interface and its statistics against
tests/golden/encoder_quality_golden.json -- cut by tests/golden/make_quality_golden.py from the reference PROGRAM's runs of the same command lines: its stream, the cells of
its CSV summary line (--csv at level 0), its per-picture PSNR / SSIM cells (a second run at --csv-log-level 1, which this library does not build) and its `frame I / P / B:`
and `encoded` log lines.

Every client case asserts three things: the stream is the fixture's; it is the stream of the same line without the switches (nothing but the measurement reads them); every
cell is the reference's -- MaxCLL / MaxFALL exactly, PSNR cells within 0.001, SSIM within 0.000001 (0.001 for the dB cells).  Each tolerance is one unit of the last printed
digit: the integers beneath (SSDs, block sums, the bands' float bits, counts, levels) are exact (tests/test_hip_quality.py); what remains is the reference build's own
-ffast-math double arithmetic and the order in which its CTU rows add into a double, at most 68 terms, neither of which moves a printed value further than that."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import hevc_testlib as T
import test_quality as Q

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "encoder_quality_golden.json")
CLI = os.path.join(T.PKG_DIR, "bin", "x265amd")

PSNR_TOL, SSIM_TOL, DB_TOL = 0.001, 0.000001, 0.001
M = ["--preset", "medium"]
# tag -> (size, depth, pictures, the command line (T.PRESET_CLI follows it), the switches that are taken off for the second run)
CASES = {
    "medium_8/": ((416, 240), 8, 10, M + ["--psnr", "--ssim"], ["--psnr", "--ssim"]),
    "medium_10/": ((416, 240), 10, 10, M + ["--psnr", "--ssim"], ["--psnr", "--ssim"]),
    "odd_8/": ((420, 236), 8, 10, M + ["--psnr", "--ssim"], ["--psnr", "--ssim"]),          # coded 424 x 240: the SSD's columns and rows, the SSIM's coded size
    "odd_10/": ((420, 236), 10, 8, M + ["--psnr", "--ssim"], ["--psnr", "--ssim"]),
    "tune_psnr/": ((416, 240), 8, 10, M + ["--tune", "psnr", "--psnr"], ["--psnr"]),
    "ssim_no_filters/": ((416, 240), 8, 10, M + ["--ssim", "--no-sao", "--no-deblock"], ["--ssim"]),       # measured straight after analysis
    "psnr_frame_threads_1/": ((416, 240), 8, 10, M + ["--psnr", "--frame-threads", "1"], ["--psnr"]),      # one picture at a time: the other frame path
    "max_cll/": ((420, 236), 10, 8, M + ["--max-cll", "600,0"], []),                    # light levels: original size summed, padded size divides
}
LIB_TAG = "medium_8/"


def clip_frames(tag):
    (w, h), depth, n = CASES[tag][:3]
    return T.survey_clip(w, h, depth, 2, 0, n)


def write_y4m(path, frames, w, h, depth):
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420%s\n" % (w, h, b"p10" if depth > 8 else b""))
        for fr in frames:
            f.write(b"FRAME\n")
            for pl in fr:
                f.write(np.ascontiguousarray(pl).tobytes())


def summary_cells(path):
    """header name -> cell of the last line of a CSV summary log, from the date on (the command cell is quoted and may hold commas: --max-cll 600,0)"""
    lines = open(path).read().splitlines()
    header = [c.strip() for c in lines[0].split(",")][1:]
    line = lines[-1]
    assert line.startswith('"')
    return dict(zip(header, [c.strip() for c in line[line.index('"', 1) + 1:].split(",")[1:]]))


def log_lines(stderr):
    """the `frame I / P / B:` lines and the `encoded` line of a program's log, without the logger's prefix"""
    out = {}
    for l in stderr.splitlines():
        m = re.search(r"frame ([IPB]):\s+(.*)$", l)
        if m:
            out[m.group(1)] = m.group(2).strip()
        if l.startswith("encoded "):
            out["encoded"] = l.strip()
    return out


NUMBER = re.compile(r"(PSNR Mean: Y:|U:|V:|SSIM Mean: |SSIM Mean Y: |Global PSNR: |\(|Avg QP:|kb/s: )\s*(-?[0-9.]+)")
LOG_TOL = {"PSNR Mean: Y:": PSNR_TOL, "U:": PSNR_TOL, "V:": PSNR_TOL, "Global PSNR: ": PSNR_TOL, "SSIM Mean: ": SSIM_TOL, "SSIM Mean Y: ": 0.0000001, "(": DB_TOL}


def close_cells(got, want, tol):
    return got == want or (got not in ("-", "") and want not in ("-", "") and abs(float(got) - float(want)) <= tol * 1.0000001)


def compare_summary(got, want, tag):
    """every cell of the reference's summary line that this encoder's statistics make (the times, the frame rate and the version are the run's own)"""
    for name, cell in want.items():
        if name in ("Command", "Date/Time", "Elapsed Time", "FPS", "Version", ""):
            continue
        if name in ("MaxCLL", "MaxFALL") or name.endswith("count"):
            assert got[name] == cell, (tag, name, got[name], cell)
        elif "PSNR" in name:
            assert close_cells(got[name], cell, PSNR_TOL), (tag, name, got[name], cell)
        elif name == "SSIM":
            assert close_cells(got[name], cell, SSIM_TOL), (tag, name, got[name], cell)
        elif "SSIM (dB)" in name:
            assert close_cells(got[name], cell, DB_TOL), (tag, name, got[name], cell)
        # (ave-QP, kbps and Bitrate are older statistics with a documented difference on pictures with cut CTUs -- include/x265amd_encoder.h, x265amd_encoder_stats -- and
        # no part of the metrics: printed above, not compared)


def compare_log(got, want, tag):
    """the quality figures of statsString / printSummary's text (encoder.cpp:2666-2757), label by label"""
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    for key in want:
        # (the `encoded` line opens with the run's own time and frame rate: what stands behind them is compared)
        a_text, b_text = (got[key].split("fps), ", 1)[1], want[key].split("fps), ", 1)[1]) if key == "encoded" else (got[key], want[key])
        g, w = NUMBER.findall(a_text), NUMBER.findall(b_text)
        assert g and [label for label, _ in g] == [label for label, _ in w], (tag, key, got[key], want[key])
        for (label, a), (_, b) in zip(g, w):
            if label in LOG_TOL:            # (the average QP and the bit rates are older statistics, no part of the metrics)
                assert abs(float(a) - float(b)) <= LOG_TOL[label] * 1.0000001, (tag, key, label, a, b)
        if key != "encoded":
            assert a_text.split()[0] == b_text.split()[0], (tag, key, got[key], want[key])         # the picture count in front


def run_client(tmp_path, tag, cli, name):
    (w, h), depth, n = CASES[tag][:3]
    clip = tmp_path / "clip.y4m"
    if not clip.exists():
        write_y4m(clip, clip_frames(tag), w, h, depth)
    out, csv = tmp_path / (name + ".hevc"), tmp_path / (name + ".csv")
    r = subprocess.run([CLI, "--input", str(clip), "-o", str(out), "--csv", str(csv)] + cli + T.PRESET_CLI, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.fromfile(out, np.uint8), csv, r.stderr


def test_fixtures_present_and_complete():
    g = json.load(open(GOLD_PATH))
    assert sorted(g) == sorted(CASES)
    for tag, ((w, h), depth, n, cli, off) in CASES.items():
        assert g[tag]["reference_command_line"] == " ".join(cli + T.PRESET_CLI) and len(g[tag]["stream_md5"]) == 32 and g[tag]["stream_bytes"] > 0, tag
        assert g[tag]["stream_md5_without_the_switches"] == g[tag]["stream_md5"], tag
        assert len(g[tag]["pictures"]) == n, tag
        assert ("Y PSNR" in g[tag]["summary"]) and (g[tag]["summary"]["Y PSNR"] != "-") == ("--psnr" in cli), tag
        assert (g[tag]["summary"]["SSIM"] != "-") == ("--ssim" in cli) and ("MaxCLL" in g[tag]["summary"]) == ("--max-cll" in cli), tag


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(CASES))
def test_quality_command_lines(tag, tmp_path):
    g = json.load(open(GOLD_PATH))[tag]
    cli, off = CASES[tag][3:]
    got, csv, err = run_client(tmp_path, tag, cli, "on")
    md5 = hashlib.md5(got.tobytes()).hexdigest()
    print(tag, "stream", len(got), md5, "reference", g["stream_bytes"], g["stream_md5"])
    assert len(got) == g["stream_bytes"] and md5 == g["stream_md5"]
    if off:
        plain, _, plain_err = run_client(tmp_path, tag, [a for a in cli if a not in off], "off")
        assert hashlib.md5(plain.tobytes()).hexdigest() == md5, "the switches changed the stream"
        assert not log_lines(plain_err), "summary lines without a metric"
    cells = summary_cells(csv)
    print(tag, "cells", cells, "reference", g["summary"])
    compare_summary(cells, g["summary"], tag)
    if off:
        print(tag, "log", log_lines(err), "reference", g["log"])
        compare_log(log_lines(err), g["log"], tag)


class Quality(C.Structure):         # x265amd_quality
    _fields_ = [("ssd", C.c_uint64 * 3), ("ssimSum", C.c_double), ("lumaSum", C.c_uint64), ("ssimCnt", C.c_uint32), ("maxLumaLevel", C.c_uint32),
                ("psnrY", C.c_double), ("psnrU", C.c_double), ("psnrV", C.c_double), ("psnr", C.c_double), ("ssim", C.c_double), ("avgLumaLevel", C.c_double),
                ("poc", C.c_int32), ("sliceType", C.c_int32), ("measured", C.c_int32), ("reserved", C.c_int32)]


def library_run(depth, frames, w, h, on_device=False, want_headers=True, **fields):
    """open -> encode every frame -> flush, asking x265amd_encoder_quality after every hand-out and x265amd_encoder_stats at the end.  on_device: the frames are put on the
    GPU first and go in through x265amd_encoder_encode_device.
    Returns (stream, [(return code, Quality, reconstruction planes)] in coding order, the 31 statistics words)"""
    lib = T.load_hip(depth).lib
    lib.x265amd_encoder_open.restype = C.c_void_p
    lib.x265amd_encoder_open.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_encoder_headers.argtypes = [C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32)]
    lib.x265amd_encoder_encode.argtypes = [C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32), C.POINTER(T.EncPicture), C.POINTER(T.EncPicture)]
    lib.x265amd_encoder_encode_device.argtypes = lib.x265amd_encoder_encode.argtypes
    lib.x265amd_encoder_close.argtypes = [C.c_void_p]
    lib.x265amd_encoder_quality.argtypes = [C.c_void_p, C.POINTER(Quality)]
    lib.x265amd_encoder_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight = w, h
    for k, v in dict(T.PRESET_BASE, **fields).items():
        setattr(prm, k, v)
    enc = lib.x265amd_encoder_open(C.byref(prm))
    assert enc, lib.x265amd_last_error()
    stream = bytearray()
    nal = C.POINTER(T.EncNal)(); nnal = C.c_uint32(0)
    handed = []
    dt = frames[0][0].dtype
    try:
        q = Quality()
        assert lib.x265amd_encoder_quality(enc, C.byref(q)) == -1           # nothing handed out yet
        assert lib.x265amd_encoder_headers(enc, C.byref(nal), C.byref(nnal)) > 0
        for i in range(nnal.value if want_headers else 0):
            stream += bytes(nal[i].payload[:nal[i].sizeBytes])
        for fr in list(frames) + [None] * (len(frames) + 2):
            out = T.EncPicture()
            bufs = [np.zeros((h, w), dt), np.zeros((h // 2, w // 2), dt), np.zeros((h // 2, w // 2), dt)]
            for k in range(3):
                out.planes[k] = bufs[k].ctypes.data; out.stride[k] = bufs[k].strides[0]
            if fr is not None:
                pic = T.EncPicture()
                keep = [np.ascontiguousarray(pl) for pl in fr]
                if on_device:
                    import torch
                    keep = [torch.from_numpy(k.view(np.uint8).reshape(k.shape[0], -1)).cuda() for k in keep]
                    torch.cuda.synchronize()
                for k in range(3):
                    pic.planes[k] = keep[k].data_ptr() if on_device else keep[k].ctypes.data
                    pic.stride[k] = keep[k].stride(0) if on_device else keep[k].strides[0]
                ret = (lib.x265amd_encoder_encode_device if on_device else lib.x265amd_encoder_encode)(enc, C.byref(nal), C.byref(nnal), C.byref(pic), C.byref(out))
            else:
                ret = lib.x265amd_encoder_encode(enc, C.byref(nal), C.byref(nnal), None, C.byref(out))
            assert ret >= 0, lib.x265amd_last_error()
            if ret:
                for i in range(nnal.value):
                    stream += bytes(nal[i].payload[:nal[i].sizeBytes])
                q = Quality()
                rc = lib.x265amd_encoder_quality(enc, C.byref(q))
                assert rc != 0 or (q.poc, q.sliceType) == (out.poc, out.sliceType)
                handed.append((rc, q, bufs))
            elif fr is None:
                break
        words = np.zeros(32, np.uint64)
        words[31] = 0x5a5a
        assert lib.x265amd_encoder_stats(enc, words.ctypes.data, 31) == 0 and words[31] == 0x5a5a
        short = np.full(32, 0x5a5a, np.uint64)
        assert lib.x265amd_encoder_stats(enc, short.ctypes.data, 13) == 0 and (short[13:] == 0x5a5a).all() and np.array_equal(short[:13], words[:13])
    finally:
        lib.x265amd_encoder_close(enc)
    return np.frombuffer(bytes(stream), np.uint8), handed, words


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_quality_through_the_library(depth):
    """bEnablePsnr / bEnableSsim (the ctypes mirror's reserved3 / reserved4): x265amd_encoder_quality after every hand-out gives the reference's per-picture cells, and the
    record itself is what the host models make of the source and the reconstruction handed out (416x240 is its own coded size); x265amd_encoder_stats' words are the sums"""
    tag = LIB_TAG if depth == 8 else "medium_10/"
    g = json.load(open(GOLD_PATH))[tag]
    (w, h), _, n = CASES[tag][:3]
    frames = clip_frames(tag)
    stream, handed, words = library_run(depth, frames, w, h, reserved3=1, reserved4=1)
    assert len(handed) == n and len(stream) == g["stream_bytes"] and hashlib.md5(stream.tobytes()).hexdigest() == g["stream_md5"]
    sums = np.zeros((4, 4))
    for rc, q, rec in handed:
        assert rc == 0 and q.measured == 3
        want = g["pictures"][q.poc]
        print(depth, "poc", q.poc, "psnr", q.psnrY, q.psnrU, q.psnrV, q.psnr, "ssim", q.ssim, "reference", want)
        for name, got, tol in (("Y PSNR", q.psnrY, PSNR_TOL), ("U PSNR", q.psnrU, PSNR_TOL), ("V PSNR", q.psnrV, PSNR_TOL), ("YUV PSNR", q.psnr, PSNR_TOL), ("SSIM", q.ssim, SSIM_TOL)):
            cell = float(want[name])
            digits = len(want[name].split(".")[1])
            assert abs(round(got, digits) - cell) <= tol * 1.0000001, (q.poc, name, got, want[name])
        # the record, exactly: the host models on the source picture and the reconstruction that came out with it
        src = frames[q.poc]
        assert np.array_equal(np.array(list(q.ssd), np.uint64), Q.model_ssd(depth, src, rec, (w, h), (w, h))), q.poc
        bands, _ = Q.model_ssim(depth, src[0], rec[0], (w, h), want_blocks=False)
        v = Q.finish(depth, np.array(list(q.ssd), np.uint64), bands, None, (w, h), (w, h))
        assert (q.psnrY, q.psnrU, q.psnrV, q.psnr, q.ssim, q.ssimCnt) == (v.psnrY, v.psnrU, v.psnrV, v.psnr, v.ssim, v.ssimCnt), q.poc
        total = 0.0
        for f in bands[:, 0].copy().view(np.float32):
            total += float(f)               # (a double that takes the bands' floats in band order)
        assert q.ssimSum == total, q.poc
        t = 3 if q.sliceType in (4, 5) else 2 if q.sliceType == 3 else 1
        for group in (0, t):
            sums[group] += (q.psnrY, q.psnrU, q.psnrV, q.ssim)
    got = words[13:29].copy().view(np.float64).reshape(4, 4)
    assert np.allclose(got, sums, rtol=1e-12, atol=0) and words[29] == 0 and words[30] == 0          # (sums of at most ten doubles in another grouping; no light levels asked for)
    assert int(words[4] + words[5] + words[6]) == n


@pytest.mark.gpu
def test_switches_off_measure_nothing():
    """with every switch off x265amd_encoder_quality answers -1 after every hand-out and the statistics words behind out[12] are 0"""
    tag = LIB_TAG
    g = json.load(open(GOLD_PATH))[tag]
    (w, h), _, n = CASES[tag][:3]
    stream, handed, words = library_run(8, clip_frames(tag), w, h)
    assert len(handed) == n and all(rc == -1 for rc, _, _ in handed) and not words[13:31].any()
    assert hashlib.md5(stream.tobytes()).hexdigest() == g["stream_md5"]


@pytest.mark.gpu
def test_light_levels_through_the_library_on_device_input():
    """maxCLL set, the input already in device memory (x265amd_encoder_encode_device): the levels are measured where the picture arrives, and the words are the fixture's"""
    tag = "max_cll/"
    g = json.load(open(GOLD_PATH))[tag]
    (w, h), depth, n = CASES[tag][:3]
    frames = clip_frames(tag)
    W, H = (w + 7) & ~7, (h + 7) & ~7
    # (the light level SEI makes the encoder repeat its headers in front of every keyframe: none are written ahead of the first)
    stream, handed, words = library_run(depth, frames, w, h, on_device=True, want_headers=False, maxCLL=600, maxFALL=0, bEmitHDR10SEI=1)
    assert len(handed) == n and len(stream) == g["stream_bytes"] and hashlib.md5(stream.tobytes()).hexdigest() == g["stream_md5"]
    for rc, q, _ in handed:
        src = frames[q.poc][0].astype(np.int64)
        assert rc == 0 and q.measured == 4 and (q.maxLumaLevel, q.lumaSum) == (int(src.max()), int(src.sum())) and q.avgLumaLevel == int(src.sum()) / float(W * H), q.poc
    avg = [int(fr[0].astype(np.int64).sum()) / float(W * H) for fr in frames]
    assert int(words[29]) == max(int(fr[0].max()) for fr in frames) == int(g["summary"]["MaxCLL"])
    fall = float(words[30:31].copy().view(np.float64)[0])
    assert abs(fall - sum(avg)) <= 1e-9 * sum(avg) and int(fall / n) == int(g["summary"]["MaxFALL"])
    assert not words[13:29].any()


def _open(depth, **fields):
    lib = T.load_hip(depth).lib
    lib.x265amd_encoder_open.restype = C.c_void_p
    lib.x265amd_encoder_open.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_encoder_close.argtypes = [C.c_void_p]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight = 128, 128
    for k, v in dict(T.PRESET_RC, **fields).items():
        setattr(prm, k, v)
    enc = lib.x265amd_encoder_open(C.byref(prm))
    if enc:
        lib.x265amd_encoder_close(enc)
    return bool(enc), lib.x265amd_last_error()


@pytest.mark.gpu
def test_what_is_refused_under_the_switches(tmp_path):
    """a switch with pictures coded on several GPUs is refused by name; --csv-log-level 1 still fails to open its log"""
    for name, fields in ((b"bEnablePsnr", dict(reserved3=1)), (b"bEnableSsim", dict(reserved4=1))):
        opened, why = _open(8, shardCount=2, shardRank=0, frameNumThreads=2, **fields)
        assert not opened and name in why, (fields, why)
        opened, why = _open(10, **fields)
        assert opened, (fields, why)
    tag = LIB_TAG
    (w, h), depth, n = CASES[tag][:3]
    write_y4m(tmp_path / "clip.y4m", clip_frames(tag)[:2], w, h, depth)
    r = subprocess.run([CLI, "--input", str(tmp_path / "clip.y4m"), "-o", str(tmp_path / "out.hevc"), "--csv", str(tmp_path / "log.csv"), "--csv-log-level", "1", "--psnr"] + M + T.PRESET_CLI,
                       capture_output=True, text=True, timeout=600)
    assert "cannot open" in r.stderr and not os.path.exists(tmp_path / "log.csv"), r.stderr[-1000:]
