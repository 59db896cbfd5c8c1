#!/usr/bin/env python3
"""Golden data of the quality metrics (--psnr, --ssim, measured light levels) below the encoder.

  tests/golden/quality_golden.npz, per bit depth and plane set of tests/test_quality.py (key d<depth>/<WxH>/<content>/...):
      ssd        the three sums of squared differences: numpy, exact; the original width, every row of the coded height (framefilter.cpp:672-673)
      block_md5  the md5 of every 4x4 block's four sums (int32 [block rows][blocks per row][4]) from the REFERENCE LIBRARY'S OWN ssim_4x4x2_core
      bands      per CTU row the float32 sum's bit pattern and the window count: the reference library's own ssim_4x4x2_core and ssim_end_4 -- both called through its primitive
                 table (slots M_ssim_4x4x2_core and M_ssim_end_4 of x265-amod_amd/host/primitive_table.h) -- under calculateSSIM's loops (framefilter.cpp:828-853) and
                 processPostRow's band limits (:692-711), restated here with the running sum kept in float32
      level      (max, sum) of the source luma over the original size: numpy, exact

This script ASSERTS, before it stores anything,
  - that a strict float32 evaluation of the order in which the reference's -ffast-math build evaluates the 10-bit ssim_end_1 (csrc/quality_dev.h) gives the bits of the
    library's ssim_end_4 on EVERY window of every 10-bit plane set, and that the source's written order gives them on every window of every 8-bit set;
  - that the built libraries' host models give the same records.

  tests/golden/encoder_quality_golden.json, per command line of tests/test_encoder_quality.py, from the reference PROGRAM (oracle/_ref/x265_ref8 / x265_ref10):
      stream_md5, stream_bytes            its stream; stream_md5_without_the_switches: of the same line without --psnr / --ssim, ASSERTED equal
      summary                             the cells of its CSV summary line by header name (--csv at level 0), MaxCLL / MaxFALL included where --max-cll is given
      pictures                            by POC the cells Y PSNR, U PSNR, V PSNR, YUV PSNR, SSIM of a second run with --csv-log-level 1 (a metric that is off: "-");
                                          its stream is ASSERTED equal as well
      log                                 its `frame I / P / B:` lines and its `encoded` line (statsString / printSummary, encoder.cpp:2666-2757)

Reads only oracle/_ref (oracle/build_ref.sh) and the built library's host code; the outputs are committed.  Usage: make_quality_golden.py [kernels] [encoder]
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hevc_testlib as T
import test_quality as Q

_REF = {}


def table_slots():
    """the two slots' indices, from this project's own header"""
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "slots.cpp")
        with open(src, "w") as f:
            f.write('#include "primitive_table.h"\n#include <stdio.h>\nint main() { printf("%d %d\\n", x265amd::slotMisc(x265amd::M_ssim_4x4x2_core), x265amd::slotMisc(x265amd::M_ssim_end_4)); }\n')
        exe = os.path.join(tmp, "slots")
        subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(T.PKG_DIR, "host"), src, "-o", exe])
        core, end4 = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    return core, end4


def ref(depth):
    """(ssim_4x4x2_core, ssim_end_4) of the reference library of that depth, out of its primitive table"""
    if depth not in _REF:
        lib = C.CDLL(os.path.join(T.REF_DIR, "libx265_ref%d.so" % depth))
        lib.x265_param_alloc.restype = C.c_void_p
        p = lib.x265_param_alloc()
        lib.x265_param_default(C.c_void_p(p))
        getattr(lib, "_ZN4x26521x265_setup_primitivesEP10x265_param")(C.c_void_p(p))
        table = (C.c_void_p * 2281).in_dll(lib, "_ZN4x26510primitivesE")
        core_slot, end4_slot = table_slots()
        assert table[core_slot] and table[end4_slot]
        core = C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_void_p)(table[core_slot])
        end4 = C.CFUNCTYPE(C.c_float, C.c_void_p, C.c_void_p, C.c_int)(table[end4_slot])
        _REF[depth] = (lib, core, end4)
    return _REF[depth][1:]


def f32_bits(v):
    return int(np.float32(v).view(np.uint32))


def reference_ssim(depth, src_y, rec_y, coded):
    """(bands [n][2], block sums [hb][wb][4], per-window terms float32 [hb - 1][wb - 1]) from the reference's functions"""
    core, end4 = ref(depth)
    W, H = coded
    (sb, so, st), (rb, ro, rt) = Q.padded(src_y), Q.padded(rec_y)
    isz = sb.itemsize
    fenc, recon = sb.ctypes.data + so * isz, rb.ctypes.data + ro * isz          # sample (0,0)
    wb, hb, geo = Q.ssim_geometry(coded)
    blocks = np.zeros((hb, wb, 4), np.int32)
    bands = np.zeros((len(geo), 2), np.uint32)
    nrows = (H + 63) >> 6
    for row in range(nrows):
        # FrameFilter::processPostRow (framefilter.cpp:692-711)
        b_end, b_start = row == nrows - 1, row == 0
        min_pix = row * 64 - 4 * (not b_start)
        max_pix = min((row + 1) * 64 - 4 * (not b_end), H)
        min_pix += 2 if b_start else -6
        pix1, pix2 = recon + (2 + min_pix * rt) * isz, fenc + (2 + min_pix * st) * isz
        # calculateSSIM (framefilter.cpp:828-853)
        width, height = (W - 2) >> 2, (max_pix - min_pix) >> 2
        buf = np.zeros((2, width + 3, 4), np.int32)
        s0, s1 = 0, 1
        z = 0
        ssim = np.float32(0.0)
        first_block_row = (min_pix - 2) >> 2
        for y in range(1, height):
            while z <= y:
                s0, s1 = s1, s0
                for x in range(0, width, 2):
                    core(pix1 + 4 * (x + z * rt) * isz, rt, pix2 + 4 * (x + z * st) * isz, st, buf[s0, x].ctypes.data)
                blocks[first_block_row + z] = buf[s0, :width]
                z += 1
            for x in range(0, width - 1, 4):
                ssim = np.float32(ssim + np.float32(end4(buf[s0, x].ctypes.data, buf[s1, x].ctypes.data, min(4, width - x - 1))))
        bands[row] = (f32_bits(ssim), (height - 1) * (width - 1))
        assert (first_block_row, height - 1) == geo[row]
    # every window's own term: ssim_end_4 with a width of 1
    terms = np.zeros((hb - 1, wb - 1), np.float32)
    two = np.zeros((2, wb + 1, 4), np.int32)
    for wy in range(hb - 1):
        two[0, :wb] = blocks[wy + 1]; two[1, :wb] = blocks[wy]
        for wx in range(wb - 1):
            terms[wy, wx] = end4(two[0, wx].ctypes.data, two[1, wx].ctypes.data, 1)
    return bands, blocks, terms


def strict_terms(depth, blocks):
    """ssim_end_1 on every window in strict float32, one rounding per operation: for 8-bit the order the source spells (pixel.cpp:693-700), for 10-bit the order the reference's
    -ffast-math build evaluates (csrc/quality_dev.h)"""
    b = blocks.astype(np.int32)
    s = b[:-1, :-1] + b[:-1, 1:] + b[1:, :-1] + b[1:, 1:]
    s1, s2, ss, s12 = [s[..., i] for i in range(4)]
    top = (1 << depth) - 1
    f = np.float32
    if depth == 8:
        c1, c2 = int(.01 * .01 * top * top * 64 + .5), int(.03 * .03 * top * top * 64 * 63 + .5)
        vars_ = ss * 64 - s1 * s1 - s2 * s2
        covar = s12 * 64 - s1 * s2
        return ((2 * s1 * s2 + c1).astype(f) * (2 * covar + c2).astype(f)) / ((s1 * s1 + s2 * s2 + c1).astype(f) * (vars_ + c2).astype(f))
    c1, c2 = f(.01 * .01 * top * top * 64), f(.03 * .03 * top * top * 64 * 63)
    fs1, fs2, fss, fs12 = s1.astype(f), s2.astype(f), ss.astype(f), s12.astype(f)
    p = fs1 * fs2
    t = fs1 * fs1 + fs2 * fs2
    covar = fs12 * f(64) - p
    num = ((covar + covar) + c2) * ((p + p) + c1)
    den = (t + c1) * ((fss * f(64) + c2) - t)
    return num / den


def reference_run(d, depth, cli, name, level=0):
    exe = os.path.join(T.REF_DIR, "x265_ref%d" % depth)
    cmd = [exe, "--input", "clip.y4m", "-o", name + ".hevc", "--csv", name + ".csv"] + (["--csv-log-level", str(level)] if level else []) + cli
    r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=3600)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(d, name + ".hevc"), "rb").read(), os.path.join(d, name + ".csv"), r.stderr


def make_encoder():
    import test_encoder_quality as EQ
    out = {}
    for tag, ((w, h), depth, n, cli, off) in EQ.CASES.items():
        with tempfile.TemporaryDirectory() as d:
            EQ.write_y4m(os.path.join(d, "clip.y4m"), EQ.clip_frames(tag), w, h, depth)
            full = cli + T.PRESET_CLI
            stream, csv, err = reference_run(d, depth, full, "summary")
            md5 = hashlib.md5(stream).hexdigest()
            plain, _, _ = reference_run(d, depth, [a for a in full if a not in off], "plain")
            assert hashlib.md5(plain).hexdigest() == md5, (tag, "the reference's stream changes with the switches")
            frames_stream, frames_csv, _ = reference_run(d, depth, full, "frames", level=1)
            assert hashlib.md5(frames_stream).hexdigest() == md5, tag
            lines = open(frames_csv).read().splitlines()
            header = [c.strip() for c in lines[0].split(",")]
            pictures = {}
            for line in lines[1:]:
                cells = [c.strip() for c in line.split(",")]
                if len(cells) < len(header) - 2 or not cells[0].isdigit():
                    break                   # (the blank line in front of the summary block)
                row = dict(zip(header, cells))
                pictures[int(row["POC"])] = {k: row.get(k, "-") for k in ("Y PSNR", "U PSNR", "V PSNR", "YUV PSNR", "SSIM")}
            assert sorted(pictures) == list(range(n)), (tag, sorted(pictures))
            summary = EQ.summary_cells(csv)
            summary = {k: v for k, v in summary.items() if k not in ("Command", "Date/Time", "Elapsed Time", "FPS", "Version", "")}
            log = EQ.log_lines(err)
            assert ("encoded" in log) and any(k in log for k in "IPB"), (tag, err[-1500:])
            out[tag] = dict(reference_command_line=" ".join(full), stream_md5=md5, stream_bytes=len(stream), stream_md5_without_the_switches=hashlib.md5(plain).hexdigest(),
                            summary=summary, pictures=[pictures[k] for k in range(n)], log=log)
            print(tag, len(stream), md5, summary, log)
    with open(EQ.GOLD_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def make_kernels():
    out = {}
    windows = {8: 0, 10: 0}
    with np.errstate(over="ignore"):
        for depth in (8, 10):
            for coded, org, name in Q.plane_sets(depth):
                src, rec = Q.planes(depth, name, coded)
                key = Q.key_of(depth, coded, name)
                ssd = Q.ssd_numpy(src, rec, coded, org)
                part = src[0][:org[1], :org[0]].astype(np.int64)
                level = np.array([int(part.max()), int(part.sum())], np.uint64)
                bands, blocks, terms = reference_ssim(depth, src[0], rec[0], coded)
                strict = strict_terms(depth, blocks)
                assert strict.dtype == np.float32 and np.array_equal(strict.view(np.uint32), terms.view(np.uint32)), \
                    (key, "the strict float32 order does not give the reference's ssim_end_4", int((strict.view(np.uint32) != terms.view(np.uint32)).sum()), terms.size)
                windows[depth] += terms.size
                # ... and this project's models
                assert np.array_equal(Q.model_ssd(depth, src, rec, coded, org), ssd), key
                got_bands, got_blocks = Q.model_ssim(depth, src[0], rec[0], coded)
                assert np.array_equal(got_blocks, blocks), key
                assert np.array_equal(got_bands, bands), (key, got_bands, bands)
                assert np.array_equal(Q.model_level(depth, src[0], org), level), key
                out[key + "ssd"] = ssd; out[key + "block_md5"] = np.array(Q.arr_md5(blocks)); out[key + "bands"] = bands; out[key + "level"] = level
                print(key, "ssd", list(ssd), "bands", len(bands), "windows", terms.size)
    np.savez_compressed(Q.GOLD_PATH, **out)
    print("strict float32 terms = the reference library's ssim_end_4 on %d 8-bit and %d 10-bit windows; the models give the reference's records on %d plane sets"
          % (windows[8], windows[10], len(out) // 4))


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernels", "encoder"]
    if "kernels" in what:
        make_kernels()
    if "encoder" in what:
        make_encoder()
