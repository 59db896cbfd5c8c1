"""--psnr / --ssim / measured light levels at the public boundaries, without a GPU: the two members' places in x265amd_param, the members of x265_stats and
x265_sliceType_stats that x265_api_abi.cpp writes (tests/native/abi_layout_quality_check.cpp against the reference's header), x265_param_parse of the switches against the
reference library's own, and x265_csvlog_encode's cells on a hand-filled statistics block against the reference's formats (source/encoder/api.cpp:1570-1629)."""
import ctypes as C
import math
import os
import struct
import subprocess

import pytest

import hevc_testlib as T
import test_x265_api_abi as A

L = A.LAYOUT


def test_param_slots_keep_their_places():
    """x265amd_param.bEnablePsnr / bEnableSsim are the four bytes each that the ctypes mirror still calls reserved3 / reserved4, 0 by default"""
    for depth in (8, 10):
        lib = T.load_hip(depth).lib
        lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
        prm = T.EncParam()
        lib.x265amd_param_default(C.byref(prm))
        assert prm.reserved3 == 0 and prm.reserved4 == 0
    assert T.EncParam.reserved3.offset == T.EncParam.vuiDispWinBottom.offset + 4 == T.EncParam.bEnableAccessUnitDelimiters.offset - 4
    assert T.EncParam.reserved4.offset == T.EncParam.decodedPictureHashSEI.offset + 4 == T.EncParam.deblockingFilterTCOffset.offset - 4


def test_layout_of_the_members_in_both_headers():
    """tests/native/abi_layout_quality_check.cpp: the slots in x265amd_param, x265amd_quality, and -- where the reference's headers are built -- every offset of x265_stats /
    x265_sliceType_stats that get_stats writes, the derived ones included"""
    ref_src = os.path.join(T.REF_DIR, "include")
    cmd = ["g++", "-std=gnu++11", "-fsyntax-only", "-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.PKG_DIR, "host")]
    if os.path.isdir(ref_src):
        cmd += ["-DWITH_REFERENCE_HEADER", "-I" + os.path.join(T.REF_DIR, "cfg"), "-I" + ref_src]
    r = subprocess.run(cmd + [os.path.join(T.ROOT, "tests", "native", "abi_layout_quality_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _switches(p):
    buf = (C.c_ubyte * L["SIZEOF_PARAM"]).from_address(p)
    return tuple(int.from_bytes(bytes(buf[L["PARAM_" + n]:L["PARAM_" + n] + 4]), "little", signed=True) for n in ("bEnablePsnr", "bEnableSsim"))


CASES = ((b"psnr", None, (1, 0)), (b"ssim", None, (1, 1)), (b"no-psnr", None, (0, 1)), (b"no-ssim", None, (0, 0)), (b"ssim", b"1", (0, 1)), (b"psnr", b"true", (1, 1)),
         (b"no-ssim", b"1", (1, 0)), (b"psnr", b"0", (0, 0)))


@pytest.mark.parametrize("depth", [8, 10])
def test_param_parse_knows_the_switches(depth):
    f = A._fns(A.table(depth), depth)
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0 and _switches(p) == (0, 0)
    for name, value, want in CASES:
        assert f["parse"](p, name, value) == 0 and _switches(p) == want, (name, value)
    assert f["parse"](p, b"psnr", b"perhaps") == -2
    f["free"](p)


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref (the reference build) is not present")
def test_param_parse_of_the_switches_matches_the_references():
    """x265_param_parse of psnr, ssim, no-psnr and no-ssim through our table against the reference library's own: return code and every member; the two tunes named after
    the metrics switch neither on, in both"""
    R, f = A._reference_api(), A._fns(A.table(8))
    a, b = R.x265_param_alloc(), f["alloc"]()
    R.x265_param_default_preset(a, b"medium", None); f["preset"](b, b"medium", None)
    for name, value, want in CASES:
        ra, rb = R.x265_param_parse(a, name, value), f["parse"](b, name, value)
        assert ra == rb == 0, (name, value, ra, rb)
        assert A._members(a) == A._members(b) and _switches(a) == _switches(b) == want, (name, value)
    for tune in (b"psnr", b"ssim"):
        R.x265_param_default_preset(a, b"medium", tune); f["preset"](b, b"medium", tune)
        assert A._members(a) == A._members(b) and _switches(a) == _switches(b) == (0, 0), tune
    R.x265_param_free(a); f["free"](b)


def _ssim2db(v):
    return 100.0 if 1 - v <= 0.0000000001 else -10.0 * math.log10(1 - v)


def _csv_line(tmp_path, depth, psnr, ssim, max_cll, stats):
    """x265_csvlog_open + x265_csvlog_encode through the table on the given statistics block: the cells of the one line behind the header"""
    lib = A.table(depth)
    f = A._fns(lib, depth)
    api = f["api"]
    csv_open = C.CFUNCTYPE(C.c_void_p, C.c_void_p)(api.fn2[4])
    csv_encode = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p)(api.fn2[6])
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0
    for name, on in ((b"psnr", psnr), (b"ssim", ssim)):
        assert f["parse"](p, name if on else b"no-" + name, None) == 0
    if max_cll:
        assert f["parse"](p, b"max-cll", max_cll) == 0
    path = str(tmp_path / ("log_%d_%d_%d.csv" % (psnr, ssim, bool(max_cll)))).encode()
    buf = (C.c_ubyte * L["SIZEOF_PARAM"]).from_address(p)
    keep = C.create_string_buffer(path)
    buf[L["PARAM_csvfn"]:L["PARAM_csvfn"] + 8] = list(C.addressof(keep).to_bytes(8, "little"))
    fp = csv_open(p)
    assert fp
    buf[L["PARAM_csvfpt"]:L["PARAM_csvfpt"] + 8] = list(int(fp).to_bytes(8, "little"))
    csv_encode(p, stats, 0, 0, 0, None)
    libc = C.CDLL(None)
    libc.fclose.argtypes = [C.c_void_p]
    libc.fclose(fp)
    f["free"](p)
    header, line = open(path.decode()).read().splitlines()
    return [c.strip() for c in header.split(",")], [c.strip() for c in line.split(",")]


def _stats_block():
    """an x265_stats as x265_encoder_get_stats fills it for 2 I, 5 P and 3 B pictures: (bytes, the numbers)"""
    st = bytearray(L["SIZEOF_STATS"])
    n = dict(I=2, P=5, B=3)
    v = dict(sumY=10 * 41.23456, sumU=10 * 44.5, sumV=10 * 45.4996, ssim=0.9812345678, cll=587, fall=143,
             I=(24.5, 812.345, 43.21049, 45.0005, 46.0, 17.2345), P=(27.25, 210.5, 41.0, 44.125, 45.25, 16.001), B=(29.0, 55.125, 40.5, 44.0, 45.0, 100.0))
    v["global"] = (v["sumY"] * 6 + v["sumU"] + v["sumV"]) / (8 * 10)
    struct.pack_into("<4d", st, L["STATS_globalPsnrY"], v["sumY"], v["sumU"], v["sumV"], v["global"])
    struct.pack_into("<d", st, L["STATS_globalSsim"], v["ssim"])
    struct.pack_into("<d", st, L["STATS_elapsedEncodeTime"], 2.5)
    struct.pack_into("<d", st, L["STATS_bitrate"], 321.987)
    struct.pack_into("<I", st, L["STATS_encodedPictureCount"], 10)
    for t in "IPB":
        at = L["STATS_stats" + t]
        qp, kbps, y, u, vv, db = v[t]
        struct.pack_into("<2d", st, at + L["SLICESTATS_avgQp"], qp, kbps)
        struct.pack_into("<4d", st, at + L["SLICESTATS_psnrY"], y, u, vv, db)
        struct.pack_into("<I", st, at + L["SLICESTATS_numPics"], n[t])
    struct.pack_into("<2H", st, L["STATS_maxCLL"], v["cll"], v["fall"])
    return (C.c_ubyte * len(st)).from_buffer(st), v, n


@pytest.mark.parametrize("depth", [8, 10])
def test_csvlog_encode_prints_the_references_cells(depth, tmp_path):
    """the summary line's cells in the reference's formats (api.cpp:1570-1629): Y / U / V PSNR are the SUMS over the picture count, the global PSNR and SSIM as stored, the
    SSIM in dB through x265_ssim2dB; per type the stored means; the light levels behind them; `-` in every cell of a metric that is off"""
    stats, v, n = _stats_block()
    header, cells = _csv_line(tmp_path, depth, 1, 1, b"600,0", stats)
    col = {name: cells[i + (len(cells) - len(header))] for i, name in enumerate(header)}        # (the command cell is empty without a command line; the date holds no comma here or the offset takes it up)
    assert [col[k] for k in ("Y PSNR", "U PSNR", "V PSNR", "Global PSNR")] == ["%.3f" % (v["sumY"] / 10), "%.3f" % (v["sumU"] / 10), "%.3f" % (v["sumV"] / 10), "%.3f" % v["global"]]
    assert col["SSIM"] == "%.6f" % v["ssim"] and col["SSIM (dB)"] == ("%6.3f" % _ssim2db(v["ssim"])).strip()
    for t in "IPB":
        qp, kbps, y, u, vv, db = v[t]
        assert [col[t + k] for k in (" count", " ave-QP", " kbps", "-PSNR Y", "-PSNR U", "-PSNR V", "-SSIM (dB)")] == \
            ["%u" % n[t], "%2.2f" % qp, ("%-8.2f" % kbps).strip(), "%.3f" % y, "%.3f" % u, "%.3f" % vv, "%.3f" % db], t
    assert col["MaxCLL"] == "587" and col["MaxFALL"] == "143"
    # one metric, then none: the other cells are `-`, the light level columns are gone without --max-cll
    header, cells = _csv_line(tmp_path, depth, 1, 0, None, stats)
    col = {name: cells[i + (len(cells) - len(header))] for i, name in enumerate(header)}
    assert "MaxCLL" not in col and col["Y PSNR"] == "%.3f" % (v["sumY"] / 10) and col["SSIM"] == col["SSIM (dB)"] == col["I-SSIM (dB)"] == col["B-SSIM (dB)"] == "-"
    assert col["P-PSNR V"] == "%.3f" % v["P"][4]
    header, cells = _csv_line(tmp_path, depth, 0, 1, None, stats)
    col = {name: cells[i + (len(cells) - len(header))] for i, name in enumerate(header)}
    assert col["Y PSNR"] == col["Global PSNR"] == col["I-PSNR Y"] == col["B-PSNR V"] == "-" and col["SSIM"] == "%.6f" % v["ssim"] and col["B-SSIM (dB)"] == "100.000"
    header, cells = _csv_line(tmp_path, depth, 0, 0, None, stats)
    col = {name: cells[i + (len(cells) - len(header))] for i, name in enumerate(header)}
    assert [col[k] for k in ("Y PSNR", "U PSNR", "V PSNR", "Global PSNR", "SSIM", "SSIM (dB)", "P-PSNR Y", "P-SSIM (dB)")] == ["-"] * 8 and col["P count"] == "5"


def test_per_frame_csv_levels_stay_unbuilt(tmp_path):
    """--csv-log-level 1 / 2 need the CU statistics: x265_csvlog_open still answers NULL for them, by name"""
    lib = A.table(8)
    f = A._fns(lib)
    lib.x265amd_last_error.restype = C.c_char_p
    csv_open = C.CFUNCTYPE(C.c_void_p, C.c_void_p)(f["api"].fn2[4])
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0 and f["parse"](p, b"psnr", None) == 0
    buf = (C.c_ubyte * L["SIZEOF_PARAM"]).from_address(p)
    keep = C.create_string_buffer(str(tmp_path / "frames.csv").encode())
    buf[L["PARAM_csvfn"]:L["PARAM_csvfn"] + 8] = list(C.addressof(keep).to_bytes(8, "little"))
    for level in (1, 2):
        buf[L["PARAM_csvLogLevel"]:L["PARAM_csvLogLevel"] + 4] = list(level.to_bytes(4, "little"))
        assert not csv_open(p) and b"per-frame log level" in lib.x265amd_last_error()
    assert not os.path.exists(str(tmp_path / "frames.csv"))
    f["free"](p)


def test_quality_entry_point_refuses_null():
    lib = T.load_hip(8).lib
    lib.x265amd_encoder_quality.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.x265amd_encoder_quality(None, None) == -1
