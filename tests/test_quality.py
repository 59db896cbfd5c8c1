"""Quality metrics (--psnr, --ssim, measured light levels) below the encoder, without a GPU: the host models x265amd_picture_ssd_model, x265amd_picture_ssim_model and
x265amd_luma_level_model and the host function x265amd_quality_finish, in both library depths, against tests/golden/quality_golden.npz -- cut by
tests/golden/make_quality_golden.py with numpy (SSD, light levels: exact integers) and with the reference library's OWN ssim_4x4x2_core and ssim_end_4, called through its
primitive table, under calculateSSIM's and processPostRow's loops restated in Python in float32.

Everything compared here is exact: 64-bit sums, the md5 of the 32-bit block sums, the bit patterns of the bands' float32 sums, the window counts.  The kernels' tests
(tests/test_hip_quality.py) use the plane sets and helpers of this file."""
import ctypes as C
import hashlib
import math
import os

import numpy as np
import pytest

import hevc_testlib as T

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "quality_golden.npz")

# coded size, original size:
#   64x16     one band that is both the first and the last, two window rows; 15 blocks per row, 14 windows: the last group has two
#   72x136    three bands, the last of 8 lines (4 block rows, 3 window rows)
#   200x152   49 blocks per row: 48 windows, 12 full groups
#   424x240 from 420x236: the SSD takes 420 columns but 240 rows, the average level divides by 424 x 240; 105 blocks, 104 windows
#   416x240   103 blocks, 102 windows: the last group has two
#   1920x1088 once, noise only: two tiles of windows per row, 17 bands
SIZES = [((64, 16), (64, 16)), ((72, 136), (72, 136)), ((200, 152), (200, 152)), ((424, 240), (420, 236)), ((416, 240), (416, 240))]
CONTENTS = ["noise", "equal", "extreme", "flatnoise"]
BIG = ((1920, 1088), (1920, 1088))
WIDE10 = ((1024, 1024), (1024, 1024))       # 10-bit, 0 against 1023: 1023^2 * 1024 * 1024 > 2^32 -- SSD partials kept in 32 bits for too long wrap


def plane_sets(depth):
    sets = [(c, o, name) for (c, o) in SIZES for name in CONTENTS] + [BIG + ("noise",)]
    if depth > 8:
        sets.append(WIDE10 + ("extreme",))
    return sets


def key_of(depth, coded, name):
    return "d%d/%dx%d/%s/" % (depth, coded[0], coded[1], name)


def dtype_of(depth):
    return np.uint16 if depth > 8 else np.uint8


def planes(depth, name, coded):
    """(source Y, Cb, Cr), (reconstruction Y, Cb, Cr) of the coded size.  The columns and rows beyond the original size carry contents of their own: a pass that reads
    where it should not gives another number."""
    w, h = coded
    top = (1 << depth) - 1
    rng = np.random.default_rng([depth, w, h, CONTENTS.index(name)])
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    if name == "noise":
        src = [rng.integers(0, top + 1, s) for s in shapes]; rec = [rng.integers(0, top + 1, s) for s in shapes]
    elif name == "equal":                   # SSD 0 -> 99.99; 8-bit: every SSIM term is exactly 1.0f
        src = [rng.integers(0, top + 1, s) for s in shapes]; rec = [p.copy() for p in src]
    elif name == "extreme":                 # the overflow case of pixel.cpp:678-680
        src = [np.zeros(s, np.int64) for s in shapes]; rec = [np.full(s, top, np.int64) for s in shapes]
    else:                                   # flat + small noise: variances and covariances are differences of nearly equal large numbers
        flat = top // 2 + 3
        src = [flat + rng.integers(-2, 3, s) for s in shapes]; rec = [flat + rng.integers(-2, 3, s) for s in shapes]
    dt = dtype_of(depth)
    return [np.ascontiguousarray(p, dtype=dt) for p in src], [np.ascontiguousarray(p, dtype=dt) for p in rec]


def padded(p, pad=8):
    """the plane inside a wider and taller buffer of guard samples; returns (buffer, element offset of sample (0,0), stride in samples).  The stride is odd: one row
    in four starts where four samples can be loaded at once, the others do not"""
    h, w = p.shape
    buf = np.full((h + 2 * pad, w + 2 * pad + 3), 0x25, p.dtype)
    buf[pad:pad + h, pad:pad + w] = p
    return buf, pad * buf.shape[1] + pad, buf.shape[1]


def padded_pair(src, rec):
    """source and reconstruction in buffers of one stride per plane kind, as the encoder keeps them"""
    s = [padded(p) for p in src]; r = [padded(p) for p in rec]
    assert s[1][2] == s[2][2] and all(a[2] == b[2] for a, b in zip(s, r))
    return s, r


def arr_md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def ssim_geometry(coded):
    """(blocks per row, block rows, [(first window row, window rows) per band]) -- processPostRow's bands (framefilter.cpp:692-711) in window rows"""
    w, h = coded
    wb, hb = (w - 2) >> 2, (h - 2) >> 2
    nb = (h + 63) >> 6
    bands = []
    for r in range(nb):
        min_pix = 64 * r - 10 if r else 2
        max_pix = h if r == nb - 1 else 64 * (r + 1) - 4
        bands.append(((min_pix - 2) >> 2, ((max_pix - min_pix) >> 2) - 1))
    return wb, hb, bands


class Values(C.Structure):      # x265amd_quality_values
    _fields_ = [("psnrY", C.c_double), ("psnrU", C.c_double), ("psnrV", C.c_double), ("psnr", C.c_double), ("ssim", C.c_double), ("avgLumaLevel", C.c_double),
                ("maxLumaLevel", C.c_uint32), ("ssimCnt", C.c_uint32)]


def _addr(buf, off):
    return buf.ctypes.data + off * buf.itemsize


def model_ssd(depth, src, rec, coded, org):
    lib = T.load_hip(depth).lib
    s, r = padded_pair(src, rec)
    sp = (C.c_void_p * 3)(*[_addr(b, o) for b, o, _ in s]); rp = (C.c_void_p * 3)(*[_addr(b, o) for b, o, _ in r])
    out = np.full(4, 0x5a5a5a5a, np.uint64)
    lib.x265amd_picture_ssd_model.argtypes = [C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    assert lib.x265amd_picture_ssd_model(sp, rp, s[0][2], s[1][2], coded[0], coded[1], org[0], org[1], out.ctypes.data) == 0
    assert out[3] == 0x5a5a5a5a
    return out[:3].copy()


def model_ssim(depth, src_y, rec_y, coded, want_blocks=True):
    """(bands as uint32 [n][2]: the float's bits and the count, block sums int32 [hb][wb][4])"""
    lib = T.load_hip(depth).lib
    (sb, so, st), (rb, ro, rt) = padded(src_y), padded(rec_y)
    wb, hb, geo = ssim_geometry(coded)
    bands = np.full((len(geo) + 1, 2), 0x5a5a5a5a, np.uint32)
    blocks = np.full(hb * wb * 4 + 4, 0x5a5a5a5a, np.int32)
    lib.x265amd_picture_ssim_model.argtypes = [C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.x265amd_picture_ssim_model(_addr(sb, so), _addr(rb, ro), st, coded[0], coded[1], bands.ctypes.data, blocks.ctypes.data if want_blocks else None) == 0
    assert (bands[-1] == 0x5a5a5a5a).all() and (blocks[-4:] == 0x5a5a5a5a).all()
    return bands[:-1].copy(), blocks[:-4].reshape(hb, wb, 4).copy()


def model_level(depth, src_y, org):
    """(max, sum) as uint64"""
    lib = T.load_hip(depth).lib
    sb, so, st = padded(src_y)
    out = np.full(3, 0x5a5a5a5a5a5a5a5a, np.uint64)
    lib.x265amd_luma_level_model.argtypes = [C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
    assert lib.x265amd_luma_level_model(_addr(sb, so), st, org[0], org[1], out.ctypes.data) == 0
    assert out[2] == 0x5a5a5a5a5a5a5a5a and int(out[1]) >> 32 == 0
    return np.array([int(out[1]) & 0xffffffff, out[0]], np.uint64)


def level_record(level):
    """x265amd_luma_level_record from (max, sum)"""
    return np.array([level[1], level[0]], np.uint64)


def finish(depth, ssd, bands, level, coded, org):
    lib = T.load_hip(depth).lib
    out = Values()
    lib.x265amd_quality_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Values)]
    keep = [None if a is None else np.ascontiguousarray(a) for a in (ssd, bands, None if level is None else level_record(level))]
    rc = lib.x265amd_quality_finish(*[None if a is None else a.ctypes.data for a in keep], coded[0], coded[1], org[0], org[1], C.byref(out))
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD_PATH)


def ssd_numpy(src, rec, coded, org):
    """quirk 1: the original width, every row of the coded height"""
    out = []
    for k in range(3):
        w = org[0] >> (1 if k else 0)
        d = src[k][:, :w].astype(np.int64) - rec[k][:, :w].astype(np.int64)
        out.append(int((d * d).sum()))
    return np.array(out, np.uint64)


@pytest.mark.parametrize("depth", [8, 10])
def test_models_equal_the_fixtures(depth, gold):
    """every model on every plane set: SSDs, the digest of the block sums, the bands' bit patterns and counts, the light levels -- all exact"""
    for coded, org, name in plane_sets(depth):
        src, rec = planes(depth, name, coded)
        key = key_of(depth, coded, name)
        ssd = model_ssd(depth, src, rec, coded, org)
        assert np.array_equal(ssd, gold[key + "ssd"]), (key, ssd, gold[key + "ssd"])
        assert np.array_equal(ssd, ssd_numpy(src, rec, coded, org)), key
        bands, blocks = model_ssim(depth, src[0], rec[0], coded)
        assert arr_md5(blocks) == str(gold[key + "block_md5"]), key
        assert np.array_equal(bands, gold[key + "bands"]), (key, bands, gold[key + "bands"])
        level = model_level(depth, src[0], org)
        assert np.array_equal(level, gold[key + "level"]), (key, level, gold[key + "level"])
        assert np.array_equal(model_ssim(depth, src[0], rec[0], coded, want_blocks=False)[0], bands), key


def test_fixture_holds_every_set(gold):
    for depth in (8, 10):
        for coded, org, name in plane_sets(depth):
            for part in ("ssd", "block_md5", "bands", "level"):
                assert key_of(depth, coded, name) + part in gold.files
    assert len(gold.files) == 4 * (len(plane_sets(8)) + len(plane_sets(10)))


def test_bands_tile_the_window_rows():
    """the bands' window rows follow one another from 0 to the last without gap or overlap, whatever the height; the counts add up to every window"""
    for h in list(range(16, 400, 8)) + [1080 + 8, 2160, 4320]:
        wb, hb, geo = ssim_geometry((64, h))
        at = 0
        for first, rows in geo:
            assert first == at and rows >= 1, (h, geo)
            at += rows
        assert at == hb - 1, (h, geo)
    assert ssim_geometry((64, 16))[2] == [(0, 2)] and ssim_geometry((72, 136))[2] == [(0, 13), (13, 16), (29, 3)]


@pytest.mark.parametrize("depth", [8, 10])
def test_original_size_and_padded_size(depth):
    """424x240 from 420x236: the SSD stops at column 420 but takes rows 236 .. 239; the light level stops at 420 x 236 and its average divides by 424 x 240"""
    coded, org = SIZES[3]
    src, rec = planes(depth, "noise", coded)
    ssd = model_ssd(depth, src, rec, coded, org)
    full = ssd_numpy(src, rec, coded, coded)
    cropped = []
    for k in range(3):
        w, h = org[0] >> (1 if k else 0), org[1] >> (1 if k else 0)
        d = src[k][:h, :w].astype(np.int64) - rec[k][:h, :w].astype(np.int64)
        cropped.append(int((d * d).sum()))
    assert all(cropped[k] < int(ssd[k]) < int(full[k]) for k in range(3))
    level = model_level(depth, src[0], org)
    part = src[0][:org[1], :org[0]].astype(np.int64)
    assert int(level[0]) == int(part.max()) and int(level[1]) == int(part.sum())
    v = finish(depth, ssd, None, level, coded, org)
    assert v.avgLumaLevel == float(int(level[1])) / (coded[0] * coded[1]) and v.maxLumaLevel == int(level[0])
    size = org[0] * org[1]
    top = 255 << (depth - 8)
    assert v.psnrY == 10.0 * math.log10(float(top) * top * size / float(int(ssd[0])))
    assert v.psnrU == 10.0 * math.log10(float(top) * top * size / 4.0 / float(int(ssd[1])))
    assert v.psnr == (v.psnrY * 6 + v.psnrU + v.psnrV) / 8 and v.ssim == 0.0 and v.ssimCnt == 0


@pytest.mark.parametrize("depth", [8, 10])
def test_equal_planes_give_99_99_and_one(depth):
    for coded, org in SIZES:
        src, rec = planes(depth, "equal", coded)
        ssd = model_ssd(depth, src, rec, coded, org)
        bands, _ = model_ssim(depth, src[0], rec[0], coded)
        assert not ssd.any()
        v = finish(depth, ssd, bands, None, coded, org)
        assert v.psnrY == v.psnrU == v.psnrV == v.psnr == 99.99
        if depth == 8:
            # integer variances and covariances: numerator and denominator are the same two floats, every term is exactly 1.0f and every band's float is its count
            assert np.array_equal(bands[:, 0].copy().view(np.float32), bands[:, 1].astype(np.float32)), (coded, bands)
            assert v.ssim == 1.0
        else:
            # all-float terms: (2 covar + c2) and (ss 64 + c2 - t) are the same number reached by different roundings.  About eight roundings of 2^-24 each, on
            # differences that are a third to a quarter of their operands for uniform noise: below 1e-5 of a term (the exact bits are the fixture's, above)
            assert abs(v.ssim - 1.0) < 1e-5 and v.ssim != 0.0
        wb, hb, _ = ssim_geometry(coded)
        assert v.ssimCnt == (wb - 1) * (hb - 1) and v.maxLumaLevel == 0 and v.avgLumaLevel == 0.0


@pytest.mark.parametrize("depth", [8, 10])
def test_quality_finish_on_hand_made_records(depth):
    coded, org = (64, 72), (60, 62)          # two bands
    top = 255 << (depth - 8)
    size = 60 * 62
    ssd = np.array([size, 0, 4 * size], np.uint64)          # mean squared error 1 in luma, 16 in Cr (a quarter of the samples)
    bands = np.array([[np.float32(0.75).view(np.uint32), 3], [np.float32(2.5).view(np.uint32), 2]], np.uint32)
    v = finish(depth, ssd, bands, np.array([777, 1000000], np.uint64), coded, org)
    assert v.psnrY == 10.0 * math.log10(float(top) * top * size / float(size)) and v.psnrU == 99.99
    assert v.psnrV == 10.0 * math.log10(float(top) * top * size / 4.0 / float(4 * size))
    assert v.psnr == (v.psnrY * 6 + v.psnrU + v.psnrV) / 8
    assert v.ssim == 3.25 / 5 and v.ssimCnt == 5
    assert v.maxLumaLevel == 777 and v.avgLumaLevel == 1000000 / (64.0 * 72.0)
    # the bands' floats go into a double one by one: 2^24 + 1 is not a float, but the double holds it
    big = np.array([[np.float32(16777216.0).view(np.uint32), 1], [np.float32(1.0).view(np.uint32), 1]], np.uint32)
    assert finish(depth, None, big, None, coded, org).ssim == 16777217.0 / 2
    lib = T.load_hip(depth).lib
    assert lib.x265amd_quality_finish(None, None, None, 64, 72, 60, 62, None) != 0
    assert lib.x265amd_quality_finish(None, None, None, 64, 60, 60, 60, C.byref(Values())) != 0         # a coded height that is no multiple of 8


@pytest.mark.parametrize("depth", [8, 10])
def test_models_refuse_bad_arguments(depth):
    lib = T.load_hip(depth).lib
    buf = np.zeros(64 * 64, dtype_of(depth))
    p3 = (C.c_void_p * 3)(buf.ctypes.data, buf.ctypes.data, buf.ctypes.data)
    out = np.zeros(64, np.uint64)
    lib.x265amd_picture_ssd_model.argtypes = [C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.x265amd_picture_ssim_model.argtypes = [C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.x265amd_picture_ssd_model(p3, p3, 64, 32, 64, 32, 64, 32, out.ctypes.data) == 0
    assert lib.x265amd_picture_ssd_model(p3, p3, 64, 32, 64, 32, 72, 32, out.ctypes.data) != 0          # original wider than coded
    assert lib.x265amd_picture_ssd_model(p3, p3, 32, 32, 64, 32, 64, 32, out.ctypes.data) != 0          # stride below the width
    assert lib.x265amd_picture_ssd_model(p3, p3, 64, 32, 64, 8, 64, 8, out.ctypes.data) != 0            # below 16 lines
    assert lib.x265amd_picture_ssim_model(buf.ctypes.data, buf.ctypes.data, 64, 64, 32, out.ctypes.data, None) == 0
    assert lib.x265amd_picture_ssim_model(buf.ctypes.data, None, 64, 64, 32, out.ctypes.data, None) != 0
    assert lib.x265amd_picture_ssim_model(buf.ctypes.data, buf.ctypes.data, 64, 60, 32, out.ctypes.data, None) != 0


@pytest.mark.parametrize("depth", [8, 10])
def test_host_half_under_the_sanitizers(depth, tmp_path):
    """tests/native/quality_model_check.cpp: a stand-alone program (host code only) that runs the models and finish on exactly sized planes under -fsanitize=address,undefined"""
    import subprocess
    exe = str(tmp_path / "quality_model_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DX265AMD_DEPTH=%d" % depth,
           "-I" + os.path.join(T.ROOT, "include"), os.path.join(T.ROOT, "tests", "native", "quality_model_check.cpp"), os.path.join(T.PKG_DIR, "host", "quality_model.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
