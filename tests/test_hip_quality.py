"""The device passes of the quality metrics -- x265amd_picture_ssd, x265amd_picture_ssim, x265amd_luma_level (csrc/quality_kernels.hip) -- in both library depths against
their host models and against tests/golden/quality_golden.npz (the reference library's own SSIM functions; see tests/test_quality.py, whose plane sets and helpers these
tests use).  Everything is exact: the 64-bit sums, every block's four sums, the bit patterns of the bands' ordered float32 sums, the window counts, the levels.
Planes lie in device memory inside guard samples at odd offsets -- the vector loads must fall back where a row is not aligned --, outputs lie between guard words that
must stay, and every pass is launched twice into the same record."""
import ctypes as C

import numpy as np
import pytest

import hevc_testlib as T
import test_quality as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(Q.GOLD_PATH)


def _lib(depth):
    lib = T.load_hip(depth).lib
    lib.x265amd_last_error.restype = C.c_char_p
    lib.x265amd_picture_ssd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.x265amd_picture_ssim.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
    lib.x265amd_luma_level.argtypes = [C.c_void_p, C.c_uint64, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
    return lib


def _to_device(buf):
    import torch
    return torch.from_numpy(buf.view(np.uint8).reshape(-1)).cuda()


def _guarded(nbytes):
    import torch
    return torch.full((nbytes + 16,), 0x5a, dtype=torch.uint8, device="cuda")


def _inner(t):
    raw = t.cpu().numpy()
    assert (raw[:8] == 0x5a).all() and (raw[-8:] == 0x5a).all(), "a pass wrote beside its output"
    return raw[8:-8]


def run_ssd(depth, src, rec, coded, org, launches=2):
    import torch
    lib = _lib(depth)
    s, r = Q.padded_pair(src, rec)
    ds, dr = [_to_device(b) for b, _, _ in s], [_to_device(b) for b, _, _ in r]
    sa = np.array([t.data_ptr() + o * b.itemsize for t, (b, o, _) in zip(ds, s)], np.uint64)
    ra = np.array([t.data_ptr() + o * b.itemsize for t, (b, o, _) in zip(dr, r)], np.uint64)
    out = _guarded(24)
    for _ in range(launches):
        assert lib.x265amd_picture_ssd(None, T._ptr(sa), T._ptr(ra), s[0][2], s[1][2], coded[0], coded[1], org[0], org[1], out.data_ptr() + 8) == 0, lib.x265amd_last_error()
    torch.cuda.synchronize()
    return _inner(out).view(np.uint64).copy()


def run_ssim(depth, src_y, rec_y, coded, launches=2, want_blocks=True):
    import torch
    lib = _lib(depth)
    (sb, so, st), (rb, ro, rt) = Q.padded(src_y), Q.padded(rec_y)
    d_s, d_r = _to_device(sb), _to_device(rb)
    wb, hb, geo = Q.ssim_geometry(coded)
    groups = (wb - 1 + 3) // 4
    bands, work, blocks = _guarded(8 * len(geo)), _guarded(4 * (hb - 1) * groups), _guarded(16 * hb * wb)
    for _ in range(launches):
        rc = lib.x265amd_picture_ssim(None, d_s.data_ptr() + so * sb.itemsize, d_r.data_ptr() + ro * rb.itemsize, st, coded[0], coded[1], bands.data_ptr() + 8, work.data_ptr() + 8,
                                      blocks.data_ptr() + 8 if want_blocks else 0)
        assert rc == 0, lib.x265amd_last_error()
    torch.cuda.synchronize()
    _inner(work)
    got_blocks = _inner(blocks)
    if not want_blocks:
        assert (got_blocks == 0x5a).all()
    return _inner(bands).view(np.uint32).reshape(len(geo), 2).copy(), got_blocks.view(np.int32).reshape(hb, wb, 4).copy()


def run_level(depth, src_y, org, launches=2):
    import torch
    lib = _lib(depth)
    sb, so, st = Q.padded(src_y)
    d_s = _to_device(sb)
    out = _guarded(16)
    for _ in range(launches):
        assert lib.x265amd_luma_level(None, d_s.data_ptr() + so * sb.itemsize, st, org[0], org[1], out.data_ptr() + 8) == 0, lib.x265amd_last_error()
    torch.cuda.synchronize()
    raw = _inner(out)
    assert not raw[12:].any()
    return np.array([int(raw[8:12].view(np.uint32)[0]), int(raw[:8].view(np.uint64)[0])], np.uint64)


def check_set(depth, coded, org, name, gold):
    src, rec = Q.planes(depth, name, coded)
    key = Q.key_of(depth, coded, name)
    ssd = run_ssd(depth, src, rec, coded, org)
    assert np.array_equal(ssd, Q.model_ssd(depth, src, rec, coded, org)) and np.array_equal(ssd, gold[key + "ssd"]), (key, ssd, gold[key + "ssd"])
    bands, blocks = run_ssim(depth, src[0], rec[0], coded)
    want_bands, want_blocks = Q.model_ssim(depth, src[0], rec[0], coded)
    assert np.array_equal(blocks, want_blocks), (key, np.argwhere(blocks != want_blocks)[:8])
    assert Q.arr_md5(blocks) == str(gold[key + "block_md5"]), key
    assert np.array_equal(bands, want_bands) and np.array_equal(bands, gold[key + "bands"]), (key, bands, gold[key + "bands"])
    level = run_level(depth, src[0], org)
    assert np.array_equal(level, Q.model_level(depth, src[0], org)) and np.array_equal(level, gold[key + "level"]), (key, level, gold[key + "level"])


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", Q.SIZES, ids=lambda s: "%dx%d" % s[0])
def test_hip_passes_equal_the_models_and_the_fixtures(size, depth, gold):
    coded, org = size
    for name in Q.CONTENTS:
        check_set(depth, coded, org, name, gold)


@pytest.mark.parametrize("depth", [8, 10])
def test_hip_passes_at_1920x1088(depth, gold):
    check_set(depth, Q.BIG[0], Q.BIG[1], "noise", gold)


def test_hip_ten_bit_extremes_at_1024x1024(gold):
    """0 against 1023 over a million samples: 1023^2 * 4105 passes 2^32, so a 32-bit partial may cover 4 104 samples at the most; every window's sums are the largest there are"""
    coded, org = Q.WIDE10
    check_set(10, coded, org, "extreme", gold)
    assert int(gold[Q.key_of(10, coded, "extreme") + "ssd"][0]) == 1023 * 1023 * 1024 * 1024


@pytest.mark.parametrize("depth", [8, 10])
def test_hip_one_launch_and_no_block_sums_give_the_same_bands(depth):
    coded, org = Q.SIZES[3]
    src, rec = Q.planes(depth, "noise", coded)
    twice, _ = run_ssim(depth, src[0], rec[0], coded)
    once, _ = run_ssim(depth, src[0], rec[0], coded, launches=1)
    bare, _ = run_ssim(depth, src[0], rec[0], coded, want_blocks=False)
    assert np.array_equal(once, twice) and np.array_equal(once, bare)
    assert np.array_equal(run_ssd(depth, src, rec, coded, org, launches=1), run_ssd(depth, src, rec, coded, org))
    assert np.array_equal(run_level(depth, src[0], org, launches=1), run_level(depth, src[0], org))


@pytest.mark.parametrize("depth", [8, 10])
def test_hip_passes_refuse_bad_arguments(depth):
    """refused before anything is launched"""
    lib = _lib(depth)
    a = np.array([4096, 4096, 4096], np.uint64)
    assert lib.x265amd_picture_ssd(None, T._ptr(a), T._ptr(a), 64, 32, 64, 32, 72, 32, 4096) != 0           # original wider than coded
    assert lib.x265amd_picture_ssd(None, T._ptr(a), T._ptr(a), 32768, 16384, 32768, 32, 32768, 32, 4096) != 0       # beyond the 32-bit partials' bound
    assert lib.x265amd_picture_ssd(None, T._ptr(a), T._ptr(a), 64, 32, 64, 32, 64, 32, None) != 0
    assert lib.x265amd_picture_ssim(None, 4096, 4096, 64, 64, 8, 4096, 4096, 0) != 0
    assert lib.x265amd_picture_ssim(None, 4096, 4096, 64, 64, 32, 4096, None, 0) != 0
    assert lib.x265amd_luma_level(None, 4096, 32, 64, 32, 4096) != 0                                          # stride below the width
    assert b"x265amd_luma_level" in lib.x265amd_last_error()
