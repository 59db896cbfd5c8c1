"""Histogram-based scene-cut detection (--hist-scenecut) below the encoder: the device pass x265amd_hist_scene_stats, its host model x265amd_hist_scene_model, and the host
half x265amd_hist_scene_finish / x265amd_hist_scene_change, against tests/golden/hist_scenecut_golden.npz -- cut by tests/golden/make_hist_scenecut_golden.py from the
reference's own LookaheadTLD::calculateHistogram and LookaheadTLD::calcVariance (libx265_ref8.so) with the loops round them restated in numpy, and from the reference
program's debug log and per-picture records for the clips of tests/test_encoder_hist_scenecut.py.

Without a GPU: the model's record against the reference's on every plane set below; finish and change against the fixtures on every clip, picture by picture; the
per-band (uint16_t) on a checkerboard; the 320x192 case where NUM64x64INPIC is 0.
On the GPU: the kernel's record against the model's and the fixture's, the optional quarter picture, two launches, a launch without the quarter picture."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import hevc_testlib as T

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "hist_scenecut_golden.npz")

# coded sizes (multiples of 8):
#   72x40     quarter 18x10: segments of 4x2 with remainders 2 and 2; chroma regions 9x5, one or two sampled rows and three columns
#   136x72    quarter 34x18: remainders 2 and 2, segments 8x4
#   416x240   quarter 104x60: no remainder; two row chunks per luma segment (15 rows, chunks of 8)
#   424x240   quarter 106x60: remainder 2 in width only
#   1920x1088 once, noise only: more blocks per band than a workgroup has lanes is not reached (240), many chunks are
SIZES = [(72, 40), (136, 72), (416, 240), (424, 240)]
CONTENTS = ["noise", "flat", "checker", "ramp"]
BIG = (1920, 1088)
PLANE_SETS = [(w, h, name) for (w, h) in SIZES for name in CONTENTS] + [BIG + ("noise",)]


def arr_md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def planes(name, w, h):
    """(Y, Cb, Cr) of the coded size"""
    rng = np.random.default_rng([w, h, CONTENTS.index(name)])
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    if name == "noise":
        y, u, v = rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h // 2, w // 2)), rng.integers(0, 256, (h // 2, w // 2))
    elif name == "flat":                   # every sample in one bin: the contention case
        y, u, v = np.full((h, w), 117), np.full((h // 2, w // 2), 128), np.full((h // 2, w // 2), 0)
    elif name == "checker":                # 0 / 255, period 1: the largest block variance there is
        y, u, v = 255 * ((xx + yy) & 1), 255 * ((cx + cy) & 1), 255 * ((cx + cy + 1) & 1)
    else:                                  # a horizontal ramp over the whole range: every segment column has bins of its own
        y, u, v = (xx * 255) // (w - 1) + 0 * yy, (cx * 255) // (w // 2 - 1) + 0 * cy, 255 - (cx * 255) // (w // 2 - 1) + 0 * cy
    return [np.ascontiguousarray(p, dtype=np.uint8) for p in (y, u, v)]


def half_plane(y):
    """Lowres::init's full-pel plane (frame_init_lowres_core's dst0) of a luma plane whose size is a multiple of 2"""
    a = y.astype(np.int32)
    s00, s10, s01, s11 = a[0::2, 0::2], a[1::2, 0::2], a[0::2, 1::2], a[1::2, 1::2]
    return ((((s00 + s10 + 1) >> 1) + ((s01 + s11 + 1) >> 1) + 1) >> 1).astype(np.uint8)


def record_bytes(h):
    return 16 * 3 * 256 * 4 + 16 * 3 * 8 + 3 * (h // 8) * 8


def parse_record(raw, h):
    raw = np.ascontiguousarray(raw).view(np.uint8)
    assert len(raw) == record_bytes(h)
    n = 16 * 3 * 256 * 4
    return dict(counts=raw[:n].view(np.uint32).reshape(16, 3, 256).copy(), sums=raw[n:n + 384].view(np.uint64).reshape(16, 3).copy(),
                bands=raw[n + 384:].view(np.uint64).reshape(3, h // 8).copy())


def padded(p, pad, fill=0xa5):
    """the plane inside a wider and taller buffer of guard bytes; returns (buffer, element offset of sample (0,0), stride)"""
    h, w = p.shape
    buf = np.full((h + 2 * pad, w + 2 * pad + 3), fill, np.uint8)
    buf[pad:pad + h, pad:pad + w] = p
    return buf, pad * buf.shape[1] + pad, buf.shape[1]


def model(pl, want_quarter=True):
    """x265amd_hist_scene_model on padded host planes: (record, quarter picture)"""
    lib = T.load_hip(8).lib
    h, w = pl[0].shape
    bufs = [padded(p, 4) for p in pl]
    hb, ho, hs = padded(half_plane(pl[0]), 2)
    assert bufs[1][2] == bufs[2][2]
    ptrs = (C.c_void_p * 3)(*[b.ctypes.data + o for b, o, _ in bufs])
    rec = np.full(record_bytes(h) + 8, 0x5a, np.uint8)
    q = np.full((h // 4, w // 4), 0x5a, np.uint8)
    lib.x265amd_hist_scene_model.argtypes = [C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rc = lib.x265amd_hist_scene_model(ptrs, bufs[0][2], bufs[1][2], hb.ctypes.data + ho, hs, w, h, rec.ctypes.data, q.ctypes.data if want_quarter else None)
    assert rc == 0
    assert (rec[-8:] == 0x5a).all()
    return parse_record(rec[:-8], h), q


class Pic(C.Structure):
    _fields_ = [("picHistogram", C.c_uint32 * (4 * 4 * 3 * 256)), ("averageIntensityPerSegment", C.c_uint8 * 48), ("averageIntensity", C.c_uint8 * 3),
                ("picAvgVariance", C.c_uint16), ("picAvgVarianceCb", C.c_uint16), ("picAvgVarianceCr", C.c_uint16)]


class State(C.Structure):
    _fields_ = [("avg", C.c_uint32 * 48), ("resetRunningAvg", C.c_int32), ("segmentCountThreshold", C.c_uint32)]


def record_raw(rec):
    return np.concatenate([rec["counts"].ravel().view(np.uint8), rec["sums"].ravel().view(np.uint8), rec["bands"].ravel().view(np.uint8)])


def finish(rec, w, h):
    lib = T.load_hip(8).lib
    raw = record_raw(rec)
    out = Pic()
    lib.x265amd_hist_scene_finish.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Pic)]
    assert lib.x265amd_hist_scene_finish(raw.ctypes.data, w, h, C.byref(out)) == 0
    return out


def pic_numbers(pic):
    """what the fixtures keep of a finished picture: the segment averages, the picture's averages and variances, and the histogram itself"""
    return dict(seg=np.frombuffer(bytes(pic.averageIntensityPerSegment), np.uint8).reshape(4, 4, 3).copy(), avg=np.array(list(pic.averageIntensity), np.uint8),
                var=np.array([pic.picAvgVariance, pic.picAvgVarianceCb, pic.picAvgVarianceCr], np.uint16), hist=np.frombuffer(bytes(pic.picHistogram), np.uint32).reshape(4, 4, 3, 256).copy())


def new_state():
    lib = T.load_hip(8).lib
    st = State()
    lib.x265amd_hist_scene_state_init.argtypes = [C.POINTER(State)]
    lib.x265amd_hist_scene_state_init.restype = None
    lib.x265amd_hist_scene_state_init(C.byref(st))
    return st


def change(prev, cur, nxt, w, h, st):
    """x265amd_hist_scene_change: (result, the 16 segment verdicts)"""
    lib = T.load_hip(8).lib
    v = (C.c_int32 * 16)()
    lib.x265amd_hist_scene_change.argtypes = [C.POINTER(Pic)] * 3 + [C.c_int, C.c_int, C.POINTER(State), C.c_void_p]
    r = lib.x265amd_hist_scene_change(C.byref(prev), C.byref(cur), C.byref(nxt), w, h, C.byref(st), v)
    return r, np.array(list(v), np.int32)


def clip_pictures(frames, w, h):
    """the finished pictures of a clip at its coded size (the pad replicates the last column / row, as the encoder's input does)"""
    W, H = (w + 7) & ~7, (h + 7) & ~7
    out = []
    for fr in frames:
        pl = [np.pad(fr[0], ((0, H - h), (0, W - w)), mode="edge")] + [np.pad(p, ((0, (H - h) // 2), (0, (W - w) // 2)), mode="edge") for p in fr[1:]]
        rec, _ = model(pl, want_quarter=False)
        out.append(finish(rec, W, H))
    return out, W, H


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD_PATH)


# ---- without a GPU ----
def test_model_equals_the_references_functions(gold):
    """the host model's record is what the reference's calculateHistogram and calcVariance give over the reference's loops, on every plane set"""
    for w, h, name in PLANE_SETS:
        rec, q = model(planes(name, w, h))
        key = "stats/%dx%d/%s/" % (w, h, name)
        for part in ("counts", "sums", "bands"):
            assert np.array_equal(rec[part], gold[key + part]), (w, h, name, part)
        assert np.array_equal(q, gold[key + "quarter"]), (w, h, name)
        # every sample of the quarter picture is counted once, every 4th chroma sample of every 4th row once
        assert int(rec["counts"][:, 0].sum()) == (w // 4) * (h // 4)
        assert int(rec["sums"][:, 0].sum()) == int(q.astype(np.int64).sum())
        if name == "flat":
            assert np.count_nonzero(rec["counts"][:, 0]) == 16 and np.count_nonzero(rec["counts"][:, 1]) == 16 and not rec["bands"].any()


def test_finish_truncates_every_band_of_a_checkerboard():
    """0 / 255 with period 1: an 8x8 block has sum 32 * 255 and ssd 32 * 255^2, variance 1040400; a band's quotient (W / 8) * 1040400 / W = 130050 does not fit
    sixteen bits, and the reference's (uint16_t) keeps 130050 - 65536 = 64514 of it per band: picAvgVariance = (H / 8) * 64514 / H"""
    for w, h in SIZES:
        rec, _ = model(planes("checker", w, h))
        assert (rec["bands"][0] == (w // 8) * 1040400).all()
        assert (rec["bands"][1:] == (w // 8) * (8 * 255 * 255 - ((8 * 255) ** 2 >> 4))).all()
        n = pic_numbers(finish(rec, w, h))
        assert (w // 8) * 1040400 // w == 130050
        assert n["var"][0] == ((h // 8) * (130050 - 65536) // h) & 0xffff
        cband = (w // 8) * 260100 // (w // 2)
        assert cband == 65025 and n["var"][1] == n["var"][2] == ((h // 8) * cband // (h // 2)) & 0xffff


def test_finish_bins_and_averages_by_hand():
    """a flat picture: one bin per segment and plane holds (1 + count) << 4, every other bin 16; the averages are the flat values (the reference's mixed-up
    width / height terms cancel where the segments have no remainder)"""
    w, h = 416, 240
    pl = planes("flat", w, h)
    n = pic_numbers(finish(model(pl)[0], w, h))
    assert (n["hist"][:, :, 0, 117] == (1 + 26 * 15) << 4).all() and (n["hist"][:, :, 1, 128] == (1 + 13 * 8) << 4).all() and (n["hist"][:, :, 2, 0] == (1 + 13 * 8) << 4).all()
    assert np.count_nonzero(n["hist"] != 16) == 48
    assert (n["seg"][:, :, 0] == 117).all() and n["avg"][0] == 117 and not n["var"].any()
    # chroma: 13 x 8 samples stand for a 104 x 60 / 4 region: (128 * 104 << 4) plus the rounding term, over 1560, is 137, not 128 -- the reference's quotient as spelt (13 x 8 samples are not a sixteenth of 52 x 30)
    assert (n["seg"][:, :, 1] == ((128 * 104 << 4) + (104 * 60 >> 3)) // (104 * 60 >> 2)).all() and (n["seg"][:, :, 2] == 0).all()


def _clips():
    import test_encoder_hist_scenecut as EH
    return EH


def test_finish_and_change_equal_the_reference_on_every_clip(gold):
    """picture by picture: the finished numbers are the fixture's (from the reference's functions), and the decisions -- made in display order, each picture with the one
    before and the one behind it, as the lookahead does -- are the ones the reference program logged (`Scene Change in Pic Number#`) and recorded (bScenecut)"""
    EH = _clips()
    for tag in EH.CLIPS:
        (w, h), _, _ = EH.CLIPS[tag]
        pics, W, H = clip_pictures(EH.clip_frames(tag), w, h)
        for k, pic in enumerate(pics):
            n = pic_numbers(pic)
            for part in ("seg", "avg", "var"):
                assert np.array_equal(n[part], gold["clip/%s/%s" % (tag, part)][k]), (tag, k, part)
            assert np.array_equal(n["hist"].sum(axis=(0, 1, 3)), gold["clip/%s/hist_sum" % tag][k]) and arr_md5(n["hist"]) == str(gold["clip/%s/hist_md5" % tag][k]), (tag, k)
        st = new_state()
        results, verdicts = [], []
        for k in range(1, len(pics) - 1):
            r, v = change(pics[k - 1], pics[k], pics[k + 1], W, H, st)
            results.append(r); verdicts.append(v)
        assert np.array_equal(np.array(results), gold["clip/%s/change" % tag]), (tag, results)
        assert np.array_equal(np.array(verdicts), gold["clip/%s/verdicts" % tag]), tag
        assert [k + 1 for k, r in enumerate(results) if r] == EH.CLIPS[tag][2], tag


def test_small_picture_has_zero_thresholds(gold):
    """320x192: a segment is 80x48, NUM64x64INPIC is 3840 >> 12 = 0 -- every threshold is 0 and any histogram difference above the running average's is abrupt.  The
    reference reports picture 6 of a clip whose content changes at 7"""
    EH = _clips()
    (w, h), _, cuts = EH.CLIPS["small"]
    assert (w, h) == (320, 192) and ((w // 4) * (h // 4)) >> 12 == 0 and cuts == [6]
    pics, W, H = clip_pictures(EH.clip_frames("small"), w, h)
    st = new_state()
    got = [change(pics[k - 1], pics[k], pics[k + 1], W, H, st)[0] for k in range(1, len(pics) - 1)]
    assert [k + 1 for k, r in enumerate(got) if r] == [6]


def test_state_starts_as_the_lookahead_object_does():
    st = new_state()
    assert not any(st.avg) and st.resetRunningAvg == 1 and st.segmentCountThreshold == 8


def test_ten_bit_library_refuses_the_model():
    lib = T.load_hip(10).lib
    buf = np.zeros(64 * 64, np.uint16)
    ptrs = (C.c_void_p * 3)(buf.ctypes.data, buf.ctypes.data, buf.ctypes.data)
    rec = np.zeros(record_bytes(32), np.uint8)
    lib.x265amd_hist_scene_model.argtypes = [C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.x265amd_hist_scene_model(ptrs, 64, 32, buf.ctypes.data, 32, 32, 32, rec.ctypes.data, None) != 0


# ---- on the GPU ----
def run_stats(pl, want_quarter=True, launches=1):
    """x265amd_hist_scene_stats on planes held in device memory inside guard bytes; the record and the quarter picture lie between guard words that must stay"""
    import torch
    lib = T.load_hip(8).lib
    h, w = pl[0].shape
    bufs = [padded(p, 4) for p in pl]
    hb, ho, hs = padded(half_plane(pl[0]), 2)
    d = [torch.from_numpy(b).cuda() for b, _, _ in bufs]
    d_half = torch.from_numpy(hb).cuda()
    addr = np.array([t.data_ptr() + o for t, (_, o, _) in zip(d, bufs)], np.uint64)
    nrec = record_bytes(h)
    d_rec = torch.full((nrec + 16,), 0x5a, dtype=torch.uint8, device="cuda")
    d_q = torch.full(((h // 4) * (w // 4) + 16,), 0x5a, dtype=torch.uint8, device="cuda")
    lib.x265amd_last_error.restype = C.c_char_p
    lib.x265amd_hist_scene_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_uint64, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p, C.c_uint64]
    for _ in range(launches):
        rc = lib.x265amd_hist_scene_stats(None, T._ptr(addr), bufs[0][2], bufs[1][2], d_half.data_ptr() + ho, hs, w, h, d_rec.data_ptr() + 8, d_q.data_ptr() + 8 if want_quarter else 0)
        assert rc == 0, lib.x265amd_last_error()
    torch.cuda.synchronize()
    rec, q = d_rec.cpu().numpy(), d_q.cpu().numpy()
    assert (rec[:8] == 0x5a).all() and (rec[-8:] == 0x5a).all() and (q[:8] == 0x5a).all() and (q[-8:] == 0x5a).all()          # nothing written beside the outputs
    if not want_quarter:
        assert (q == 0x5a).all()
    return parse_record(rec[8:-8], h), q[8:-8].reshape(h // 4, w // 4)


def same_record(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("counts", "sums", "bands"))


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_hip_record_equals_the_models_and_the_fixtures(size, gold):
    w, h = size
    for name in CONTENTS:
        pl = planes(name, w, h)
        want, want_q = model(pl)
        got, got_q = run_stats(pl)
        for part in ("counts", "sums", "bands"):
            assert np.array_equal(got[part], want[part]), (name, part, np.argwhere(got[part] != want[part])[:8])
            assert np.array_equal(got[part], gold["stats/%dx%d/%s/%s" % (w, h, name, part)]), (name, part)
        assert np.array_equal(got_q, want_q), (name, np.argwhere(got_q != want_q)[:8])


@pytest.mark.gpu
def test_hip_record_at_1920x1088(gold):
    w, h = BIG
    pl = planes("noise", w, h)
    got, got_q = run_stats(pl)
    for part in ("counts", "sums", "bands"):
        assert np.array_equal(got[part], gold["stats/%dx%d/noise/%s" % (w, h, part)]), part
    assert np.array_equal(got_q, gold["stats/%dx%d/noise/quarter" % (w, h)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noise", "flat"])
def test_hip_two_launches_and_no_quarter_plane_give_the_same_record(name):
    """the call zeroes the record it adds into: a second launch on the same buffers gives the same record; so does a call without the optional plane"""
    w, h = 424, 240
    pl = planes(name, w, h)
    once, _ = run_stats(pl)
    twice, _ = run_stats(pl, launches=2)
    bare, _ = run_stats(pl, want_quarter=False)
    assert same_record(once, twice) and same_record(once, bare) and same_record(once, model(pl)[0])
