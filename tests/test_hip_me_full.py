"""The exhaustive motion search (--me full, X265_FULL_SEARCH, reference motion.cpp:1422-1466) on the device: bit for bit
(mvx, mvy, cost) against the reference's own MotionEstimate for method 5 (tests/golden/me_full_golden.npz, cut by
tests/golden/make_me_full_golden.py from the job sets this file defines)."""
import os

import numpy as np
import pytest

import hevc_testlib as T

ME_FULL = 5
FLAG_STAR, FLAG_CHROMA, FLAG_FULL = 1, 2, 4         # X265AMD_ME_FLAG_* (include/x265amd.h)
GOLD_PATH = os.path.join(T.GOLDEN_DIR, "me_full_golden.npz")
RAND_SCENES = ((1, (5, -3)), (2, (-17, 9)))         # two of test_hip_me.SCENES
CHROMA_SCENE = (11, (6, -4))
_gold = []


def gold():
    if not _gold:
        _gold.append(np.load(GOLD_PATH))
    return _gold[0]


# ----------------------------------------------------------------------------------------------------------
# the job sets (shared with the fixture's generator)
# ----------------------------------------------------------------------------------------------------------
def rand_set(depth, seed, motion):
    """case 1: about 40 jobs of all PU sizes, ranges cut at the picture margin, areas of a few hundred candidates"""
    return T.me_make_planes(depth, seed, motion=motion), T.me_jobs(seed * 100 + 57, 40, motion=motion, methods=(ME_FULL,), submes=(0, 2, 3), merange=12)


def _job(x, y, w, h, mvmin, mvmax, mvp, subme=2, qp=28, mvc=(), method=ME_FULL):
    return dict(x=x, y=y, w=w, h=h, qp=qp, mvp=mvp, mvmin=mvmin, mvmax=mvmax, mvc=list(mvc), merange=12, method=method, subme=subme)


def degenerate_set(depth):
    """case 2: hand-made areas on scene 1, whose top-left quadrant moves by (5, -3)"""
    planes = T.me_make_planes(depth, 1, motion=(5, -3))
    jobs = [
        _job(32, 16, 16, 16, (5, -3), (5, -3), (20, -12)),                  # one candidate, the true motion
        _job(32, 16, 16, 16, (-9, 7), (-9, 7), (0, 0)),                     # one candidate; the zero vector of the predictor stage lies outside the area
        _job(32, 16, 16, 16, (2, 2), (2, 2), (9, 7), subme=0),              # one candidate, a quarter-pel predictor clipped onto it
        _job(32, 16, 8, 8, (5, -7), (5, 1), (8, -4)),                       # width 1, height 9
        _job(40, 24, 8, 8, (4, -7), (4, 1), (18, -10), subme=3),            # width 1 beside the true motion: the predictor stage's rounding decides
        _job(32, 16, 4, 8, (3, -5), (7, -1), (12, -8), subme=0),            # width 5
        _job(32, 16, 8, 4, (3, -5), (7, -1), (13, -9), subme=3),
        _job(80, 16, 16, 16, (-30, -4), (36, -2), (0, 0)),                  # width 67: more than one wavefront's worth in a row
        _job(0, 0, 64, 64, (-20, -4), (46, -2), (37, -11), subme=3),        # the same under the largest PU
        _job(32, 16, 32, 32, (-4, -12), (5, -3), (-8, -30)),                # the minimum in the last row and the last column
        _job(32, 16, 16, 16, (-4, -12), (5, -3), (-8, -30), subme=0, mvc=((-60, 12), (3, 3))),
        _job(16, 16, 12, 16, (5, -3), (9, 4), (30, 2), subme=2),            # the minimum in the first row and the first column
    ]
    return planes, jobs


def _periodic_planes(depth, kind):
    """case 3: plane pairs on which many candidates cost the same"""
    w, h, m = 256, 192, T.ME_MARGIN
    stride, rows = w + 2 * m, h + 2 * m
    dt = np.uint8 if depth == 8 else np.uint16
    if kind == "tiled":
        # a random 16x16 patch with period 8 along x and 16 along y; the current plane is the same plane moved by (8, 5), no noise: SAD 0 wherever mx % 8 == 0 and my % 16 == 5
        patch = np.random.default_rng(0x71E5).integers(0, 1 << depth, (16, 16))
        ref = np.tile(patch[:, :8], (rows // 16, stride // 8))
        assert ref.shape == (rows, stride)
        cur = np.roll(ref, (-5, -8), (0, 1))
    else:
        # flat, and the current plane 3 above it everywhere: only the vector's price and the raster order decide
        ref = np.full((rows, stride), 100 << (depth - 8))
        cur = ref + 3
    return np.ascontiguousarray(cur.astype(dt)).ravel(), np.ascontiguousarray(ref.astype(dt)).ravel(), stride, m * stride + m


def ties_set(depth, kind):
    planes = _periodic_planes(depth, kind)
    rng = np.random.default_rng(0x7135 + (kind == "flat"))
    sizes = [(16, 16), (8, 8), (32, 32), (16, 8), (8, 16), (4, 8), (8, 4), (64, 64), (32, 16), (12, 16), (16, 4), (24, 32)]
    jobs = []
    for i in range(24):
        w, h = sizes[i % len(sizes)]
        x = int(rng.integers(0, 4)) * 64 + int(rng.integers(0, (64 - w) // 4 + 1)) * 4
        y = int(rng.integers(0, 3)) * 64 + int(rng.integers(0, (64 - h) // 4 + 1)) * 4
        if kind == "tiled":
            # a full-pel predictor with x = 4 (mod 8): the columns of SAD 0 stand at equal distances on both sides of it
            mvp = (4 * (8 * int(rng.integers(-2, 3)) + 4), 4 * int(rng.integers(-9, 10)))
        else:
            # half- and quarter-pel predictors: the full-pel vectors on both sides of them cost the same
            mvp = (int(rng.integers(-40, 41)), int(rng.integers(-40, 41)))
            if i % 3 == 0: mvp = (mvp[0] | 2) & ~1, mvp[1]
            if i % 3 == 1: mvp = mvp[0], ((mvp[1] | 2) & ~1)
        mr = 12
        mn = ((mvp[0] >> 2) - mr, (mvp[1] >> 2) - mr)
        mx = ((mvp[0] >> 2) + mr, (mvp[1] >> 2) + mr)
        mvc = [(int(rng.integers(-60, 61)), int(rng.integers(-60, 61))) for _ in range(i % 3)]
        jobs.append(_job(x, y, w, h, mn, mx, mvp, subme=(0, 2, 3)[i % 3], qp=int(rng.integers(12, 46)), mvc=mvc))
    return planes, jobs


def window_set(depth):
    """case 4: case 1's first scene with merange 57 -- 8 jobs, two of them 64x64, whose areas with the block and the window's margins exceed 192 x 192"""
    seed, motion = RAND_SCENES[0]
    pool = [j for j in T.me_jobs(seed * 100 + 57, 120, motion=motion, methods=(ME_FULL,), submes=(0, 2, 3), merange=57) if j["merange"] == 57]
    big = [j for j in pool if (j["w"], j["h"]) == (64, 64)][:2]
    rest = [j for j in pool if (j["w"], j["h"]) != (64, 64)][:6]
    assert len(big) == 2 and len(rest) == 6
    return T.me_make_planes(depth, seed, motion=motion), big + rest


def chroma_set(depth):
    seed, motion = CHROMA_SCENE
    return T.me_make_yuv(depth, seed, motion=motion), T.me_jobs(seed * 100 + 57, 20, motion=motion, methods=(ME_FULL,), submes=(3, 4), merange=12)


def golden_sets(depth):
    """key -> (planes, jobs, chroma form) of everything me_full_golden.npz holds for `depth`"""
    out = {}
    for seed, motion in RAND_SCENES:
        out["mef/%d/rand/%d" % (depth, seed)] = rand_set(depth, seed, motion) + (False,)
    out["mef/%d/degenerate" % depth] = degenerate_set(depth) + (False,)
    for kind in ("tiled", "flat"):
        out["mef/%d/ties/%s" % (depth, kind)] = ties_set(depth, kind) + (False,)
    out["mef/%d/window" % depth] = window_set(depth) + (False,)
    out["mefc/%d/rand/%d" % (depth, CHROMA_SCENE[0])] = chroma_set(depth) + (True,)
    return out


def cut(L, planes, jobs, chroma):
    """the [n,3] results of `jobs` through the host library L (the reference's MotionEstimate)"""
    if chroma:
        cur, rp, stride, cstride, origin, corg = planes
        return T.me_run_host_c(L, cur, rp, stride, cstride, origin, corg, jobs)
    cur, rp, stride, origin = planes
    return T.me_run_host(L, cur, rp, stride, origin, jobs)


def scan_minima(planes, jobs, mvcost):
    """step 2 alone, by brute force: for every job (cheapest cost, number of candidates that attain it, the first of them in raster order -- y outer, x inner).
    mvcost(qp) -> the 2 * 65536 + 1 prices of that QP, difference 0 at [65536]"""
    cur, ref, stride, origin = planes
    cur2, ref2 = cur.reshape(-1, stride).astype(np.int64), ref.reshape(-1, stride).astype(np.int64)
    oy, ox = divmod(origin, stride)
    out = []
    for j in jobs:
        tab = mvcost(j["qp"]).astype(np.int64)
        blk = cur2[oy + j["y"]:oy + j["y"] + j["h"], ox + j["x"]:ox + j["x"] + j["w"]]
        (mnx, mny), (mxx, mxy) = j["mvmin"], j["mvmax"]
        area = ref2[oy + j["y"] + mny:oy + j["y"] + mxy + j["h"], ox + j["x"] + mnx:ox + j["x"] + mxx + j["w"]]
        sad = np.abs(np.lib.stride_tricks.sliding_window_view(area, blk.shape) - blk).sum(axis=(2, 3))
        px = tab[65536 + 4 * np.arange(mnx, mxx + 1) - j["mvp"][0]]
        py = tab[65536 + 4 * np.arange(mny, mxy + 1) - j["mvp"][1]]
        cost = sad + ((py[:, None] + px[None, :]) & 0xffff)
        at = np.argwhere(cost == cost.min())
        out.append((int(cost.min()), len(at), (mnx + int(at[0][1]), mny + int(at[0][0]))))
    return out


# ----------------------------------------------------------------------------------------------------------
# the tests
# ----------------------------------------------------------------------------------------------------------
def _same(want, got, jobs, what):
    bad = np.argwhere((want != got).any(axis=1))
    assert len(bad) == 0, "%s, job %d: %s want %s got %s" % (what, bad[0][0], jobs[int(bad[0][0])], want[int(bad[0][0])], got[int(bad[0][0])])


@pytest.fixture(scope="module", params=[8, 10])
def me(request):
    m = T.HipME(request.param)
    m.depth = request.param
    yield m
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", range(len(RAND_SCENES)))
def test_random_scenes(me, scene):
    seed, motion = RAND_SCENES[scene]
    (cur, rp, stride, origin), jobs = rand_set(me.depth, seed, motion)
    _same(gold()["mef/%d/rand/%d" % (me.depth, seed)], me.run(cur, rp, stride, origin, jobs, flags=FLAG_FULL), jobs, "scene %d" % seed)


@pytest.mark.gpu
def test_degenerate_areas(me):
    (cur, rp, stride, origin), jobs = degenerate_set(me.depth)
    _same(gold()["mef/%d/degenerate" % me.depth], me.run(cur, rp, stride, origin, jobs, flags=FLAG_FULL), jobs, "degenerate areas")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tiled", "flat"])
def test_ties_go_to_the_first_in_raster_order(me, kind):
    """many candidates attain the cheapest cost: the reference's strict `<` in raster order keeps the first of them, and keeps the predictor stage's vector when the
    area's cheapest only equals it"""
    planes, jobs = ties_set(me.depth, kind)
    tied = sum(1 for _, n, _ in scan_minima(planes, jobs, me.host_mvcost) if n >= 2)
    assert 3 * tied >= len(jobs), (tied, len(jobs))
    cur, rp, stride, origin = planes
    _same(gold()["mef/%d/ties/%s" % (me.depth, kind)], me.run(cur, rp, stride, origin, jobs, flags=FLAG_FULL), jobs, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("win", [(192, 192), (80, 80), (128, 96)])
def test_areas_larger_than_the_window(me, win):
    """merange 57: candidates whose block leaves the staged window are read from memory, the result is the same for every window size"""
    (cur, rp, stride, origin), jobs = window_set(me.depth)
    # with the margins x265amd_me_plan gives a window (6 left, 10 right, 6 above, 7 below) the 64x64 PUs' areas do not fit 192 x 192
    assert sum(1 for j in jobs if j["mvmax"][0] - j["mvmin"][0] + j["w"] + 16 > 192 or j["mvmax"][1] - j["mvmin"][1] + j["h"] + 13 > 192) >= 2
    _same(gold()["mef/%d/window" % me.depth], me.run(cur, rp, stride, origin, jobs, max_win=win, flags=FLAG_FULL), jobs, "window %dx%d" % win)


@pytest.mark.gpu
def test_flag_independence(me):
    """X265AMD_ME_FLAG_FULL only chooses the kernel: without it the second pass scans from memory; other methods' jobs in the same call keep their results"""
    seed, motion = RAND_SCENES[0]
    (cur, rp, stride, origin), jobs = rand_set(me.depth, seed, motion)
    full = jobs[:20]
    want = gold()["mef/%d/rand/%d" % (me.depth, seed)][:20]
    others = T.me_jobs(seed * 100 + 58, 20, motion=motion, methods=(T.ME_HEX, T.ME_STAR), submes=(2,))
    alone = me.run(cur, rp, stride, origin, others, flags=FLAG_STAR)
    for flags in (0, FLAG_FULL, FLAG_STAR):
        _same(want, me.run(cur, rp, stride, origin, full, flags=flags), full, "flags %d" % flags)
    mixed = [j for pair in zip(full, others) for j in pair]
    for flags in (FLAG_STAR | FLAG_FULL, FLAG_FULL, 0):
        got = me.run(cur, rp, stride, origin, mixed, flags=flags)
        _same(want, got[0::2], full, "mixed, flags %d" % flags)
        _same(alone, got[1::2], others, "the other methods' jobs, flags %d" % flags)


@pytest.mark.gpu
def test_chroma_satd_form(me):
    (cur, rp, stride, cstride, origin, corg), jobs = chroma_set(me.depth)
    _same(gold()["mefc/%d/rand/%d" % (me.depth, CHROMA_SCENE[0])], me.run_c(cur, rp, stride, cstride, origin, corg, jobs), jobs, "chroma SATD")
