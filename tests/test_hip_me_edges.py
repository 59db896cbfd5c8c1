"""The diamond, hexagon and star motion searches (csrc/me_dev.h: me_search, me_star_pattern) where their comparisons decide: equal costs, ranges thinner than the
pattern, clipped predictors and candidates, the largest costs.  Bit for bit (mvx, mvy, cost) against the reference's own MotionEstimate::motionEstimate
(tests/golden/me_edges_golden.npz, cut by tests/golden/make_me_edges_golden.py from the job sets this file defines), on every path a job can take on the device:
the inlined dia/hex kernel, the variant that carries the star search, the direct-from-memory second pass, windows too small for the areas, batches that mix the
methods and both chroma forms, and the job server's ME_SEARCH / ME_SEARCH_STAR / ME_DEFERRED commands.

The sets (each for 8 and 10 bits, at most 48 jobs per method, all 24 PU sizes, subme 0..7 in turn):
  mirror       a reference plane mirror-symmetric about every CTU's centre lines, and in every CTU a current plane that is the mean of four reference blocks
               displaced by (4a +- D, 4b +- E): a PU centred on (tile centre - (4a, 4b)) with the full-pel predictor (16a, 16b) sees SAD, SATD and the vector's
               price symmetric about its start vector, so left/right, up/down and the hexagon's diagonals cost the same at full, half and quarter sample, and
               with D or E != 0 the start is not the cheapest.  (a, b) belongs to the TILE here: the current block must be symmetric about the PU's own centre,
               which a tile symmetric about its own centre gives only for a = b = 0.  PU widths or heights of 4, 12 (no multiple of 8) cannot be centred on a
               position that is a multiple of 4: they tie along the other axis only.
               A second ring of displaced blocks in two CTUs makes the half hexagon after a horizontal step tie too; the candidates are one of the tied minima,
               pairs that mirror each other in x or in y, and (a != 0, no candidates) a range that ends 4 beyond the centre, which makes the zero vector the
               mirror image of the clipped predictor.
               Deciding ties (see deciding_ties) reached with the reference's price tables, of 48 jobs:  8 bits dia 27, hex 32, star 22;  10 bits dia 27, hex 32,
               star 23.  Sub-pel results: 81 of 144 at both depths.  With chroma planes, of 15 jobs: dia 8, hex 11, star 7 at both depths.
  price/*      the flat and the tiled plane pair of test_hip_me_full with half- and quarter-sample predictors, ranges wider (12, 57) and narrower (1, 2) than the
               pattern: equal distortion everywhere (flat) or on a lattice (tiled), only the vector's price and the order of the comparisons decide
  stripes/*    source 0 against stripes of 0 and pmax, a predictor half a sample between two full-pel vectors of equal cost that the predictor's own cost does
               not undercut: the start, its neighbour and (predictor (2, 0) / (0, 2)) the zero vector tie, and nothing merely equal may displace the start
  degenerate   hand-made ranges: one vector, one column and one row on either side of the true motion, the predictor outside on each side, the zero vector outside in
               x, in y, in both, merange 1, 2, 3 in ranges as small, merange 2, 3, 4, 6 in a range of +- 12 (the hexagon's loop count ends the search)
  raster       periodic planes with a start from which the star pattern finds its best point 8 away (star_first_distance proves it), so that the raster scan runs;
               range widths whose last columns fail `tx + 15 <= mvmax.x`; two jobs whose result hangs on the price of the scan's fourth column (8 tx, 8 ty)
  candidates   12 extra candidates: distinct, equal, one the predictor, one zero, one clipped onto the predictor, two clipped onto each other, the best first / last
  extremes/*   source 0 against reference pmax, and a pmax checkerboard (against itself and against its inverse): the largest SAD and SATD, QP 0, 51, 69,
               predictors 80 quarter samples off
  mirror-c     the mirror set with chroma planes built the same way at half size, subme 3..7, in the encoder's chroma-SATD form and (same jobs) in the luma form"""
import os

import numpy as np
import pytest

import hevc_testlib as T
import test_hip_me_full as MF

FLAG_STAR = 1                                      # X265AMD_ME_FLAG_* (include/x265amd.h)
GOLD_PATH = os.path.join(T.GOLDEN_DIR, "me_edges_golden.npz")
METHODS = (T.ME_DIA, T.ME_HEX, T.ME_STAR)
METHOD_NAME = {T.ME_DIA: "dia", T.ME_HEX: "hex", T.ME_STAR: "star"}
PIC_W, PIC_H = 256, 192
# the 24 PU sizes of T.me_jobs
SIZES = [(64, 64), (32, 32), (16, 16), (8, 8), (32, 16), (16, 32), (16, 8), (8, 16), (64, 32), (32, 64), (8, 4), (4, 8),
         (16, 12), (12, 16), (16, 4), (4, 16), (32, 24), (24, 32), (32, 8), (8, 32), (64, 48), (48, 64), (64, 16), (16, 64)]
# the first pattern around the start vector: dia's 4 points, hex's 6, star's 4 at distance 1
PATTERN = {T.ME_DIA: ((0, -1), (0, 1), (-1, 0), (1, 0)), T.ME_HEX: ((-2, 0), (-1, 2), (1, 2), (2, 0), (1, -2), (-1, -2)), T.ME_STAR: ((0, -1), (-1, 0), (1, 0), (0, 1))}
_gold = []


def gold():
    if not _gold:
        _gold.append(np.load(GOLD_PATH))
    return _gold[0]


# ----------------------------------------------------------------------------------------------------------
# the job sets (shared with the fixture's generator)
# ----------------------------------------------------------------------------------------------------------
def _job(x, y, w, h, mvmin, mvmax, mvp, method, subme, qp=28, mvc=(), merange=12):
    return dict(x=int(x), y=int(y), w=int(w), h=int(h), qp=int(qp), mvp=(int(mvp[0]), int(mvp[1])), mvmin=(int(mvmin[0]), int(mvmin[1])), mvmax=(int(mvmax[0]), int(mvmax[1])),
                mvc=[(int(a), int(b)) for a, b in mvc], merange=int(merange), method=int(method), subme=int(subme))


def _cut_range(x, y, w, h, mvp, mr):
    """setSearchRange (reference: search.cpp:2724-2768) as T.me_jobs does it: mvp +- merange in full samples, cut so that the block reaches at most 64 samples outside the picture"""
    lim = 64
    mn = (max((mvp[0] >> 2) - mr, -x - lim), max((mvp[1] >> 2) - mr, -y - lim))
    mx = (min((mvp[0] >> 2) + mr, PIC_W - x - w + lim), min((mvp[1] >> 2) + mr, PIC_H - y - h + lim))
    return mn, mx


def _checked(jobs):
    """what every set keeps to: a PU inside one CTU at a multiple of 4, a non-empty range whose blocks stay 64 samples or less outside the picture (the planes have
    96: room for the pattern's steps beyond the range in x and for the interpolation), at most 12 candidates, a QP of the price tables"""
    for j in jobs:
        assert j["x"] % 4 == 0 and j["w"] % 4 == 0 and j["h"] % 4 == 0 and (j["x"] & 63) + j["w"] <= 64 and (j["y"] & 63) + j["h"] <= 64, j
        assert 0 <= j["x"] and j["x"] + j["w"] <= PIC_W and 0 <= j["y"] and j["y"] + j["h"] <= PIC_H, j
        assert j["mvmin"][0] <= j["mvmax"][0] and j["mvmin"][1] <= j["mvmax"][1], j
        assert j["x"] + j["mvmin"][0] >= -64 and j["y"] + j["mvmin"][1] >= -64 and j["x"] + j["w"] + j["mvmax"][0] <= PIC_W + 64 and j["y"] + j["h"] + j["mvmax"][1] <= PIC_H + 64, j
        assert len(j["mvc"]) <= 12 and 0 <= j["qp"] < 70 and 0 <= j["subme"] <= 7 and j["method"] in METHODS, j
        assert all(abs(v) < 2048 for v in j["mvp"]) and all(abs(v) < 2048 for c in j["mvc"] for v in c), j
    return jobs


# ---- 1 and 6: mirror ties ----
# (D, E, a, b) of the 12 CTUs, row by row; a fifth entry (D2, E2) adds a second ring of displaced blocks at twice the weight: the hexagon's first step goes to
# (+-D, 0), and its next half hexagon finds (+-D2, -E2) and (+-D2, +E2) tied below it
MIRROR_TILES = [(2, 0, 0, 0), (1, 2, 1, 0), (3, 0, 0, -1), (2, 0, -1, 1, (3, 2)),
                (1, 0, 0, 0), (0, 1, 1, -1), (1, 1, -1, 0), (0, 2, 0, 1),
                (1, 0, 1, 1), (5, 5, 0, 0), (4, 0, -1, -1), (2, 0, 0, 0, (3, 2))]
MIRROR_TILES_OF = {T.ME_HEX: (0, 1, 2, 3, 9, 11), T.ME_DIA: (4, 5, 6, 7, 8, 9), T.ME_STAR: (4, 5, 6, 7, 8, 9, 10, 1)}


def _mirror_pair(depth, seed, period, width, height, margin):
    """(cur, ref) as 2-D int arrays with margins: sample (x, y) of the reference is N[f(y), f(x)], f(u) = min(u mod period, period - 1 - u mod period)"""
    rng = np.random.default_rng(seed)
    n = period // 2
    tab = rng.integers(0, 1 << depth, (n, n)).astype(np.int64)
    tab = (2 * tab + np.roll(tab, 1, 0) + np.roll(tab, 1, 1) + 2) >> 2          # lightly smoothed: the sub-sample positions have something to follow
    fx = np.arange(-margin, width + margin) % period
    fy = np.arange(-margin, height + margin) % period
    ref = tab[np.minimum(fy, period - 1 - fy)[:, None], np.minimum(fx, period - 1 - fx)[None, :]]
    assert ref.shape[0] % period == 0 and ref.shape[1] % period == 0            # np.roll below wraps onto the same pattern
    r = lambda dx, dy: np.roll(ref, (-dy, -dx), (0, 1))
    cur = ref.copy()
    s = period // 16        # 4 for luma, 2 for chroma: the predictor (16a, 16b) in samples of this plane
    for k, tile in enumerate(MIRROR_TILES):
        D, E, a, b = tile[:4]
        y0, x0 = margin + (k // 4) * period, margin + (k % 4) * period
        four = lambda D, E: r(s * a + D, s * b + E) + r(s * a - D, s * b + E) + r(s * a + D, s * b - E) + r(s * a - D, s * b - E)
        mean = (four(D, E) + 2) >> 2 if len(tile) == 4 else (four(D, E) + 2 * four(*tile[4]) + 6) // 12
        cur[y0:y0 + period, x0:x0 + period] = mean[y0:y0 + period, x0:x0 + period]
    return cur, ref


def _flat(a, depth):
    return np.ascontiguousarray(a.astype(np.uint8 if depth == 8 else np.uint16)).ravel()


def mirror_planes(depth):
    m = T.ME_MARGIN
    cur, ref = _mirror_pair(depth, 0x3117, 64, PIC_W, PIC_H, m)
    stride = PIC_W + 2 * m
    return _flat(cur, depth), _flat(ref, depth), stride, m * stride + m


def mirror_yuv(depth):
    """the mirror planes with chroma planes built the same way at half size: the layout of T.me_make_yuv"""
    cy, ry, stride, origin = mirror_planes(depth)
    cm = T.ME_MARGIN // 2
    cu, ru = _mirror_pair(depth, 0x3118, 32, PIC_W // 2, PIC_H // 2, cm)
    cv, rv = _mirror_pair(depth, 0x3119, 32, PIC_W // 2, PIC_H // 2, cm)
    cstride = PIC_W // 2 + 2 * cm
    return [cy, _flat(cu, depth), _flat(cv, depth)], [ry, _flat(ru, depth), _flat(rv, depth)], stride, cstride, origin, cm * cstride + cm


def _mirror_jobs(seed, per_method, submes):
    rng = np.random.default_rng(seed)
    jobs = []
    for method in METHODS:
        for i in range(per_method):
            w, h = SIZES[i % len(SIZES)]
            # a PU of 64 cannot leave the CTU's centre
            fit = [k for k in MIRROR_TILES_OF[method] if (w < 64 or MIRROR_TILES[k][2] == 0) and (h < 64 or MIRROR_TILES[k][3] == 0)]
            k = fit[(i + i // len(SIZES)) % len(fit)]
            D, E, a, b = MIRROR_TILES[k][:4]
            x = 64 * (k % 4) + ((32 - w // 2) & ~3) - 4 * a
            y = 64 * (k // 4) + ((32 - h // 2) & ~3) - 4 * b
            mvp = (16 * a, 16 * b)
            mr = (57, 16, 8, 57, 24)[i % 5]
            mn, mx = _cut_range(x, y, w, h, mvp, mr)
            if i % 4 == 0:
                mvc = []
                # the range ends 4 beyond the centre: the clipped predictor (8a, 8b) and the zero vector mirror each other, equal in SAD and in price
                if a > 0: mn = (8, mn[1])
                if a < 0: mx = (-8, mx[1])
                if a and b > 0: mn = (mn[0], 8)
                if a and b < 0: mx = (mx[0], -8)
            elif i % 4 == 1:    # one of the tied full-pel minima: the pattern search ends on it or on its mirror image at the same cost
                mvc = [(16 * a + 4 * D, 16 * b + 4 * E)]
            elif i % 4 == 2:    # two candidates that mirror each other in x, a quarter sample inside the minima
                mvc = [(16 * a + 4 * D - 1, 16 * b + 4 * E), (16 * a - 4 * D + 1, 16 * b + 4 * E)]
            else:               # two that mirror each other in y, a half sample outside
                mvc = [(16 * a + 4 * D, 16 * b - 4 * E - 2), (16 * a + 4 * D, 16 * b + 4 * E + 2)]
            jobs.append(_job(x, y, w, h, mn, mx, mvp, method, submes[(i + i // len(SIZES)) % len(submes)], qp=int(rng.integers(0, 70)), mvc=mvc, merange=mr))
    return _checked(jobs)


def mirror_set(depth):
    return mirror_planes(depth), _mirror_jobs(0x3120, 48, tuple(range(8)))


def mirror_chroma_set(depth):
    return mirror_yuv(depth), _mirror_jobs(0x3121, 15, (3, 4, 5, 6, 7))


# ---- 2: price-only ties ----
def price_set(depth, kind):
    planes = MF._periodic_planes(depth, kind)
    rng = np.random.default_rng(0x9A1C + (kind == "flat"))
    jobs = []
    for method in METHODS:
        for i in range(24):
            w, h = SIZES[i]
            x = int(rng.integers(0, 4)) * 64 + int(rng.integers(0, (64 - w) // 4 + 1)) * 4
            y = int(rng.integers(0, 3)) * 64 + int(rng.integers(0, (64 - h) // 4 + 1)) * 4
            if kind == "tiled":     # around x = 4 (mod 8): the columns of SAD 0 stand at equal distances on both sides
                mvp = [4 * (8 * int(rng.integers(-2, 3)) + 4), 4 * int(rng.integers(-9, 10))]
            else:
                mvp = [int(rng.integers(-40, 41)), int(rng.integers(-40, 41))]
            # half-sample in x, half-sample in y, quarter-sample in both: the full-pel vectors on both sides of them cost the same
            if i % 3 == 0: mvp[0] = (mvp[0] | 2) & ~1
            if i % 3 == 1: mvp[1] = (mvp[1] | 2) & ~1
            if i % 3 == 2: mvp = [mvp[0] | 1, mvp[1] | 1]
            mr = (12, 1, 57, 2)[i % 4]
            mn, mx = _cut_range(x, y, w, h, mvp, mr)
            mvc = [(int(rng.integers(-60, 61)), int(rng.integers(-60, 61))) for _ in range(i % 3)]
            jobs.append(_job(x, y, w, h, mn, mx, mvp, method, (i + method) % 8, qp=int(rng.integers(0, 70)), mvc=mvc, merange=mr))
    return planes, _checked(jobs)


# ---- 3: degenerate ranges ----
def degenerate_set(depth):
    """hand-made ranges on scene 1, whose top-left quadrant moves by (5, -3); every entry once per method"""
    planes = T.me_make_planes(depth, 1, motion=(5, -3))
    specs = [   # x, y, w, h, mvmin, mvmax, mvp, merange
        (32, 16, 16, 16, (5, -3), (5, -3), (20, -12), 12),          # mvmin == mvmax: the true motion
        (32, 16, 16, 16, (-9, 7), (-9, 7), (0, 0), 12),             # mvmin == mvmax, the zero vector outside in x and y
        (32, 16, 16, 16, (2, 2), (2, 2), (9, 7), 12),               # mvmin == mvmax, a quarter-sample predictor clipped onto it
        (32, 16, 8, 8, (5, -9), (5, 3), (20, -14), 12),             # one column: the pattern's points left and right of it are never tested against x
        (40, 24, 8, 8, (4, -9), (4, 3), (18, -10), 12),             # one column beside the true motion
        (32, 16, 16, 8, (-3, -3), (12, -3), (6, -12), 12),          # one row: the y tests reject every point above and below
        (32, 16, 32, 32, (-3, -2), (12, -2), (22, -9), 12),         # one row beside the true motion
        (32, 16, 16, 16, (2, -8), (10, 2), (-30, -12), 12),         # the predictor left of the range
        (32, 16, 16, 16, (2, -8), (10, 2), (90, -12), 12),          # right of it
        (32, 16, 8, 16, (2, -8), (10, 2), (20, -70), 12),           # above it
        (32, 16, 16, 8, (2, -8), (10, 2), (20, 50), 12),            # below it
        (0, 0, 64, 64, (2, -8), (10, 2), (-33, 47), 12),            # left and below, quarter-sample
        (32, 16, 16, 16, (3, -6), (9, 4), (20, -12), 12),           # the zero vector outside in x only
        (32, 16, 16, 16, (-4, -9), (8, -1), (20, -12), 12),         # outside in y only (above the zero row)
        (32, 16, 12, 16, (-4, 2), (8, 9), (10, 20), 12),            # outside in y only (below the zero row): by = mvmin.y
        (32, 16, 16, 16, (2, -9), (9, -1), (20, -12), 12),          # outside in both
        (32, 16, 16, 16, (4, -4), (6, -2), (20, -12), 1),           # merange 1: the hexagon's loop count (merange >> 1) - 1 is -1
        (32, 16, 24, 32, (3, -5), (7, -1), (12, -4), 2),            # merange 2: 0
        (32, 16, 16, 16, (2, -6), (8, 0), (8, -4), 3),              # merange 3: 0
        (32, 16, 4, 8, (3, -5), (7, -1), (21, -11), 2),
        (32, 16, 16, 16, (-8, -15), (16, 9), (0, -12), 2),          # merange 2, 3, 4, 6 in a range of +- 12 with the true motion 5 or more away: the loop count alone ends the hexagon
        (32, 16, 16, 16, (-8, -15), (16, 9), (0, -12), 3),
        (32, 16, 16, 16, (-8, -15), (16, 9), (40, -12), 4),
        (32, 16, 32, 32, (-8, -15), (16, 9), (20, 16), 6),
        (32, 16, 8, 8, (6, -9), (6, 3), (24, -14), 12),             # one column right of the true motion: the cheaper points lie left of it
        (32, 16, 16, 16, (7, -9), (7, 3), (28, -12), 12),
        (32, 16, 16, 16, (3, -9), (3, 3), (12, -12), 12),           # and left of it
        (32, 16, 16, 16, (-3, -4), (12, -4), (20, -16), 12),        # one row above the true motion
        (32, 16, 8, 16, (-3, -1), (12, -1), (20, -4), 12),          # and two below it
    ]
    jobs = []
    for method in METHODS:
        for i, (x, y, w, h, mn, mx, mvp, mr) in enumerate(specs):
            jobs.append(_job(x, y, w, h, mn, mx, mvp, method, (i + method) % 8, qp=(28, 0, 51, 69, 37)[i % 5], merange=mr))
    return planes, _checked(jobs)


# ---- 3, last item: the star search's raster scan ----
def raster_set(depth):
    """planes of period 8 along x and 16 along y, the current one moved by (8, 8): SAD 0 wherever mx % 8 == 0 and my % 16 == 8, and the same SAD at all vectors of
    equal residues.  A start of residues (0, 0) has its nearest such vectors exactly 8 above and 8 below, and the zero vector (same residues, a price on top) never
    takes its place: the star pattern ends with bDistance 8 > RasterDistance (star_first_distance), and the raster scan runs over a range whose width leaves 1 to
    3 single columns"""
    m = T.ME_MARGIN
    stride, rows = PIC_W + 2 * m, PIC_H + 2 * m
    patch = np.random.default_rng(0x7A57).integers(0, 1 << depth, (16, 8))
    ref = np.tile(patch, (rows // 16, stride // 8))
    assert ref.shape == (rows, stride)
    planes = (_flat(np.roll(ref, (-8, -8), (0, 1)), depth), _flat(ref, depth), stride, m * stride + m)
    sizes = [(16, 16), (8, 8), (32, 32), (64, 64), (16, 8), (8, 16), (32, 16), (4, 16), (12, 16), (24, 32)]
    starts = [(0, 0), (8, 16), (-8, 0), (0, 16), (8, 0), (-8, 16), (-16, 0), (16, 0), (0, -16), (8, -16)]
    jobs = []
    for method in METHODS:
        for i, ((w, h), (sx, sy)) in enumerate(zip(sizes, starts)):
            x = 64 * (1 + i % 2) + (((64 - w) // 8) & ~3)
            y = 64 + (((64 - h) // 8) & ~3)
            mn, mx = (sx - 57 + i % 5, sy - 57), (sx + 57 - i % 3, sy + 57 - i % 2)
            jobs.append(_job(x, y, w, h, mn, mx, (4 * sx, 4 * sy), method, (i + method) % 8, qp=(30, 12, 45, 0, 51)[i % 5], merange=57))
        # the scan's fourth column of every four is priced at (8 tx, 8 ty) (motion.cpp:1221).  Start (16, 16), columns -27 + 5i, rows -27 + 5j: the only vectors of
        # SAD 0 on that grid are (8, 8) and (48, 8), and (8, 8) is column i = 7, a fourth one: priced as (64, 64), the predictor itself, it undercuts the pattern's
        # (16, 8) / (16, 24); priced as the other columns are it would not
        for i, (w, h) in enumerate(((16, 16), (32, 32))):
            jobs.append(_job(64 + 16 * i, 64 + 8 * i, w, h, (-27, -27), (73, 70), (64, 64), method, (3 * i + method) % 8, qp=(24, 36)[i], merange=57))
    return planes, _checked(jobs)


# ---- 4: candidates ----
def candidates_set(depth):
    """12 extra candidates on scene 2, whose top-left quadrant moves by (-17, 9); the range is the predictor's +- 12"""
    motion = (-17, 9)
    planes = T.me_make_planes(depth, 2, motion=motion)
    rng = np.random.default_rng(0xCA4D)
    true = (4 * motion[0], 4 * motion[1])
    jobs = []
    for method in METHODS:
        for i in range(16):
            w, h = SIZES[(3 * i + method) % len(SIZES)]
            x = int(rng.integers(0, 2)) * 64 + int(rng.integers(0, (64 - w) // 4 + 1)) * 4
            y = int(rng.integers(0, (64 - h) // 4 + 1)) * 4
            mvp = (true[0] + int(rng.integers(-14, 15)), true[1] + int(rng.integers(-14, 15)))
            mr = 12
            mn, mx = _cut_range(x, y, w, h, mvp, mr)
            qmn, qmx = (4 * mn[0], 4 * mn[1]), (4 * mx[0], 4 * mx[1])
            far = lambda: (int(rng.integers(-60, 61)) + true[0], int(rng.integers(-60, 61)) + true[1])
            mvc = [far() for _ in range(12)]
            kind = i % 8
            if kind == 0:       # all distinct
                assert len(set(mvc)) == 12
            elif kind == 1:     # all equal
                mvc = [mvc[0]] * 12
            elif kind == 2:     # one equal to the predictor
                mvc[5] = mvp
            elif kind == 3:     # one zero
                mvc[7] = (0, 0)
            elif kind == 4:     # one that clips onto the (clipped) predictor: the predictor beyond the range's corner, the candidate further out
                mvp = (qmx[0] + 9, qmn[1] - 6)
                mvc[3] = (qmx[0] + 120, qmn[1] - 77)
            elif kind == 5:     # two that clip onto each other, beyond the opposite corner
                mvc[2] = (qmn[0] - 50, qmx[1] + 13)
                mvc[9] = (qmn[0] - 3, qmx[1] + 90)
            elif kind == 6:     # the best candidate first
                mvc[0] = true
            else:               # the best candidate last
                mvc[11] = true
            jobs.append(_job(x, y, w, h, mn, mx, mvp, method, (i + method) % 8, qp=int(rng.integers(0, 70)), mvc=mvc, merange=mr))
    return planes, _checked(jobs)


# ---- 5: extremes ----
def extremes_set(depth, kind):
    pmax = (1 << depth) - 1
    m = T.ME_MARGIN
    stride, rows = PIC_W + 2 * m, PIC_H + 2 * m
    yy, xx = np.mgrid[0:rows, 0:stride]
    if kind == "saturated":     # the largest SAD and the largest DC of the SATD at every vector
        ref = np.full((rows, stride), pmax)
        cur = np.zeros((rows, stride), np.int64)
    else:                       # a checkerboard of 0 and pmax: against its inverse in the left half of the picture (vectors of even x + y cost the most, odd ones nothing),
        ref = ((xx + yy) & 1) * pmax                                            # against itself in the right half; the interpolation filters run at their extremes
        cur = np.where(xx < stride // 2, pmax - ref, ref)
    planes = (_flat(cur, depth), _flat(ref, depth), stride, m * stride + m)
    rng = np.random.default_rng(0xE87E + (kind == "saturated"))
    sizes = [(64, 64), (64, 64), (32, 32), (16, 16), (8, 8), (64, 32), (32, 64), (8, 4), (4, 8), (16, 12), (48, 64), (24, 32)]
    jobs = []
    for method in METHODS:
        for i, (w, h) in enumerate(sizes):
            x = int(rng.integers(0, 4)) * 64 + int(rng.integers(0, (64 - w) // 4 + 1)) * 4
            y = int(rng.integers(0, 3)) * 64 + int(rng.integers(0, (64 - h) // 4 + 1)) * 4
            # 80 quarter samples off the zero vector, with a few quarter samples of scatter
            mvp = ((80, -80)[i & 1] + int(rng.integers(-5, 6)), (80, -80)[(i >> 1) & 1] + int(rng.integers(-5, 6)))
            mr = (57, 12)[i % 2]
            mn, mx = _cut_range(x, y, w, h, mvp, mr)
            mvc = [(int(rng.integers(-90, 91)), int(rng.integers(-90, 91))) for _ in range(i % 3)]
            jobs.append(_job(x, y, w, h, mn, mx, mvp, method, (i + method) % 8, qp=(0, 51, 69)[i % 3], mvc=mvc, merange=mr))
    return planes, _checked(jobs)


# ---- 2b: ties with the start itself ----
def stripes_set(depth, kind):
    """source 0 against stripes of 0 and pmax one sample wide, vertical ("v") or horizontal ("h"), with a predictor half a sample between two full-pel vectors and a
    small QP.  Both full-pel vectors see half the samples at pmax -- the same SAD -- and the same price; the half-sample position between them interpolates to
    (pmax + 1) / 2 everywhere, a SAD half a unit per sample above theirs, so the predictor's own cost does not undercut them.  The start (the predictor rounded up)
    therefore meets its equal in its left / upper neighbour, and for the predictors (2, 0) / (0, 2) in the zero vector: nothing equal may displace it"""
    pmax = (1 << depth) - 1
    m = T.ME_MARGIN
    stride, rows = PIC_W + 2 * m, PIC_H + 2 * m
    yy, xx = np.mgrid[0:rows, 0:stride]
    ref = ((xx if kind == "v" else yy) & 1) * pmax
    planes = (_flat(np.zeros_like(ref), depth), _flat(ref, depth), stride, m * stride + m)
    rng = np.random.default_rng(0x5791 + (kind == "v"))
    sizes = [(16, 16), (8, 8), (32, 32), (64, 64), (16, 8), (8, 16), (32, 16), (16, 32), (64, 32), (32, 64), (24, 32), (16, 12)]
    jobs = []
    for method in METHODS:
        for i, (w, h) in enumerate(sizes):
            x = int(rng.integers(0, 4)) * 64 + int(rng.integers(0, (64 - w) // 4 + 1)) * 4
            y = int(rng.integers(0, 3)) * 64 + int(rng.integers(0, (64 - h) // 4 + 1)) * 4
            k, n = (0, 0) if i % 3 == 0 else (int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
            mvp = (4 * k + 2, 4 * n) if kind == "v" else (4 * n, 4 * k + 2)
            mr = (12, 57, 3)[(i // 3) % 3]
            mn, mx = _cut_range(x, y, w, h, mvp, mr)
            jobs.append(_job(x, y, w, h, mn, mx, mvp, method, (i + method) % 8, qp=(0, 4, 9, 2)[i % 4], merange=mr))
    return planes, _checked(jobs)


LUMA_SETS = {"mirror": mirror_set, "stripes/v": lambda d: stripes_set(d, "v"), "stripes/h": lambda d: stripes_set(d, "h"), "price/flat": lambda d: price_set(d, "flat"), "price/tiled": lambda d: price_set(d, "tiled"), "degenerate": degenerate_set,
             "raster": raster_set, "candidates": candidates_set, "extremes/saturated": lambda d: extremes_set(d, "saturated"),
             "extremes/checkerboard": lambda d: extremes_set(d, "checkerboard")}
_sets = {}


def luma_set(depth, name):
    """(planes, jobs) of a set, built once: nothing changes them"""
    if (depth, name) not in _sets:
        _sets[depth, name] = LUMA_SETS[name](depth)
    return _sets[depth, name]


def chroma_set(depth):
    if (depth, "mirror-c") not in _sets:
        _sets[depth, "mirror-c"] = mirror_chroma_set(depth)
    return _sets[depth, "mirror-c"]


def luma_of(planes):
    cur, ref, stride, cstride, origin, corg = planes
    return cur[0], ref[0], stride, origin


def golden_sets(depth):
    """key -> (planes, jobs, chroma form) of everything me_edges_golden.npz holds for `depth`"""
    out = {"mee/%d/%s" % (depth, name): luma_set(depth, name) + (False,) for name in LUMA_SETS}
    planes, jobs = chroma_set(depth)
    out["meec/%d/mirror" % depth] = (planes, jobs, True)
    out["mee/%d/mirror-c" % depth] = (luma_of(planes), jobs, False)         # the same jobs without chroma SATD: the other half of a mixed batch
    return out


# ----------------------------------------------------------------------------------------------------------
# what makes a set worth its name, by brute force
# ----------------------------------------------------------------------------------------------------------
def _fullpel_cost(planes, j, mvcost):
    """cost(mx, my) = SAD + price of a full-pel vector of job j.  mvcost(qp) -> the 2 * 65536 + 1 prices of that QP, difference 0 at [65536]"""
    cur, ref, stride, origin = planes
    cur2, ref2 = cur.reshape(-1, stride).astype(np.int64), ref.reshape(-1, stride).astype(np.int64)
    oy, ox = divmod(origin, stride)
    tab = mvcost(j["qp"]).astype(np.int64)
    blk = cur2[oy + j["y"]:oy + j["y"] + j["h"], ox + j["x"]:ox + j["x"] + j["w"]]

    def cost(mx, my, sad_only=False):
        area = ref2[oy + j["y"] + my:oy + j["y"] + my + j["h"], ox + j["x"] + mx:ox + j["x"] + mx + j["w"]]
        return int(np.abs(area - blk).sum()) + (0 if sad_only else int(tab[65536 + 4 * mx - j["mvp"][0]] + tab[65536 + 4 * my - j["mvp"][1]]) & 0xffff)
    return cost


def _start(j):
    """the clipped, rounded predictor (motion.cpp:796, :806)"""
    pmx = min(max(j["mvp"][0], 4 * j["mvmin"][0]), 4 * j["mvmax"][0])
    pmy = min(max(j["mvp"][1], 4 * j["mvmin"][1]), 4 * j["mvmax"][1])
    return (pmx + 2) >> 2, (pmy + 2) >> 2


def _start_is_fullpel(j):
    """the start's cost is the clipped predictor's SAD alone when that is a full-pel vector (motion.cpp:803, :807), SAD + price of the rounded one otherwise (:809)"""
    pmx = min(max(j["mvp"][0], 4 * j["mvmin"][0]), 4 * j["mvmax"][0])
    pmy = min(max(j["mvp"][1], 4 * j["mvmin"][1]), 4 * j["mvmax"][1])
    return not ((pmx | pmy) & 3)


def deciding_ties(planes, jobs, mvcost):
    """per job: at the first pattern around the start vector two or more points (those the reference's y test lets through) attain the cheapest cost, and that cost
    is below the start's"""
    out = []
    for j in jobs:
        cost = _fullpel_cost(planes, j, mvcost)
        sx, sy = _start(j)
        pts = [cost(sx + dx, sy + dy) for dx, dy in PATTERN[j["method"]] if j["mvmin"][1] <= sy + dy <= j["mvmax"][1]]
        out.append(bool(pts) and min(pts) < cost(sx, sy, _start_is_fullpel(j)) and pts.count(min(pts)) >= 2)
    return out


def star_first_distance(planes, j, mvcost):
    """bDistance after the star search's first StarPatternSearch (motion.cpp:387-629, EarlyExitIters 3) from the start vector, for a job whose range holds every
    point of the pattern (asserted): the distance label of the last point that lowered the cost on strict `<`, 0 when none did"""
    cost = _fullpel_cost(planes, j, mvcost)
    ox, oy = _start(j)
    best, bdist, rounds = cost(ox, oy, _start_is_fullpel(j)), 0, 0
    assert not (ox | oy) or cost(0, 0) >= best, (j, "the zero vector takes the start's place (motion.cpp:812-821)")
    dist = 1
    while dist <= j["merange"]:
        assert j["mvmin"][0] <= ox - dist and ox + dist <= j["mvmax"][0] and j["mvmin"][1] <= oy - dist and oy + dist <= j["mvmax"][1], (j, dist)
        h = dist >> 1
        if dist == 1:
            pts = [(0, -1, 1), (-1, 0, 1), (1, 0, 1), (0, 1, 1)]
        elif dist <= 8:
            pts = [(0, -dist, dist), (-h, -h, h), (h, -h, h), (-dist, 0, dist), (dist, 0, dist), (-h, h, h), (h, h, h), (0, dist, dist)]
        else:
            pts = [(0, -dist, dist), (-dist, 0, dist), (dist, 0, dist), (0, dist, dist)]
            for k in (1, 2, 3):
                q = (dist >> 2) * k
                pts += [(-q, -dist + q, dist), (q, -dist + q, dist), (-q, dist - q, dist), (q, dist - q, dist)]
        saved = best
        for dx, dy, label in pts:
            c = cost(ox + dx, oy + dy)
            if c < best:
                best, bdist = c, label
        if best < saved:
            rounds = 0
        else:
            rounds += 1
            if rounds >= 3:
                break
        dist <<= 1
    return bdist


def quality(key, planes, jobs, res, mvcost):
    """the conditions a set has to meet, from its planes, the price table and its results `res`; returns what the generator prints"""
    note = ""
    luma = luma_of(planes) if len(planes) == 6 else planes
    assert len({(int(r[0]), int(r[1])) for r in res}) >= 8, (key, "fewer than 8 distinct result vectors")
    if "/mirror" in key:
        tied = deciding_ties(luma, jobs, mvcost)
        for method in METHODS:
            of = [t for t, j in zip(tied, jobs) if j["method"] == method]
            assert 4 * sum(of) >= len(of), (key, METHOD_NAME[method], sum(of), len(of))
            note += ", %s %d of %d deciding ties" % (METHOD_NAME[method], sum(of), len(of))
        sub = sum(1 for r in res if (int(r[0]) | int(r[1])) & 3)
        assert 3 * sub >= len(res), (key, sub, len(res))
        note += ", %d of %d sub-pel results" % (sub, len(res))
    if key.endswith("/raster"):
        d = [star_first_distance(luma, j, mvcost) for j in jobs if j["method"] == T.ME_STAR]
        assert all(v > 5 for v in d), (key, d)
        for j in jobs:      # columns mvmin.x, +5, ...: not a multiple of 4 of them, the last ones are priced one by one
            assert ((j["mvmax"][0] - j["mvmin"][0]) // 5 + 1) % 4 != 0, j
        note += ", star's first pattern ends at distances %s" % sorted(set(d))
    if key.endswith("/candidates"):
        assert all(len(j["mvc"]) == 12 for j in jobs)
    return note


def pairs_seen(depth):
    """every (method, subme) pair occurs in some luma set, and every PU size"""
    seen, sizes = set(), set()
    for name in LUMA_SETS:
        for j in luma_set(depth, name)[1]:
            seen.add((j["method"], j["subme"])); sizes.add((j["w"], j["h"]))
    return seen, sizes


# ----------------------------------------------------------------------------------------------------------
# CPU tests: the fixture, the oracle, the sets' quality
# ----------------------------------------------------------------------------------------------------------
def lib_mvcost(L):
    """mvcost(qp) of a host library (the oracle's orc_mvcost_table, the reference driver's ref_mvcost_table): the 2 * 65536 + 1 prices of that QP, difference 0 at [65536]"""
    import ctypes as C
    fn = getattr(L.lib, L.prefix + "mvcost_table")
    fn.restype = C.POINTER(C.c_uint16)

    def table(qp):
        p = fn(qp)
        return np.ctypeslib.as_array(C.cast(C.addressof(p.contents) - 2 * 65536, C.POINTER(C.c_uint16)), (2 * 65536 + 1,))
    return table


@pytest.mark.parametrize("depth", [8, 10])
def test_fixture_keys(depth):
    want = set(golden_sets(depth))
    have = {k for k in gold().files if k.split("/")[1] == str(depth)}
    assert have == want, (sorted(have - want), sorted(want - have))
    assert all(k.split("/")[1] in ("8", "10") for k in gold().files)
    for key, (planes, jobs, chroma) in golden_sets(depth).items():
        assert gold()[key].shape == (len(jobs), 3) and gold()[key].dtype == np.int32, key
        for method in METHODS:
            assert sum(1 for j in jobs if j["method"] == method) <= 48, key
    seen, sizes = pairs_seen(depth)
    assert seen == {(m, s) for m in METHODS for s in range(8)} and sizes == set(SIZES)
    assert {(j["method"], j["subme"]) for j in chroma_set(depth)[1]} == {(m, s) for m in METHODS for s in range(3, 8)}
    assert {(j["w"], j["h"]) for j in luma_set(depth, "mirror")[1]} == set(SIZES)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("name", list(LUMA_SETS) + ["mirror-c"])
def test_oracle_equals_fixture(depth, name):
    """the C restatement of the search (oracle/hevc_oracle_me.c) gives the reference's numbers on every set"""
    orc = T.load_oracle(depth)
    if name == "mirror-c":
        planes, jobs = chroma_set(depth)
        cur, rp, stride, cstride, origin, corg = planes
        MF._same(gold()["meec/%d/mirror" % depth], T.me_run_host_c(orc, cur, rp, stride, cstride, origin, corg, jobs), jobs, "oracle, chroma form")
        planes = luma_of(planes)
    else:
        planes, jobs = luma_set(depth, name)
    cur, rp, stride, origin = planes
    MF._same(gold()["mee/%d/%s" % (depth, name)], T.me_run_host(orc, cur, rp, stride, origin, jobs), jobs, "oracle, %s" % name)


@pytest.mark.parametrize("depth", [8, 10])
def test_set_quality(depth):
    """deciding ties, sub-pel results, distinct vectors, the raster scan's precondition: with the oracle's prices (the GPU test repeats the ties with me.host_mvcost)"""
    mvcost = lib_mvcost(T.load_oracle(depth))
    for key, (planes, jobs, chroma) in golden_sets(depth).items():
        quality(key, planes, jobs, gold()[key], mvcost)


# ----------------------------------------------------------------------------------------------------------
# GPU tests
# ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[8, 10])
def me(request):
    m = T.HipME(request.param)
    m.depth = request.param
    yield m
    m.close()


def _check(me, planes, jobs, want, idx, what, **kw):
    cur, rp, stride, origin = planes
    sub = [jobs[i] for i in idx]
    MF._same(want[idx], me.run(cur, rp, stride, origin, sub, **kw), sub, what)


def _of(jobs, methods):
    return [i for i, j in enumerate(jobs) if j["method"] in methods]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LUMA_SETS))
def test_kernel_variants(me, name):
    """the flags as the encoder sets them (FLAG_STAR exactly when a star job is present), the non-inlined variant on batches without star jobs, and the second pass
    alone on star jobs (without the flag the first kernel hands them on)"""
    planes, jobs = luma_set(me.depth, name)
    want = gold()["mee/%d/%s" % (me.depth, name)]
    if name == "mirror":
        tied = deciding_ties(planes, jobs, me.host_mvcost)
        for method in METHODS:
            of = [t for t, j in zip(tied, jobs) if j["method"] == method]
            assert 4 * sum(of) >= len(of), (METHOD_NAME[method], sum(of), len(of))
    dh, star = _of(jobs, (T.ME_DIA, T.ME_HEX)), _of(jobs, (T.ME_STAR,))
    _check(me, planes, jobs, want, list(range(len(jobs))), "%s, all methods, the encoder's flags" % name)
    _check(me, planes, jobs, want, dh, "%s, dia and hex, the encoder's flags (inlined variant)" % name)
    _check(me, planes, jobs, want, star, "%s, star, the encoder's flags" % name)
    _check(me, planes, jobs, want, dh, "%s, dia and hex under FLAG_STAR (non-inlined variant)" % name, flags=FLAG_STAR)
    _check(me, planes, jobs, want, star, "%s, star without FLAG_STAR (second pass)" % name, flags=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LUMA_SETS))
def test_small_windows(me, name):
    """windows smaller than the areas: the jobs whose candidates leave them are redone from memory"""
    planes, jobs = luma_set(me.depth, name)
    want = gold()["mee/%d/%s" % (me.depth, name)]
    for win in ((80, 80), (128, 96)):
        _check(me, planes, jobs, want, list(range(len(jobs))), "%s, window %dx%d" % ((name,) + win), max_win=win)
    _check(me, planes, jobs, want, _of(jobs, (T.ME_DIA, T.ME_HEX)), "%s, dia and hex, window 80x80 (inlined variant)" % name, max_win=(80, 80))


def _run_yuv(me, planes, jobs, chroma_mask, max_win=(192, 192)):
    """T.HipME.run_c with the chroma-SATD bit on the jobs of `chroma_mask` only"""
    cur, ref, stride, cstride, origin, corg = planes
    packed = T.me_pack_jobs(jobs)
    packed["method"] |= np.where(chroma_mask, 0x80, 0).astype(np.uint8)
    groups, order = me.plan(packed, 0, max_win)
    d = [me.upload(p) for p in cur + ref]
    isz = cur[0].itemsize
    chroma = me.upload(np.array([d[1].data_ptr() + corg * isz, d[2].data_ptr() + corg * isz, d[4].data_ptr() + corg * isz, d[5].data_ptr() + corg * isz], np.uint64))
    d_out = me.search(d[0], [d[3]], stride, origin, isz, groups, packed[order], max_win, d_chroma=chroma, cstride=cstride)
    me.torch.cuda.synchronize()
    res = d_out.cpu().numpy().view(T.ME_RESULT_DT)
    out = np.zeros((len(jobs), 3), np.int32)
    out[order, 0] = res["mv"][:, 0]; out[order, 1] = res["mv"][:, 1]; out[order, 2] = res["cost"]
    return out


@pytest.mark.gpu
def test_chroma_form(me):
    """the mirror set with chroma SATD in the sub-pel comparisons; then one batch that mixes the three methods and both chroma forms"""
    planes, jobs = chroma_set(me.depth)
    with_c, without = gold()["meec/%d/mirror" % me.depth], gold()["mee/%d/mirror-c" % me.depth]
    assert (with_c != without).any()
    every = np.ones(len(jobs), bool)
    MF._same(with_c, _run_yuv(me, planes, jobs, every), jobs, "chroma form")
    for win in ((80, 80), (128, 96)):
        MF._same(with_c, _run_yuv(me, planes, jobs, every, max_win=win), jobs, "chroma form, window %dx%d" % win)
    mask = (np.arange(len(jobs)) % 2 == 0) ^ (np.arange(len(jobs)) % 5 == 0)
    assert all({bool(m) for m, j in zip(mask, jobs) if j["method"] == method} == {False, True} for method in METHODS)
    MF._same(np.where(mask[:, None], with_c, without), _run_yuv(me, planes, jobs, mask), jobs, "mixed batch (three methods, chroma form on %d of %d jobs)" % (mask.sum(), len(jobs)))
    cur, rp, stride, origin = luma_of(planes)
    MF._same(without, me.run(cur, rp, stride, origin, jobs), jobs, "the chroma set's jobs in the luma form")


@pytest.mark.gpu
@pytest.mark.parametrize("star", [False, True])
def test_job_server(me, star):
    """the mirror set as ONE command of the resident job server (csrc/device_queue.hip: xa_op_me) and its ME_DEFERRED command: ME_SEARCH with the dia and hex jobs,
    ME_SEARCH_STAR with all three methods; the pattern of test_queue_ops.test_me_search"""
    from test_queue_ops import ME_WIN, server_ran
    planes, jobs = luma_set(me.depth, "mirror")
    cur, rp, stride, origin = planes
    idx = list(range(len(jobs))) if star else _of(jobs, (T.ME_DIA, T.ME_HEX))
    sub = [jobs[i] for i in idx]
    op = "ME_SEARCH_STAR" if star else "ME_SEARCH"
    packed = T.me_pack_jobs(sub)
    groups, order = me.plan(packed, 0, ME_WIN)
    assert len(groups) > 1 and groups["num_jobs"].max() > 1        # several groups of several jobs: the server takes them one after the other
    d_cur, d_ref = me.upload(cur), me.upload(rp)
    what = "%s, mirror set (%d jobs in %d groups)" % (op, len(sub), len(groups))
    with server_ran(me.L, what, ME_DEFERRED=1, **{op: 1}) as q:
        d_out = me.search(d_cur, [d_ref], stride, origin, cur.itemsize, groups, packed[order], ME_WIN, stream=q, flags=None)
    res = d_out.cpu().numpy().view(T.ME_RESULT_DT)
    got = np.zeros((len(sub), 3), np.int32)
    got[order, 0] = res["mv"][:, 0]; got[order, 1] = res["mv"][:, 1]; got[order, 2] = res["cost"]
    MF._same(gold()["mee/%d/mirror" % me.depth][idx], got, sub, what)
