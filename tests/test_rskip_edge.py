"""The edge-based recursion skip (--rskip 2) below the encoder: the device pass x265amd_rskip_edge_counts, its host model x265amd_rskip_edge_model and the decision
x265amd_rskip_edge_skip, against tests/golden/rskip_edge_golden.npz -- bit planes cut by tests/golden/make_rskip_edge_golden.py from the reference's own computeEdge
(libx265_ref{8,10}.so: no angle plane, white pixel 1, the output plane zeroed first as Frame::create does).

Without a GPU: the host model against the reference's planes; the decision against the reference's formula over every count.
On the GPU: the kernel's counts against the model's, for every size and content below, both bit depths.

A gradient whose magnitude is EXACTLY the threshold T (255 / 1023) does not exist: gH and gV are both congruent to tl + tr + bl + br modulo 2 (the weights 3 are odd, the
weights 10 even), so gH * gH + gV * gV is a multiple of 4 or a multiple of 4 plus 2 -- never the odd T * T.  What can be built, and is: the pair of gradients whose squared magnitude
is the smallest at or above T * T and the pair with the largest below it (`near_above`, `near_below`: T * T + 1 and the nearest sum beneath), and plain steps whose
gradient 16 * d is the first at or above T (`step_at`: 256 / 1024) and the last below it (`step_below`: 240 / 1008)."""
import ctypes as C
import os

import numpy as np
import pytest

import hevc_testlib as T

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "rskip_edge_golden.npz")

# The kernel's workgroup is one 32x32 block with a halo of one sample:
#   64x64    four whole blocks, every halo side met inside the picture
#   40x40    one whole block, partial ones right, below and in the corner (8 of 32 samples)
#   104x72   partial blocks right (8 columns) and below (8 rows), four blocks across
#   136x72   five blocks across, the last one 8 columns wide
SIZES = [(64, 64), (40, 40), (104, 72), (136, 72)]
CONTENTS = ["flat", "noise40", "step_at", "step_below", "near_above", "near_below", "stripes_v", "stripes_h", "stripes_d", "max_border"]


def _near_pairs(depth):
    """neighbourhoods (tr, mr, br, bc; the other four neighbours 0) whose gradients' squared magnitude is the smallest >= T * T and the largest < T * T that such a
    neighbourhood reaches: gH = 3 tr + 10 mr + 3 br, gV = -3 tr + 3 br + 10 bc"""
    pmax = (1 << depth) - 1
    tr, mr, br, bc = np.meshgrid(np.arange(16), np.arange(pmax // 8), np.arange(16), np.arange(16), indexing="ij")
    gh = 3 * tr + 10 * mr + 3 * br; gv = -3 * tr + 3 * br + 10 * bc
    m = (gh * gh + gv * gv).ravel().astype(np.int64)
    t2 = pmax * pmax
    above = int(np.flatnonzero(m == m[m >= t2].min())[0]); below = int(np.flatnonzero(m == m[m < t2].max())[0])
    pick = lambda i: (int(tr.ravel()[i]), int(mr.ravel()[i]), int(br.ravel()[i]), int(bc.ravel()[i]), int(m[i]))
    return pick(above), pick(below)


_NEAR = {}


def plane(name, w, h, depth):
    rng = np.random.default_rng([depth, w, h, CONTENTS.index(name)])
    pmax = (1 << depth) - 1
    sc = 1 << (depth - 8)
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "flat":
        p = np.full((h, w), 100 * sc)
    elif name == "noise40":
        p = 100 * sc + rng.integers(0, 40 * sc + 1, (h, w))          # gradient magnitudes on both sides of T
    elif name in ("step_at", "step_below"):
        d = (pmax + 15) // 16 - (name == "step_below")                # 16 d = 256 / 1024, or 240 / 1008
        # vertical steps next to the block boundary x = 32 and elsewhere; step_at has a horizontal one at y = 31 as well (where two steps cross the gradient is larger,
        # so step_below, which must stay without a single edge, has none)
        p = 50 * sc + d * ((xx >= w // 2 - 3).astype(np.int64) + (xx >= 33) + ((yy >= 31) if name == "step_at" else 0))
    elif name in ("near_above", "near_below"):
        if depth not in _NEAR:
            _NEAR[depth] = _near_pairs(depth)
        tr, mr, br, bc, _ = _NEAR[depth][name == "near_below"]
        p = np.zeros((h, w), np.int64)
        for cy in range(1, h - 1, 4):                                   # neighbourhoods four apart: centres at every position relative to the blocks, the halo included
            for cx in range(1, w - 1, 4):
                p[cy - 1, cx + 1], p[cy, cx + 1], p[cy + 1, cx + 1], p[cy + 1, cx] = tr, mr, br, bc
    elif name == "stripes_v":
        p = 60 * sc + 40 * sc * ((xx // 3) % 2)
    elif name == "stripes_h":
        p = 60 * sc + 40 * sc * ((yy // 5) % 2)
    elif name == "stripes_d":
        p = 60 * sc + 40 * sc * (((xx + yy) // 4) % 2)
    else:
        p = np.zeros((h, w), np.int64)
        p[0, :] = p[-1, :] = p[:, 0] = p[:, -1] = pmax               # the outermost row and column at the largest value: their own bits stay 0, their neighbours' are 1
    return np.clip(p, 0, pmax).astype(np.uint8 if depth == 8 else np.uint16)


def block_counts(bits):
    h, w = bits.shape
    bh, bw = (h + 31) // 32, (w + 31) // 32
    e = np.zeros((bh * 32, bw * 32), np.int64)
    e[:h, :w] = bits
    return e.reshape(bh, 32, bw, 32).sum(axis=(1, 3)).ravel().astype(np.uint32)


def model(depth, src, stride_extra=0):
    """x265amd_rskip_edge_model: (bit plane, counts)"""
    lib = T.load_hip(depth).lib
    h, w = src.shape
    stride = w + stride_extra
    buf = np.zeros((h, stride), src.dtype); buf[:, :w] = src
    bits = np.full((h, w), 7, np.uint8)
    counts = np.full(((h + 31) // 32) * ((w + 31) // 32), 0xffffffff, np.uint32)
    lib.x265amd_rskip_edge_model.argtypes = [C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.x265amd_rskip_edge_model(T._ptr(buf), stride, w, h, T._ptr(bits), T._ptr(counts)) == 0
    return bits, counts


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD_PATH)


# ---- without a GPU ----
@pytest.mark.parametrize("depth", [8, 10])
def test_model_equals_the_references_compute_edge(depth, gold):
    """the host model's plane is the reference's computeEdge plane, sample for sample, and its counts are that plane's ones per 32x32 block"""
    ones = 0
    for w, h in SIZES:
        for name in CONTENTS:
            want = gold["ce%d/%dx%d/%s" % (depth, w, h, name)]
            bits, counts = model(depth, plane(name, w, h, depth), stride_extra=3)
            assert np.array_equal(bits, want), (w, h, name, np.argwhere(bits != want)[:8])
            assert np.array_equal(counts, block_counts(want)), (w, h, name)
            assert not want[0].any() and not want[-1].any() and not want[:, 0].any() and not want[:, -1].any()
            ones += int(want.sum())
            if name in ("flat", "step_below"):
                assert not want.any(), (w, h, name)
            if name in ("near_above", "near_below"):          # the planted centres decide by one unit of the squared magnitude (their neighbours see other gradients)
                assert want[1:h - 1:4, 1:w - 1:4].all() if name == "near_above" else not want[1:h - 1:4, 1:w - 1:4].any(), (w, h, name)
            if name in ("step_at", "near_above", "stripes_v", "stripes_h", "stripes_d", "max_border"):
                assert want.any(), (w, h, name)
        n40 = gold["ce%d/%dx%d/noise40" % (depth, w, h)]
        assert 0.2 < n40[1:-1, 1:-1].mean() < 0.8, (w, h)            # the noise does straddle the threshold
    assert ones > 0
    (_, _, _, _, above), (_, _, _, _, below) = _near_pairs(depth)
    t2 = ((1 << depth) - 1) ** 2
    assert above == t2 + 1 and below < t2


def test_decision_equals_the_references_formula_over_every_count():
    """Analysis::complexityCheckCU's edge branch: cuEdgeVariance = (ss - ((double)sum * sum / pixelCount)) / pixelCount with sum = ss = count, against
    (double)edgeVarThreshold -- the FLOAT widened (0.05f is 0.0500000007..., 0.06f is 0.0599999986...) -- for every count of a 32x32 and a 64x64 CU.  Every operation of
    the formula is exact in doubles here (counts up to 2^12, divisions by powers of two), so Python's doubles are the reference's."""
    lib = T.load_hip(8).lib
    lib.x265amd_rskip_edge_skip.argtypes = [C.c_uint32, C.c_int, C.c_float]
    lib.x265amd_rskip_edge_skip.restype = C.c_int
    for size in (32, 64):
        n = size * size
        for thr in (0.0, 0.05, 0.06, 0.25, 1.0):
            thr32 = np.float32(thr)
            got = np.array([lib.x265amd_rskip_edge_skip(c, size, C.c_float(float(thr32))) for c in range(n + 1)])
            want = np.array([0 if (c - (float(c) * c / n)) / n > float(thr32) else 1 for c in range(n + 1)])
            assert np.array_equal(got, want), (size, thr, np.flatnonzero(got != want)[:8])
            # the counts at which the variance crosses the threshold: c (n - c) / n^2 > thr, in exact integers against the float's exact value
            num, den = float(thr32).as_integer_ratio()
            exact = np.array([0 if c * (n - c) * den > num * n * n else 1 for c in range(n + 1)])
            assert np.array_equal(got, exact), (size, thr)
            if thr == 0.0:
                assert got[0] == 1 and got[n] == 1 and not got[1:n].any()          # only a plane without edges, or of nothing but edges, has variance 0
            elif thr < 0.25:
                cross = np.flatnonzero(np.diff(got))
                assert len(cross) == 2 and got[0] == 1 and got[n // 2] == 0 and got[n] == 1, (size, thr, cross)
            else:
                assert got.all()                                                    # the variance of a 0 / 1 plane never exceeds 0.25


def test_new_entry_points_are_exported():
    """the device pass and the analysis entries that take the picture's edge counts (the existing entries have nowhere to take them and keep rejecting rskip 2)"""
    lib = T.load_hip(8).lib
    for name in ("x265amd_compress_ctu_inter_ex", "x265amd_analyse_frame_ex", "x265amd_rskip_edge_counts"):
        assert hasattr(lib, name), name


# ---- on the GPU ----
def run_counts(depth, src, stride_extra=0, lead=0):
    """x265amd_rskip_edge_counts on a plane held in device memory with a guard of 0xa5 bytes round it (a row above, a row below, the stride's slack, `lead` elements in
    front) that no counted gradient may come from"""
    import torch
    lib = T.load_hip(depth).lib
    h, w = src.shape
    stride = w + stride_extra
    host = np.full(lead + (h + 2) * stride, 0xa5a5 if depth > 8 else 0xa5, src.dtype)
    host[lead:].reshape(h + 2, stride)[1:h + 1, :w] = src
    d = torch.from_numpy(host.view(np.uint8)).cuda()
    nb = ((w + 31) // 32) * ((h + 31) // 32)
    d_counts = torch.full((nb + 2,), -1, dtype=torch.int32, device="cuda")
    lib.x265amd_last_error.restype = C.c_char_p
    lib.x265amd_rskip_edge_counts.argtypes = [C.c_void_p, C.c_uint64, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
    rc = lib.x265amd_rskip_edge_counts(None, d.data_ptr() + (lead + stride) * src.itemsize, stride, w, h, d_counts.data_ptr() + 4)
    assert rc == 0, lib.x265amd_last_error()
    torch.cuda.synchronize()
    out = d_counts.cpu().numpy().view(np.uint32)
    assert out[0] == 0xffffffff and out[-1] == 0xffffffff          # nothing written beside the blocks
    return out[1:-1].copy()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SIZES)
def test_hip_counts_equal_the_models(depth, size):
    w, h = size
    for name in CONTENTS:
        src = plane(name, w, h, depth)
        bits, want = model(depth, src)
        assert np.array_equal(want, block_counts(bits))
        got = run_counts(depth, src)
        assert np.array_equal(got, want), (name, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("layout", ["wide_stride", "odd_offset"])
def test_hip_counts_with_a_wider_stride_and_an_odd_offset(depth, layout):
    """the plane inside a wider buffer (stride = width + 7) and starting at an odd element offset of the allocation: the guard samples round it are read by no gradient
    that counts"""
    extra, lead = (7, 0) if layout == "wide_stride" else (5, 1)
    for w, h in ((104, 72), (40, 40)):
        for name in ("noise40", "stripes_d", "max_border", "near_above"):
            src = plane(name, w, h, depth)
            _, want = model(depth, src)
            got = run_counts(depth, src, stride_extra=extra, lead=lead)
            assert np.array_equal(got, want), (layout, w, h, name, got, want)
