"""Residual path against golden results of the reference's Quant / RDCost classes (tests/golden/tu_golden.npz):
the oracle (always), and the product's host-side RDCost formulas (pure host code, no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

import hevc_testlib as T

GOLD = np.load(os.path.join(T.GOLDEN_DIR, "tu_golden.npz"))


def check_tu(L, depth):
    for seed in range(4):
        cases = T.tu_cases(depth, 100 + seed, 150)
        res = T.tu_run_host(L, cases)
        assert np.array_equal(np.array([r[0] for r in res], np.int32), GOLD["tu/%d/%d/numsig" % (depth, seed)])
        assert np.array_equal(np.concatenate([r[1] for r in res]), GOLD["tu/%d/%d/coeff" % (depth, seed)])
        assert np.array_equal(np.concatenate([r[2].ravel() for r in res]), GOLD["tu/%d/%d/resi" % (depth, seed)])


def check_rdcost(lib, fn, depth):
    rng = np.random.default_rng(5)
    want = GOLD["rdcost/%d" % depth]
    for k in range(300):
        qp, st = int(rng.integers(0, 70)), int(rng.integers(0, 3))
        psy = float(rng.choice([0.0, 1.0, 2.0, 0.7]))
        dist, bits, pc = int(rng.integers(0, 1 << 24)), int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 16))
        a = np.zeros(6, np.uint64)
        getattr(lib, fn)(qp, st, C.c_double(psy), C.c_uint64(dist), C.c_uint32(bits), C.c_uint32(pc), T._ptr(a))
        assert np.array_equal(a, want[k]), (k, qp, st, psy)


@pytest.mark.parametrize("depth", [8, 10])
def test_oracle_tu(depth):
    check_tu(T.load_oracle(depth), depth)


@pytest.mark.parametrize("depth", [8, 10])
def test_oracle_rdcost(depth):
    check_rdcost(T.load_oracle(depth).lib, "orc_rdcost", depth)


@pytest.mark.parametrize("depth", [8, 10])
def test_product_rdcost_host(depth):
    """x265amd_rdcost is host arithmetic inside the C-ABI library: checked without a GPU"""
    check_rdcost(T.load_hip(depth).lib, "x265amd_rdcost", depth)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_transform_inverse(depth):
    check_tu(T.load_hip(depth), depth)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_tu_chain(depth):
    """the fused per-TU kernel (x265amd_tu_chain) on a batch, against the oracle's restatement of the measurement"""
    hip, orc = T.load_hip(depth), T.load_oracle(depth)
    for seed in range(3):
        cases = T.tu_cases(depth, 300 + seed, 200)
        want = T.tu_run_chain_oracle(orc, cases)
        got = T.tu_chain_run_hip(hip, cases, depth)
        for i, (c, w, g) in enumerate(zip(cases, want, got)):
            st, coeff, resi, recon = w
            assert tuple(int(v) for v in g[0]) == tuple(int(v) for v in st), (i, g[0], st)
            assert np.array_equal(g[3], recon), i
            assert np.array_equal(g[1], coeff), i
            assert np.array_equal(g[2], resi), i
