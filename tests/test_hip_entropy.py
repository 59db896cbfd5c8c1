"""GPU: contexts / estBit / RDOQ / bits-only coefficient coding of libx265amd against the oracle and the golden vectors of the
reference (host-pointer forms), then the batched device entry points (x265amd_est_bit, x265amd_tu_chain_rdoq,
x265amd_coeff_bits) against the oracle on the same cases."""
import numpy as np
import pytest

import hevc_testlib as T
from test_entropy_golden import check_entropy


@pytest.mark.parametrize("depth", [8, 10])
def test_product_entropy_reset_host(depth):
    """x265amd_entropy_reset is host arithmetic inside the C-ABI library: checked without a GPU"""
    import os
    gold = np.load(os.path.join(T.GOLDEN_DIR, "entropy_golden.npz"))["reset/%d" % depth]
    L = T.load_hip(depth)
    assert np.array_equal(np.stack([T.entropy_reset(L, st, qp) for st in range(3) for qp in range(52)]), gold)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_entropy_matches_golden(depth):
    check_entropy(T.load_hip(depth), depth, seeds=(0,))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_est_bit_batch(depth):
    hip, orc = T.load_hip(depth), T.load_oracle(depth)
    rng = np.random.default_rng(9)
    shapes = [(l, 1) for l in range(2, 6)] + [(l, 0) for l in range(2, 5)]
    n = 300
    ctxs = np.zeros((n, 160), np.uint8)
    ctxs[:, :T.CTX_COUNT] = rng.integers(0, 126, (n, T.CTX_COUNT))
    per_job = [shapes[i % len(shapes)] for i in range(n)]
    want = [T.est_bit(orc, ctxs[i], l, lu) for i, (l, lu) in enumerate(per_job)]
    assert np.array_equal(T.est_bit_run_hip(hip, ctxs, per_job), np.stack(want))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_tu_chain_rdoq_and_coeff_bits(depth):
    hip, orc = T.load_hip(depth), T.load_oracle(depth)
    for seed in range(3):
        cases = T.rdoq_cases(depth, 800 + seed, 300)
        if seed == 2:
            for c in cases[::3]:
                c["rdoq"] = 0          # jobs of one batch may mix RDOQ and plain quantisation
        want = [T.rdoq_chain_oracle(orc, [c])[0] if c["rdoq"] else T.tu_run_chain_oracle(orc, [c])[0] for c in cases]
        chain, bits, ctx_out = T.tu_chain_rdoq_run_hip(hip, cases, coeff_bits=True)
        wbits = T.coeff_bits_run(orc, cases, [(int(w[0][0]), w[1]) for w in want])
        for i, (c, w, g) in enumerate(zip(cases, want, chain)):
            st, coeff, resi, recon = w
            assert tuple(int(v) for v in g[0]) == tuple(int(v) for v in st), (i, g[0], st)
            assert np.array_equal(g[1], coeff), i
            assert np.array_equal(g[3], recon), i
            assert np.array_equal(g[2], resi), i
            assert int(bits[i]) == wbits[i][0], (i, int(bits[i]), wbits[i][0])
            assert np.array_equal(ctx_out[i, :T.CTX_COUNT], wbits[i][1]), i
