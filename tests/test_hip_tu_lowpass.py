"""X265AMD_TU_LOWPASS in the transform-unit chains: x265amd_tu_chain, x265amd_intra_tu_chain and their RDOQ forms, as kernels of their own and as commands of the job
server (a wavefront per unit, and the whole workgroup per large unit), against the reference's own Quant with its primitive table switched the way
enableLowpassDCTPrimitives switches it (tests/golden/lowpass_dct_golden.npz, cut by tests/golden/make_lowpass_dct_golden.py).  The units are those of
hevc_testlib.tu_cases / intra_tu_cases, picked by lowpass_dct_lib: 32x32 and 16x16 luma, 16x16 chroma of both planes, 8x8 and 4x4 units (which the flag must not
touch), sign hiding on and off, RDOQ levels 1 and 2 with psy-RDOQ.  With the flag clear the chains give what the C oracle gives, as before."""
import numpy as np
import pytest

import hevc_testlib as T
import lowpass_dct_lib as LP

pytestmark = pytest.mark.gpu

_G = {}


def _golden():
    if "g" not in _G:
        _G["g"] = np.load(LP.GOLDEN)
    return _G["g"]


def _want(name, depth, cases):
    return LP.unflat(_golden(), "%s%d/" % (name, depth), cases, LP.INTER_NAMES if name == "inter" else LP.INTRA_NAMES)


def _inter_oracle(depth, cases):
    return T.tu_run_chain_oracle(T.load_oracle(depth), cases)


@pytest.mark.parametrize("via", ["kernel", "queue_waves", "queue_workgroup"])
@pytest.mark.parametrize("depth", [8, 10])
def test_tu_chain_with_the_flag(depth, via):
    """x265amd_tu_chain: every unit flagged.  queue_waves: all 40 units in one command (more than 4 * XA_SERVER_WAVES: a wavefront per unit); queue_workgroup: the
    large units a few at a time (the whole workgroup takes each)"""
    L = T.load_hip(depth)
    cases = LP.inter_cases(depth)
    want = _want("inter", depth, cases)
    if via == "queue_workgroup":
        idx = [i for i, c in enumerate(cases) if c["log2"] >= 4][:6] + [i for i, c in enumerate(cases) if c["log2"] < 4][:2]
        sub = [cases[i] for i in idx]
        got = LP.tu_run_hip(L, sub, [LP.TU_LOWPASS] * len(sub), stream=T.held_queue(L))
        LP.assert_units(got, [want[i] for i in idx], sub, LP.INTER_NAMES, "tu_chain, workgroup form")
        return
    assert len(cases) > 32
    got = LP.tu_run_hip(L, cases, [LP.TU_LOWPASS] * len(cases), stream=T.held_queue(L) if via == "queue_waves" else None)
    LP.assert_units(got, want, cases, LP.INTER_NAMES, "tu_chain (%s)" % via)


@pytest.mark.parametrize("depth", [8, 10])
def test_flagged_and_unflagged_units_in_one_launch(depth):
    """every other unit flagged: the flagged ones give the reference's switched results, the others the oracle's; and the flag on 4x4 / 8x8 units changes nothing"""
    L = T.load_hip(depth)
    cases = LP.inter_cases(depth)
    want, plain = _want("inter", depth, cases), _inter_oracle(depth, cases)
    flags = [LP.TU_LOWPASS if i % 2 else 0 for i in range(len(cases))]
    got = LP.tu_run_hip(L, cases, flags)
    LP.assert_units(got, [w if f else p for w, p, f in zip(want, plain, flags)], cases, LP.INTER_NAMES, "tu_chain, mixed flags")
    small = [i for i, c in enumerate(cases) if c["log2"] < 4]
    assert len(small) == 20
    LP.assert_units(want, plain, cases, LP.INTER_NAMES, "the fixture's small units against the oracle", only=set(small))
    changed = [i for i, c in enumerate(cases) if c["log2"] >= 4 and any(not np.array_equal(np.asarray(a).ravel(), np.asarray(b).ravel()) for a, b in zip(want[i], plain[i]))]
    assert len(changed) >= 8, "the option has to show in the large units"


@pytest.mark.parametrize("depth", [8, 10])
def test_the_flag_clear_gives_the_oracle(depth):
    """a record with the flags byte 0: the chains as they were (and the reserved bits of the byte ask for nothing)"""
    L = T.load_hip(depth)
    cases = LP.inter_cases(depth)
    plain = _inter_oracle(depth, cases)
    LP.assert_units(LP.tu_run_hip(L, cases, [0] * len(cases)), plain, cases, LP.INTER_NAMES, "tu_chain, flag clear")
    icases = LP.intra_cases(depth, True)
    want = T.intra_tu_run_host(T.load_oracle(depth), icases)
    LP.assert_units(LP.intra_run_hip(L, icases, [0] * len(icases)), want, icases, LP.INTRA_NAMES, "intra_tu_chain (RDOQ), flag clear")


@pytest.mark.parametrize("via", ["kernel", "queue"])
@pytest.mark.parametrize("rdoq", [False, True])
@pytest.mark.parametrize("depth", [8, 10])
def test_intra_tu_chain_with_the_flag(depth, rdoq, via):
    """x265amd_intra_tu_chain and its RDOQ form (levels 1 and 2, psy-RDOQ on the luma units: the source block's transform is the low-pass one too)"""
    L = T.load_hip(depth)
    name = "intra_rdoq" if rdoq else "intra"
    cases = LP.intra_cases(depth, rdoq)
    got = LP.intra_run_hip(L, cases, [LP.TU_LOWPASS] * len(cases), stream=T.held_queue(L) if via == "queue" else None)
    LP.assert_units(got, _want(name, depth, cases), cases, LP.INTRA_NAMES, "intra_tu_chain %s (%s)" % (name, via))


@pytest.mark.parametrize("via", ["kernel", "queue"])
@pytest.mark.parametrize("depth", [8, 10])
def test_tu_chain_rdoq_with_the_flag(depth, via):
    """x265amd_tu_chain_rdoq on the RDOQ units of the intra set, their predictions handed over: the same levels, residuals, reconstructions and figures"""
    L = T.load_hip(depth)
    icases = LP.intra_cases(depth, True)
    want = _want("intra_rdoq", depth, icases)
    cases = LP.as_tu_cases(icases, [np.asarray(w[1]).reshape(1 << c["log2"], 1 << c["log2"]) for w, c in zip(want, icases)])
    got = LP.tu_run_hip(L, cases, [LP.TU_LOWPASS] * len(cases), rdoq=True, stream=T.held_queue(L) if via == "queue" else None)
    # (stats, pred, recon, coeff, resi) of the fixture in the order of the chain's (stats, coeff, resi, recon)
    LP.assert_units(got, [(w[0], w[3], w[4], w[2]) for w in want], cases, LP.INTER_NAMES, "tu_chain_rdoq (%s)" % via)
