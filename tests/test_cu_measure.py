"""The CU measurement (x265amd_measure_tiles, x265amd_measure_tile_list): every field of x265amd_cu_measure against the oracle's primitives.

The record feeds the merge and bi-prediction decisions (sa8d, sa8d_luma) and the recursion skip (src_mean, src_homo), and it is computed by two bodies:
block_cu_measure_job (a whole workgroup per CU: k_cu_measure_wg for n <= 64, and the job server's XA_OP_CU_MEASURE for n <= 16) and wave_cu_measure_job (a
wavefront per CU: k_cu_measure above 64, the job server above 16).  CPU (not gpu): the expectation itself (hevc_testlib.cu_measure_expected on the oracle)
against the same helper on the reference build's primitives, and its mean / deviation against a plain loop.  GPU: both kernels and both server forms, on
either side of each threshold."""
import functools

import numpy as np
import pytest

import hevc_testlib as T

FIELDS = ("sse", "psy", "sa8d", "sa8d_luma", "src_mean", "src_homo", "reserved")


@functools.lru_cache(maxsize=None)
def case_and_expected(depth):
    """the cases and the oracle's records, computed once per depth and shared (read-only) by every test"""
    c = T.measure_case(depth)
    want = T.cu_measure_expected(T.load_oracle(depth), depth, [p.ravel() for p in c["src"]], c["stride"], c["cstride"], c["cus"], c["tiles"])
    want.setflags(write=False)
    return c, want


def pick(n, shift):
    """n CUs of the case list: CU 0 (64x64, source pmax against tile 0) always, then n - 1 of the others from `shift` on, wrapping (72 CUs in all)"""
    return np.array([0] + [1 + (shift + k) % 71 for k in range(n - 1)])


def describe(c, i):
    cu = c["cus"][i]
    return "CU %d (%dx%d at %d,%d; %s)" % (i, 1 << int(cu["log2_size"]), 1 << int(cu["log2_size"]), cu["x"], cu["y"], T.MEASURE_KINDS[c["kinds"][i]])


def test_case_list_holds_every_size_and_content_and_the_largest_sse():
    for depth in (8, 10):
        c, want = case_and_expected(depth)
        assert {(int(cu["log2_size"]), k) for cu, k in zip(c["cus"], c["kinds"])} == {(l, k) for l in (3, 4, 5, 6) for k in range(6)}
        pmax = (1 << depth) - 1
        assert int(c["cus"][0]["log2_size"]) == 6 and c["kinds"][0] == 3
        assert int(want[0]["sse"][0]) == 4096 * pmax * pmax
    # 10 bit: 4096 * 1023^2 does not fit a signed 32-bit sum
    assert int(case_and_expected(10)[1][0]["sse"][0]) == 4286582784 > 2 ** 31


def test_mean_and_deviation_against_a_plain_loop():
    for depth in (8, 10):
        c, want = case_and_expected(depth)
        small = [i for i in range(len(c["cus"])) if int(c["cus"][i]["log2_size"]) <= 4 and c["kinds"][i] in (0, 4)][:2]
        assert len(small) == 2
        for i in small:
            cu = c["cus"][i]
            S = 1 << int(cu["log2_size"])
            total = 0
            for y in range(S):
                for x in range(S):
                    total += int(c["src"][0][int(cu["y"]) + y, int(cu["x"]) + x])
            mean = total // (S * S)
            dev = 0
            for y in range(S):
                for x in range(S):
                    dev += abs(int(c["src"][0][int(cu["y"]) + y, int(cu["x"]) + x]) - mean)
            assert (int(want[i]["src_mean"]), int(want[i]["src_homo"])) == (mean, dev // (S * S)), describe(c, i)


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("depth", [8, 10])
def test_expected_records_match_the_reference_primitives(depth):
    """cu_measure_expected on the oracle = the same helper on the reference build's sa8d / sse_pp / psy_cost_pp, on the cases of the GPU tests"""
    c, want = case_and_expected(depth)
    ref = T.cu_measure_expected(T.load_ref(depth), depth, [p.ravel() for p in c["src"]], c["stride"], c["cstride"], c["cus"], c["tiles"])
    for i in range(len(want)):
        for f in FIELDS:
            assert np.array_equal(want[i][f], ref[i][f]), "%s: %s oracle %s, reference %s" % (describe(c, i), f, want[i][f], ref[i][f])


def check(depth, n, shift, queue, tile_list):
    hip = T.load_hip(depth)
    c, want = case_and_expected(depth)
    idx = pick(n, shift)
    what = "%s, %d jobs, %s" % ("measure_tile_list" if tile_list else "measure_tiles", n, "job server" if queue else "launch")
    if queue:
        T.queue_stats(hip, reset=1)
    got, tiles, src = T.cu_measure_run_hip(hip, c, idx, stream=T.held_queue(hip) if queue else None, tile_list=tile_list)
    if queue:
        ran = T.queue_stats(hip)["CU_MEASURE"]
        assert ran == 1, "%s: the job server ran %d CU_MEASURE commands, not 1" % (what, ran)
    for k, i in enumerate(idx):
        for f in FIELDS:
            assert np.array_equal(got[k][f], want[i][f]), "%s: job %d = %s: %s %s, want %s" % (what, k, describe(c, i), f, got[k][f], want[i][f])
        assert np.array_equal(tiles[k], c["tiles"][i]), "%s: job %d = %s: the tile (block and the pattern around it) changed" % (what, k, describe(c, i))
    for p in range(3):
        assert np.array_equal(src[p], c["src"][p]), "%s: source plane %d changed" % (what, p)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("n,shift", [(1, 0), (64, 0), (65, 7)])       # measure_use_wg: n <= 64 a workgroup per CU, above a wavefront per CU
def test_hip_measure_tiles_launch(depth, n, shift):
    check(depth, n, shift, queue=False, tile_list=False)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("n,shift", [(1, 0), (16, 0), (17, 15), (40, 31)])      # xa_op_cu_measure: n <= 2 * XA_SERVER_WAVES the block form, above the wave form on LDS tiles of xa_smem
def test_hip_measure_tiles_job_server(depth, n, shift):
    check(depth, n, shift, queue=True, tile_list=False)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("queue", [False, True])
@pytest.mark.parametrize("n,shift", [(2, 40), (17, 50)])
def test_hip_measure_tile_list(depth, n, shift, queue):
    check(depth, n, shift, queue=queue, tile_list=True)
