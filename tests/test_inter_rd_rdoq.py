"""Residual RD of inter CUs with RDOQ (x265amd_inter_residual_rd, rdoq_level 1 / 2) against the reference's own Search::encodeResAndCalcRdInterCU.

With RDOQ the transform units are quantised during the walk, under the entropy state it has reached, so only the whole entry point runs this path (x265amd_inter_rd_walk
refuses it).  The expected results are the reference's (tests/golden/inter_rd_rdoq_golden.npz, written by tests/golden/make_golden.py: make_inter_rd_rdoq_golden)."""
import os

import numpy as np
import pytest

import hevc_testlib as T

# (depth, seed, slice type (0 B, 1 P), tuQTMaxInterDepth, psy-rd, rdoqLevel, psyRdoqScale)
CASES = [(8, 601, 1, 1, 2.0, 2, 256), (8, 602, 0, 2, 0.0, 1, 0), (10, 603, 1, 3, 2.0, 1, 1024), (10, 604, 0, 4, 1.0, 2, 0)]
GOLD_PATH = os.path.join(T.GOLDEN_DIR, "inter_rd_rdoq_golden.npz")


def rdoq_case(depth, seed, st, td, psy, rdoq_level, psy_rdoq_scale):
    """six candidate CUs on the 128x128 picture of T.rd_case (tu_log2_min is 2 there: an 8x8 CU's transform range reaches 4x4 whenever it may split)"""
    c = T.rd_case(depth, seed, st, td, psy, ncu=6)
    c["rp"]["rdoq_level"], c["rp"]["psy_rdoq_scale"] = rdoq_level, psy_rdoq_scale
    return c


def lowest_transform(c, i):
    """CUData::getInterTUQtDepthRange: log2 of the smallest transform CU i may use"""
    si = c["si"]
    log2, part, td = int(c["cus"][i]["log2_size"]), int(c["cu_units"][i][0]["part_size"]), int(si["tu_max_depth_inter"])
    return min(max(log2 - (td - 1 + int(td == 1 and part != 0)), int(si["tu_log2_min"])), int(si["tu_log2_max"]))


def test_outcomes_are_varied():
    """the golden set holds CUs of every size, an 8x8 CU whose transforms reach 4x4 (its four luma units share one chroma block), roots with and without residual
    and transform splits"""
    gold = np.load(GOLD_PATH)
    sizes, shared_chroma, root1, root0, split = set(), 0, 0, 0, 0
    levels = set()
    for k, case in enumerate(CASES):
        c = rdoq_case(*case)
        levels.add(case[5])
        for i in range(len(c["cus"])):
            u = gold["%d/%d/units" % (k, i)]
            log2 = int(c["cus"][i]["log2_size"])
            sizes.add(log2)
            shared_chroma += int(log2 == 3 and lowest_transform(c, i) == 2)
            root1 += int(u[:, 1:4].any()); root0 += int(not u[:, 1:4].any()); split += int(u[:, 0].max() > 0)
    assert sizes == {3, 4, 5, 6} and levels == {1, 2} and shared_chroma > 0 and root1 > 0 and root0 > 0 and split > 0, (sizes, levels, shared_chroma, root1, root0, split)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)))
def test_hip_inter_residual_rd_with_rdoq_matches_reference_golden(k):
    gold = np.load(GOLD_PATH)
    c = rdoq_case(*CASES[k])
    packed = T.rd_pack(T.rd_run_hip(T.load_hip(CASES[k][0]), c), c)
    for i, d in enumerate(packed):
        for name, a in d.items():
            want = gold["%d/%d/%s" % (k, i, name)]
            assert np.array_equal(a, want), "case %d CU %d (log2 %d qp %d): %s differs from the reference's result" % (
                k, i, c["cus"][i]["log2_size"], c["cus"][i]["qp"], name)
