"""Intra candidates of inter-slice CUs (x265amd_intra_in_inter; SURVEY row a7, RD side) against golden results of the reference's own
Search::checkIntraInInter + encodeIntraInInter run on CUData / Slice / Search / PicYuv fixtures (tests/golden/intra_rd_golden.npz, generated
here from oracle/_ref by tests/golden/make_golden.py)."""
import os

import numpy as np
import pytest

import hevc_testlib as T

# (depth, seed, slice type (0 B, 1 P), psy-rd, strong intra smoothing)
CASES = [(8, 601, 1, 2.0, 1), (8, 602, 0, 0.0, 1), (10, 603, 1, 2.0, 1), (8, 604, 1, 1.0, 0), (10, 605, 0, 0.0, 0), (8, 606, 1, 2.0, 1)]
GOLD_PATH = os.path.join(T.GOLDEN_DIR, "intra_rd_golden.npz")


def test_golden_covers_modes_and_edges():
    gold = np.load(GOLD_PATH)
    modes = set(); cmodes = set(); nocbf = 0
    for k in range(len(CASES)):
        for i in range(10):
            d = gold["%d/%d/dirs" % (k, i)]
            modes.add(int(d[0, 0])); cmodes.add(int(d[0, 1]))
            nocbf += int(not gold["%d/%d/units" % (k, i)][:, 1:4].any())
    assert len(modes) >= 8 and len(cmodes) >= 4, (modes, cmodes)


@pytest.mark.gpu
def test_hip_intra_in_inter_matches_reference_golden():
    gold = np.load(GOLD_PATH)
    for k, (depth, seed, st, psy, strong) in enumerate(CASES):
        c = T.intra_rd_case(depth, seed, st, psy, strong=strong)
        got = T.intra_rd_pack(T.intra_rd_run_hip(T.load_hip(depth), c), c)
        for i, d in enumerate(got):
            for name in ("info", "dirs", "pred", "units", "coeff", "recon", "res", "ctx"):
                want = gold["%d/%d/%s" % (k, i, name)]
                a = np.asarray(d[name])
                if not np.array_equal(a, want):
                    bad = np.argwhere(a != want)[:6].tolist() if a.shape == want.shape else "shape"
                    raise AssertionError("case %d CU %d (x %d y %d log2 %d qp %d): %s differs from the reference's result at %s: got %s want %s" % (
                        k, i, c["cus"][i]["x"], c["cus"][i]["y"], c["cus"][i]["log2_size"], c["cus"][i]["qp"], name, bad,
                        a[tuple(np.array(bad).T)].tolist() if bad != "shape" else a.shape, want[tuple(np.array(bad).T)].tolist() if bad != "shape" else want.shape))


# ---- Search::checkIntra: (depth, seed, slice type (2 I, 1 P, 0 B), psy-rd, strong intra smoothing) ----
CHECK_CASES = [(8, 701, 2, 2.0, 1), (8, 702, 2, 0.0, 1), (10, 703, 2, 2.0, 0), (8, 704, 1, 2.0, 1), (10, 705, 2, 1.0, 1), (8, 706, 2, 2.0, 1),
               (8, 707, 2, 2.0, 1, 4), (8, 708, 1, 0.0, 1, 4), (10, 709, 2, 2.0, 1, 4),           # 6th field: tu-intra-depth 4 (three levels of transform splits)
               (8, 711, 1, 2.0, 1), (8, 722, 0, 2.0, 1)]                                           # P / B slices without delta QP (tests/test_intra_cu_bits.py)
CHECK_GOLD_PATH = os.path.join(T.GOLDEN_DIR, "check_intra_golden.npz")


def test_check_intra_golden_covers_nxn_and_splits():
    gold = np.load(CHECK_GOLD_PATH)
    nxn = split = 0
    for k in range(len(CHECK_CASES)):
        for i in range(10):
            nxn += int(gold["%d/%d/dirs" % (k, i)][0, 2] == 3)
            split += int(gold["%d/%d/units" % (k, i)][:, 0].max() > int(gold["%d/%d/dirs" % (k, i)][0, 2] == 3))
    assert nxn >= 5 and split >= 3, (nxn, split)


@pytest.mark.gpu
def test_hip_check_intra_matches_reference_golden():
    gold = np.load(CHECK_GOLD_PATH)
    for k, cfg in enumerate(CHECK_CASES):
        depth, seed, st, psy, strong = cfg[:5]
        c = T.check_intra_case(depth, seed, st, psy, strong=strong, tu_intra=cfg[5] if len(cfg) > 5 else 0)
        got = T.intra_rd_pack(T.check_intra_run_hip(T.load_hip(depth), c), c)
        for i, d in enumerate(got):
            for name in ("dirs", "pred", "units", "coeff", "recon", "res", "ctx"):
                want = gold["%d/%d/%s" % (k, i, name)]
                a = np.asarray(d[name])
                if not np.array_equal(a, want):
                    bad = np.argwhere(a != want)[:6].tolist() if a.shape == want.shape else "shape"
                    raise AssertionError("case %d CU %d (x %d y %d log2 %d qp %d part %d): %s differs from the reference's result at %s: got %s want %s" % (
                        k, i, c["cus"][i]["x"], c["cus"][i]["y"], c["cus"][i]["log2_size"], c["cus"][i]["qp"], c["parts"][i], name, bad,
                        a[tuple(np.array(bad).T)].tolist() if bad != "shape" else a.shape, want[tuple(np.array(bad).T)].tolist() if bad != "shape" else want.shape))


# ---- what the two plain entries refuse: error code and x265amd_last_error text as recorded from the commit before the entry paths were split by name ----
E_NULL = b"intra rd: null argument"
E_LOSSLESS = b"intra rd: lossless coding is not supported"
E_NXN = b"intra rd: NxN only for 8x8 CUs with 4x4 transforms"
E_PLACE = b"intra rd: CU outside the picture, misaligned, or not 8..32"


def refusals(W):
    """(name, CU x / y / log2 size, part_size (None: both entries, 0), slice fields changed, out is NULL, code, text) on a picture W samples wide"""
    return [("null out", (16, 16, 4), None, {}, True, -1, E_NULL),
            ("64x64 CU", (0, 0, 6), None, {}, False, -1, E_PLACE),
            ("misaligned by 4", (20, 16, 4), None, {}, False, -1, E_PLACE),
            ("one sample past the right edge", (W - 15, 16, 4), None, {}, False, -1, E_PLACE),
            ("aligned, one sample past the right edge", (W - 16, 16, 4), None, {"pic_width": W - 1}, False, -1, E_PLACE),
            ("NxN on a 16x16 CU", (16, 16, 4), 3, {}, False, -1, E_NXN),
            ("lossless", (16, 16, 4), None, {"tq_bypass_enabled": 1}, False, -1, E_LOSSLESS)]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_plain_entries_refuse_before_touching_anything(depth):
    """x265amd_check_intra and x265amd_intra_in_inter return the recorded code and leave the recorded text for every refusal, and the picture's units are byte for
    byte what went in.  Nothing is launched before a refusal, so nothing here reads a device result.  One CU on the picture of T.check_intra_case (128x128)."""
    import ctypes as C
    import torch
    c = T.check_intra_case(depth, 701, 2, 2.0)
    L = T.load_hip(depth)
    L.lib.x265amd_last_error.restype = C.c_char_p
    W = c["width"]
    isz = c["preds"].dtype.itemsize
    d_src = [torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1)).cuda() for p in c["src"]]
    d_rec = [torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1)).cuda() for p in c["rec"]]
    planes = np.array([d.data_ptr() for d in d_src], np.uint64)
    rplanes = np.array([d.data_ptr() for d in d_rec], np.uint64)
    d_pred = torch.zeros(T.RD_TILE * isz, dtype=torch.uint8, device="cuda")
    d_recon = torch.zeros(T.RD_TILE * isz, dtype=torch.uint8, device="cuda")
    for name, (x, y, log2), part, fields, null_out, code, text in refusals(W):
        cu = c["cus"][:1].copy()
        cu[0]["x"], cu[0]["y"], cu[0]["log2_size"] = x, y, log2
        si = np.array([c["si"]], T.SLICE_INFO_DT)
        for f, v in fields.items():
            si[0][f] = v
        for entry in ("check_intra", "intra_in_inter"):
            if part is not None and entry != "check_intra":
                continue
            units = np.ascontiguousarray(c["units"].copy())
            before = units.tobytes()
            uo = np.zeros(256, T.CU_UNIT_DT); res = np.zeros(1, T.RD_RESULT_DT); coeff = np.zeros(T.RD_TILE, np.int16); info = np.zeros(4, np.uint64)
            out = None if null_out else T._ptr(res)
            head = (None, T._ptr(si), T._ptr(c["rp"]), T._ptr(units), T._ptr(planes), T._ptr(rplanes), C.c_ssize_t(W), C.c_ssize_t(W // 2), T._ptr(cu))
            tiles = (C.c_uint64(d_pred.data_ptr()), C.c_uint64(d_recon.data_ptr()))
            if entry == "check_intra":
                rc = L.lib.x265amd_check_intra(*head, int(part or 0), T._ptr(uo), *tiles, out, T._ptr(coeff))
            else:
                rc = L.lib.x265amd_intra_in_inter(*head, T._ptr(uo), *tiles, out, T._ptr(coeff), T._ptr(info))
            got = L.lib.x265amd_last_error()
            print("refusal %-40s %-15s depth %2d: rc %d, %r" % (name, entry, depth, rc, got))
            assert (rc, got) == (code, text), (name, entry, rc, got)
            assert units.tobytes() == before, (name, entry)
