"""Residual RD of inter CUs (x265amd_inter_residual_rd) against the reference's own Search::encodeResAndCalcRdInterCU.

CPU (not gpu): the product's host stages -- planning, the decision walk with the bit-counting CABAC coder, the final cost -- are driven with
the oracle executing the transform-chain records, and compared (a) with the reference driver when oracle/_ref is present, (b) with the
committed golden results (tests/golden/inter_rd_golden.npz, generated here from oracle/_ref by tests/golden/make_golden.py).
GPU: the whole entry point (both launches + the walk) against the same golden results."""
import os

import numpy as np
import pytest

import hevc_testlib as T

# (depth, seed, slice type (0 B, 1 P), tuQTMaxInterDepth, psy-rd)
CASES = [(8, 201, 1, 1, 2.0), (8, 202, 0, 2, 2.0), (8, 203, 1, 3, 0.0), (8, 204, 0, 4, 1.0), (10, 205, 1, 2, 2.0), (10, 206, 0, 3, 0.0), (8, 207, 1, 3, 2.0), (8, 208, 0, 1, 0.0)]
GOLD_PATH = os.path.join(T.GOLDEN_DIR, "inter_rd_golden.npz")


def check_golden(res, c, gold, k):
    packed = T.rd_pack(res, c)
    for i, d in enumerate(packed):
        for name, a in d.items():
            want = gold["%d/%d/%s" % (k, i, name)]
            assert np.array_equal(a, want), "case %d CU %d (log2 %d qp %d): %s differs from the reference's result" % (
                k, i, c["cus"][i]["log2_size"], c["cus"][i]["qp"], name)


def test_host_stages_match_golden():
    gold = np.load(GOLD_PATH)
    for k, (depth, seed, st, td, psy) in enumerate(CASES):
        c = T.rd_case(depth, seed, st, td, psy)
        check_golden(T.rd_run_stages_cpu(T.load_hip(depth), T.load_oracle(depth), c), c, gold, k)


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref not built")
def test_host_stages_match_reference_fresh_seeds():
    for k, (depth, seed, st, td, psy) in enumerate([(8, 301, 1, 2, 2.0), (8, 302, 0, 3, 0.0), (10, 303, 0, 4, 2.0), (8, 304, 1, 1, 0.4)]):
        c = T.rd_case(depth, seed, st, td, psy, ncu=12)
        want = T.rd_run_ref(T.load_ref(depth), c)
        T.rd_compare(T.rd_run_stages_cpu(T.load_hip(depth), T.load_oracle(depth), c), want, c, "case %d" % k)


def test_outcomes_are_varied():
    """the golden set exercises skips, transform splits, zeroed roots and mixed coded block flags"""
    gold = np.load(GOLD_PATH)
    skip = split = root0 = mixed = 0
    for k, (depth, seed, st, td, psy) in enumerate(CASES):
        c = T.rd_case(depth, seed, st, td, psy)
        for i in range(len(c["cus"])):
            u = gold["%d/%d/units" % (k, i)]
            skip += int(u[0, 4] == 3); split += int(u[:, 0].max() > 0); root0 += int(not u[:, 1:4].any()); mixed += int(u[:, 1:4].any() and not u[:, 1:4].all())
    assert skip > 0 and split > 5 and root0 > 5 and mixed > 5, (skip, split, root0, mixed)


@pytest.mark.gpu
def test_hip_inter_residual_rd_matches_reference_golden():
    gold = np.load(GOLD_PATH)
    for k, (depth, seed, st, td, psy) in enumerate(CASES):
        c = T.rd_case(depth, seed, st, td, psy)
        check_golden(T.rd_run_hip(T.load_hip(depth), c), c, gold, k)


@pytest.mark.gpu
def test_hip_matches_host_stages_on_a_larger_batch():
    """200 candidates in one call (one launch of ~10^4 transform chains) against the staged CPU run of the same host code"""
    c = T.rd_case(8, 401, 0, 3, 2.0, ncu=200)
    got = T.rd_run_hip(T.load_hip(8), c)
    want = T.rd_run_stages_cpu(T.load_hip(8), T.load_oracle(8), c)
    T.rd_compare(got, want, c, "batch")


# ---- Search::encodeResAndCalcRdSkipCU ----
SKIP_CASES = [(8, 501, 1, 2.0), (8, 502, 0, 0.0), (10, 503, 0, 2.0)]
SKIP_GOLD_PATH = os.path.join(T.GOLDEN_DIR, "skip_rd_golden.npz")


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref not built")
def test_skip_host_stage_matches_reference():
    for k, (depth, seed, st, psy) in enumerate(SKIP_CASES + [(8, 511, 1, 0.6), (10, 512, 1, 0.0)]):
        c = T.skip_case(depth, seed, st, psy)
        T.rd_compare(T.skip_run_host_cpu(T.load_hip(depth), T.load_oracle(depth), c), T.skip_run_ref(T.load_ref(depth), c), c, "skip case %d" % k)


def test_skip_host_stage_matches_golden():
    gold = np.load(SKIP_GOLD_PATH)
    for k, (depth, seed, st, psy) in enumerate(SKIP_CASES):
        c = T.skip_case(depth, seed, st, psy)
        check_golden(T.skip_run_host_cpu(T.load_hip(depth), T.load_oracle(depth), c), c, gold, k)


@pytest.mark.gpu
def test_hip_skip_rd_matches_reference_golden():
    gold = np.load(SKIP_GOLD_PATH)
    for k, (depth, seed, st, psy) in enumerate(SKIP_CASES):
        c = T.skip_case(depth, seed, st, psy)
        check_golden(T.skip_run_hip(T.load_hip(depth), c), c, gold, k)


# ---- what the entries refuse: return code, x265amd_last_error() text and an untouched picture map, as recorded from the library before the walk was split into steps ----
PLAN_PLACED = b"inter_residual_rd: CU outside the picture or misaligned"
PLAN_RANGE = b"inter_residual_rd: transform size range"
RD_LOSSLESS = b"inter_residual_rd: lossless coding is not supported"
WALK_RDOQ = b"inter_rd_walk: with RDOQ the transform units are quantised during the walk: use x265amd_inter_residual_rd"
FILLER = 0xAB


class Entries:
    """two merged 2Nx2N CUs (every entry takes those) on the 128x128 picture of T.skip_case, and the arguments of each entry by name.  Without `device` the picture and
    the tiles are host memory or made-up addresses: the refusals tested that way come before anything reads them."""

    def __init__(self, depth, device=False):
        import ctypes as C
        c = T.skip_case(depth, 521, 1, 2.0, ncu=2)
        self.C, self.L, self.W, self.n = C, T.load_hip(depth), c["width"], len(c["cus"])
        self.L.lib.x265amd_last_error.restype = C.c_char_p
        self.L.lib.x265amd_inter_rd_scratch_bytes.restype = C.c_size_t
        self.tile = T.RD_TILE * c["preds"].dtype.itemsize
        self.si, self.rp, self.cus, self.cu_units = np.array([c["si"]], T.SLICE_INFO_DT), c["rp"].copy(), c["cus"].copy(), c["cu_units"].copy()
        self.units = np.ascontiguousarray(c["units"].copy())
        self.before = self.units.tobytes()
        self.keep = [np.ascontiguousarray(p) for p in c["src"]] + [np.ascontiguousarray(c["preds"])]
        if device:
            import torch
            self.keep = [torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda() for a in self.keep] + [torch.zeros(self.n * self.tile, dtype=torch.uint8, device="cuda")]
            torch.cuda.synchronize()
            addr = [d.data_ptr() for d in self.keep]
        else:
            addr = [a.ctypes.data for a in self.keep] + [0x10000]
        self.planes, self.pred, self.recon = np.array(addr[:3], np.uint64), addr[3], addr[4]
        self.scratch = 0x20000 if device else np.zeros(self.n * self.L.lib.x265amd_inter_rd_scratch_bytes(), np.uint8).ctypes.data
        self.jobs = np.zeros(64, T.TU_JOB_DT)
        self.tu_res, self.levels, self.sel = np.zeros(64, T.TU_RESULT_DT), np.zeros(self.n * T.RD_SCRATCH_ELEMS, np.int16), np.zeros(self.n * T.RD_SEL_BYTES, np.uint8)
        self.meas = np.full(self.n, FILLER, np.uint8).repeat(T.CU_MEASURE_DT.itemsize).view(T.CU_MEASURE_DT)
        self.out = np.full(self.n * T.RD_RESULT_DT.itemsize, FILLER, np.uint8).view(T.RD_RESULT_DT)
        self.coeff = np.full(self.n * T.RD_TILE, FILLER, np.uint8).view(np.int8).astype(np.int16)
        self.tile_addrs = np.array([self.pred + i * self.tile for i in range(self.n)], np.uint64)

    def args(self, entry, stream=None):
        C, p = self.C, T._ptr
        pic = dict(h_src=p(self.planes), stride=C.c_ssize_t(self.W), cstride=C.c_ssize_t(self.W // 2))
        tiles = dict(d_pred=C.c_uint64(self.pred), d_recon=C.c_uint64(self.recon), tile_bytes=C.c_size_t(self.tile))
        if entry == "inter_rd_plan":
            return dict(si=p(self.si), cus=p(self.cus), n=self.n, cu_units=p(self.cu_units), **pic, d_pred=C.c_uint64(self.pred), tile_bytes=C.c_size_t(self.tile),
                        scratch=C.c_uint64(self.scratch), jobs_out=p(self.jobs), cap=len(self.jobs))
        if entry == "inter_rd_walk":
            return dict(si=p(self.si), rp=p(self.rp), units=p(self.units), cus=p(self.cus), n=self.n, cu_units=p(self.cu_units), res=p(self.tu_res), levels=p(self.levels),
                        levels_stride=C.c_size_t(T.RD_SCRATCH_ELEMS * 2), zero_meas=p(self.meas), sel=p(self.sel), out=p(self.out), coeff_out=p(self.coeff))
        if entry == "skip_rd_host":
            return dict(si=p(self.si), rp=p(self.rp), units=p(self.units), cus=p(self.cus), n=self.n, cu_units=p(self.cu_units), meas=p(self.meas), out=p(self.out))
        if entry == "inter_residual_rd":
            return dict(stream=stream, si=p(self.si), rp=p(self.rp), units=p(self.units), **pic, cus=p(self.cus), n=self.n, cu_units=p(self.cu_units), **tiles,
                        out=p(self.out), coeff_out=p(self.coeff))
        if entry == "skip_rd":
            return dict(stream=stream, si=p(self.si), rp=p(self.rp), units=p(self.units), **pic, cus=p(self.cus), n=self.n, cu_units=p(self.cu_units), **tiles, out=p(self.out))
        if entry == "measure_tiles":
            return dict(stream=stream, **pic, cus=p(self.cus), n=self.n, d_tiles=C.c_uint64(self.pred), tile_bytes=C.c_size_t(self.tile), out=p(self.meas))
        assert entry == "measure_tile_list"
        return dict(stream=stream, **pic, cus=p(self.cus), n=self.n, tile_addrs=p(self.tile_addrs), out=p(self.meas))

    def refused(self, what, entry, code, text, stream=None, **change):
        """calls the entry with the named arguments replaced; the return code, the text left behind and the picture map"""
        a = self.args(entry, stream)
        assert set(change) <= set(a), (entry, change)
        a.update(change)
        rc = getattr(self.L.lib, "x265amd_" + entry)(*a.values())
        got = self.L.lib.x265amd_last_error()
        print("refusal %-22s %-34s depth %2d: rc %d, %r" % (entry, what, self.L.depth, rc, got))
        assert rc == code and (text is None or got == text), (entry, what, rc, got)
        assert self.units.tobytes() == self.before, (entry, what)

    def outputs(self):
        return self.out.tobytes() + self.meas.tobytes() + self.coeff.tobytes() + self.jobs.tobytes() + self.cu_units.tobytes()


POINTERS = {"inter_rd_plan": ("si", "cus", "cu_units", "h_src"),
            "inter_rd_walk": ("si", "rp", "units", "cus", "cu_units", "res", "levels", "zero_meas", "sel", "out"),
            "skip_rd_host": ("si", "rp", "units", "cus", "cu_units", "meas", "out"),
            "inter_residual_rd": ("si", "rp", "units", "h_src", "cus", "cu_units", "d_pred", "d_recon", "out"),
            "skip_rd": ("si", "rp", "units", "h_src", "cus", "cu_units", "d_pred", "d_recon", "out"),
            "measure_tiles": ("h_src", "cus", "d_tiles", "out"),
            "measure_tile_list": ("h_src", "cus", "tile_addrs", "out")}
NULL_TEXT = {"inter_rd_plan": b"inter_rd_plan: null argument", "inter_rd_walk": b"inter_rd_walk: null argument", "skip_rd_host": b"skip_rd: null argument",
             "inter_residual_rd": b"inter_residual_rd: null argument", "skip_rd": b"skip_rd: null argument", "measure_tiles": b"measure_tiles: null argument",
             "measure_tile_list": b"measure_tile_list: null argument"}


@pytest.mark.parametrize("depth", [8, 10])
def test_entries_refuse_before_touching_anything(depth):
    """No HIP call comes before these refusals, so they are checked without a GPU: every entry's null arguments and negative count, the host stages' own refusals, and what
    the device entries refuse ahead of their first allocation.  n == 0 is no refusal: X265AMD_OK with every output as it was."""
    import ctypes as C
    e = Entries(depth)
    untouched = e.outputs()
    for entry, names in POINTERS.items():
        for name in names:
            e.refused("null " + name, entry, -1, NULL_TEXT[entry], **{name: None if name not in ("d_pred", "d_recon", "d_tiles") else C.c_uint64(0)})
        e.refused("n < 0", entry, -1, NULL_TEXT[entry], n=-1)

    def moved(dx):
        cus = e.cus.copy()
        cus[0]["x"] += dx
        return T._ptr(cus), cus
    def slice_with(**fields):
        si = e.si.copy()
        for f, v in fields.items():
            si[0][f] = v
        return T._ptr(si), si
    def params_with(**fields):
        rp = e.rp.copy()
        for f, v in fields.items():
            rp[0][f] = v
        return T._ptr(rp), rp

    # x265amd_inter_rd_plan
    ptr, keep = moved(4)
    e.refused("CU misaligned by 4", "inter_rd_plan", -1, PLAN_PLACED, cus=ptr)
    cus = e.cus.copy()
    cus[0]["x"] = e.W - (1 << int(cus[0]["log2_size"]))
    ptr, keep = slice_with(pic_width=e.W - 1)
    e.refused("CU one sample past the right edge", "inter_rd_plan", -1, PLAN_PLACED, si=ptr, cus=T._ptr(cus))
    cus = e.cus.copy()
    cus[0]["x"], cus[0]["y"], cus[0]["log2_size"] = 0, 0, 3         # an 8x8 CU two transform depths down: 2x2 units
    for what, fields in (("tu_log2_min 1", dict(tu_log2_min=1, tu_max_depth_inter=3)), ("tu_log2_max 6", dict(tu_log2_max=6)), ("tu_log2_min above tu_log2_max", dict(tu_log2_min=5, tu_log2_max=4))):
        ptr, keep = slice_with(**fields)
        e.refused(what, "inter_rd_plan", -1, PLAN_RANGE, si=ptr, cus=T._ptr(cus))
    nj = e.L.lib.x265amd_inter_rd_plan(*{**e.args("inter_rd_plan"), "jobs_out": None, "cap": 0}.values())
    assert 0 < nj <= len(e.jobs)
    e.refused("cap one short", "inter_rd_plan", -1, b"inter_rd_plan: job array too small", cap=nj - 1)
    # x265amd_inter_rd_walk
    ptr, keep = params_with(rdoq_level=1)
    e.refused("rdoq_level 1", "inter_rd_walk", -1, WALK_RDOQ, rp=ptr)
    ptr, keep = slice_with(tq_bypass_enabled=1)
    e.refused("lossless", "inter_rd_walk", -1, RD_LOSSLESS, si=ptr)
    # x265amd_skip_rd_host
    e.refused("lossless", "skip_rd_host", -1, b"skip_rd: lossless coding is not supported", si=ptr)
    ptr, keep = moved(4)
    e.refused("CU misaligned by 4", "skip_rd_host", -1, b"skip_rd: CU outside the picture or misaligned", cus=ptr)
    # the device entries, ahead of their first allocation
    short = C.c_size_t(e.tile - 1)
    e.refused("tile one byte too small", "inter_residual_rd", -1, b"inter_residual_rd: tile too small", tile_bytes=short)
    e.refused("tile one byte too small", "skip_rd", -1, b"skip_rd: tile too small", tile_bytes=short)
    ptr, keep = slice_with(tq_bypass_enabled=1)
    e.refused("lossless", "inter_residual_rd", -1, RD_LOSSLESS, si=ptr)
    assert e.outputs() == untouched
    for entry in ("inter_residual_rd", "skip_rd", "measure_tiles", "measure_tile_list"):
        e.refused("n == 0", entry, 0, None, n=0)
    assert e.outputs() == untouched


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_entries_refuse_behind_their_first_device_work(depth):
    """x265amd_inter_residual_rd meets a misaligned CU in its plan, behind the scratch allocation; x265amd_skip_rd meets lossless coding in its host stage, behind the
    measurement.  Both leave the picture map as it was."""
    e = Entries(depth, device=True)
    cus = e.cus.copy()
    cus[0]["x"] += 4
    si = e.si.copy()
    si[0]["tq_bypass_enabled"] = 1
    with T.call_stream(e.L) as st_:
        e.refused("CU misaligned by 4", "inter_residual_rd", -1, PLAN_PLACED, stream=st_, cus=T._ptr(cus))
        e.refused("lossless", "skip_rd", -1, b"skip_rd: lossless coding is not supported", stream=st_, si=T._ptr(si))
