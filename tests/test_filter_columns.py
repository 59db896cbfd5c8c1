"""The column forms of the in-loop filter entry points under seeded schedules: what the filter thread of a picture (x265amd_encoder::filterRowsCols,
csrc/encoder_frame.hip) drives per column chunk while the picture's analysis still advances -- x265amd_deblock_units_rect, x265amd_deblock_rows_cols,
x265amd_sao_stats_rows_cols, x265amd_sao_rdo_cols, x265amd_sao_apply_rows_cols, x265amd_extend_border_band_420 -- in the order and with the arguments that
x265amd_filter_plan (host/filter_plan.cpp, the function the filter thread itself calls) gives for a sequence of snapshots of the analysis.

Expected: the same picture through the picture-wide forms on the CPU (the oracle's deblocking, SAO statistics, offsets and borders, which tests/test_deblock.py,
test_sao.py and test_planes.py pin to the reference; the product's whole-picture SAO decision in between, which the host test below pins the chunked decision to).
Integer paths: every comparison is exact.

Whatever a chunk has not produced yet is poisoned on the device -- the deblocking records outside the rectangles uploaded so far, the statistics, the SAO
parameters, the final planes with all their margins, the margins of the reconstruction -- so a read of something that is not final yet shows as a wrong value.
After every sweep the samples the sweep has published must already be final: for CTU row k the lines of the row in the luma columns [0, pub_x[k]), their left
margin once pub_x[k] > 0, their right margin once pub_x[k] == width, with row 0 the top margin above those columns and with the last row the bottom margin below
them, chroma at half of everything.  That is what a picture that references this one may read: gateRefWait (csrc/encoder_frame.hip) admits the samples up to
column xMax of the CTU rows of lines yMin .. yMax (clamped into the picture) once published(row) >= xMax + 1, the right margin with published(row) == width; a
block that lies in the left margin alone (xMax < 0) waits for nothing there, but its CTU only starts behind gateCtuReady, which has seen every row it can reach
published beyond column 0.

Records and SAO parameters are passed as device memory here (the C entry points take either; the encoder itself once had this copy form behind two switches); the
encoder's form, mapped memory the kernels read in place, stays covered by the stream fixtures only (tests/test_encoder_api.py, test_encoder_full_size.py).

What these tests were seen to catch (value-only changes on a scratch copy, 8-bit library, one run each):
  - a chunk's seam edge nobody's (x265amd_deblock_rows_cols: xvEnd = 16 * ctu_col_end): test_filter_columns_product, 200x72 wavefront schedule, chunk minimum 1, sweep 1:
    plane 0 x 62 y 8 (tests/test_deblock.py and test_row_forms.py still pass: whole rows have no seam);
  - the first sample column of a range not offset (k_sao_apply: x <= x0): product and contract tests, first at 72x200 sweep 0, plane 0 x -96 y -80 (the corner repeats column 0);
  - the right corners never written (k_extend_band / k_extend_band3: to = xb): product, contract and band tests, first at 72x200 sweep 0, plane 0 x 72 y -80;
  - the row's entropy state not taken over from `carry` (sao_rdo.cpp): test_sao_rdo_cols_equal_picture, 264x200 B unreferenced, single schedule, row 2 CTUs 3..5, CTU 4;
  - publishing 64 * c1 instead of 64 * c1 - 8 (filter_plan.cpp): product test, 200x72 wavefront schedule sweep 0: plane 2 x 31 y 16 (an edge class at chroma column
    32 * c1 - 1 reads column 32 * c1, which the next chunk's horizontal edges still change).  Publishing 64 * c1 - 2 passes everything here."""
import ctypes as C
import functools

import numpy as np
import pytest

import hevc_testlib as T

_ptr = lambda a: a.ctypes.data_as(C.c_void_p)

# (width, height, slice_b, bypass, seed): the last CTU column 8 samples wide and the last row 8 lines high (y4t == y4e: nothing left to deblock in the FULL step); two
# CTU rows; the geometries of tests/test_row_forms.py; 11 CTU columns (chunks on both sides of the fuse limit of x265amd_deblock_rows_cols)
PRODUCT_GEOMETRIES = ((72, 200, True, False, 11), (200, 72, False, False, 19), (200, 136, True, False, 13), (200, 136, False, False, 14), (384, 264, True, True, 15),
                      (648, 136, False, False, 16))
# a picture of one CTU row or one CTU column never takes the column path in the encoder: the entry points' contract only
CONTRACT_GEOMETRIES = ((64, 64, True, False, 21), (320, 64, True, False, 22), (64, 200, True, False, 23))
CHUNK_MINIMA = (1, 2, "w")


def product_cases():
    """every (geometry, schedule kind, chunk minimum, early TOP) with the schedule's seed"""
    out = []
    for g, geo in enumerate(PRODUCT_GEOMETRIES):
        for s, kind in enumerate(T.FILTER_SCHEDULES):
            for m in CHUNK_MINIMA:
                for early in (1, 0):
                    out.append((geo, kind, m, early, 1000 + 10 * g + s))
    return out


def _sweeps(L, geo, kind, m, early, seed, max_step=None):
    w, h = geo[0], geo[1]
    ctuW, ctuH = (w + 63) // 64, (h + 63) // 64
    sched = T.filter_schedule(kind, seed, ctuW, ctuH, max_step)
    return sched, T.filter_sweeps(L, w, h, sched, *T.filter_min_chunks(m, ctuW), early)


def test_filter_schedules_cover():
    """host code: the schedules hold what they claim and the planner's answers to them hold every kind of chunk the GPU test is there for"""
    L = T.load_hip(8)
    seen = dict(one=0, wide=0, unaligned=0, top_full_rows=0, full_then_top=0, three_chunks=0)
    pairs = set()
    for (geo, kind, m, early, seed) in product_cases():
        w, h = geo[0], geo[1]
        ctuW, ctuH = (w + 63) // 64, (h + 63) // 64
        sched, sweeps = _sweeps(L, geo, kind, m, early, seed)
        pairs |= {("km", kind, m), ("kg", kind, geo[:2])}
        # the schedule is what its name says
        prev = [0] * ctuH
        for snap in sched:
            assert all(0 <= a <= ctuW and a >= p for a, p in zip(snap, prev)), (kind, snap, prev)
            if kind in ("wavefront", "single"):
                assert all(snap[r - 1] == ctuW or snap[r] <= max(0, snap[r - 1] - 1) for r in range(1, ctuH)), (kind, snap)
            if kind == "raster":
                assert all(snap[r - 1] == ctuW or snap[r] == 0 for r in range(1, ctuH)), snap
            if kind == "single":
                assert sum(snap) == sum(prev) + 1, (snap, prev)
            prev = snap
        assert prev == [ctuW] * ctuH
        if kind == "all":
            assert len(sched) == 1
        if kind == "wavefront" and ctuH > 2 and ctuW > 3:
            assert any(sum(0 < a < ctuW for a in snap) >= 2 for snap in sched), "no snapshot with two rows in flight"
        # the sweeps: every CTU of every row in exactly one TOP and one FULL chunk, in column order; every sample column finished once
        top = [[] for _ in range(ctuH)]; full = [[] for _ in range(ctuH)]; fin = [[] for _ in range(ctuH)]
        for sw in sweeps:
            st = sw["steps"]
            for s in st:
                (top if s["kind"] == T.FILTER_TOP else full)[s["row"]].append((int(s["col_begin"]), int(s["col_end"])))
                n = s["col_end"] - s["col_begin"]
                seen["one"] += n == 1; seen["wide"] += n > 8
            for f in sw["finish"]:
                fin[f["row"]].append((int(f["x_begin"]), int(f["x_end"])))
                seen["unaligned"] += f["x_end"] % 64 != 0
            tops = {int(s["row"]) for s in st if s["kind"] == T.FILTER_TOP}; fulls = {int(s["row"]) for s in st if s["kind"] == T.FILTER_FULL}
            seen["top_full_rows"] += bool(tops and fulls and (len(tops | fulls) > 1))
            seen["full_then_top"] += any(r + 1 in tops for r in fulls)
        for r in range(ctuH):
            for lst, end in ((top[r], ctuW), (full[r], ctuW), (fin[r], w)):
                assert lst and lst[0][0] == 0 and lst[-1][1] == end and all(a[1] == b[0] for a, b in zip(lst, lst[1:])), (geo, kind, m, early, r, lst)
            seen["three_chunks"] += len(full[r]) >= 3
    assert all(v > 0 for v in seen.values()), seen
    for kind in T.FILTER_SCHEDULES:
        assert all(("km", kind, m) in pairs for m in CHUNK_MINIMA) and all(("kg", kind, g[:2]) in pairs for g in PRODUCT_GEOMETRIES)


def test_deblock_units_rect_equal_picture():
    """host code: the deblocking records rectangle by rectangle as the TOP steps of every schedule ask for them, into a poisoned array, equal the picture-wide
    records; a call writes nothing outside its rectangle"""
    L = T.load_hip(8)
    for (w, h, seed) in ((200, 136, 1), (72, 200, 2), (648, 136, 3)):
        for st in (0, 1):
            c = T.cabac_case(seed, w, h, st)
            w4, h4 = w // 4, h // 4
            ctuW, ctuH = (w + 63) // 64, (h + 63) // 64
            rng = np.random.default_rng(seed)
            motion = np.zeros(w4 * h4, T.MV_UNIT_DT)
            motion["pred_mode"] = c["units"]["pred_mode"].reshape(-1)
            motion["inter_dir"] = rng.integers(1, 4 if st == 0 else 2, w4 * h4)
            motion["ref_idx"] = rng.integers(0, 2, (w4 * h4, 2))
            motion["mv"] = rng.integers(-40, 41, (w4 * h4, 2, 2))
            info = np.zeros(1, T.MVPRED_INFO_DT)
            info["pic_width"], info["pic_height"], info["num_ref_idx"] = w, h, (2, 2 if st == 0 else 0)
            info["ref_poc"][0, 0, :2] = (4, 2); info["ref_poc"][0, 1, :2] = (8, 4)
            si = np.array([c["si"]], T.SLICE_INFO_DT)
            units = np.ascontiguousarray(c["units"].reshape(-1))
            whole = np.zeros(w4 * h4, T.DB_UNIT_DT)
            assert L.lib.x265amd_deblock_units(_ptr(si), _ptr(info), _ptr(units), _ptr(motion), _ptr(whole)) == 0
            whole2 = whole.view(np.uint8).reshape(h4, w4, 12)
            for k, kind in enumerate(T.FILTER_SCHEDULES):
                for m in CHUNK_MINIMA:
                    for early in (1, 0):
                        sched = T.filter_schedule(kind, 50 + k, ctuW, ctuH)
                        got = np.full((h4, w4, 12), 0xA5, np.uint8)
                        written = np.zeros((h4, w4), bool)
                        for sw in T.filter_sweeps(L, w, h, sched, *T.filter_min_chunks(m, ctuW), early):
                            for s in sw["steps"]:
                                if s["kind"] != T.FILTER_TOP:
                                    continue
                                y0, y1, x0, x1 = int(s["y4_begin"]), int(s["rec_y4_end"]), int(s["rec_x4_begin"]), int(s["rec_x4_end"])
                                before = got.copy()
                                assert L.lib.x265amd_deblock_units_rect(_ptr(si), _ptr(info), _ptr(units), _ptr(motion), _ptr(got), y0, y1, x0, x1) == 0
                                assert np.array_equal(got[y0:y1, x0:x1], whole2[y0:y1, x0:x1]), (w, h, st, kind, m, early, y0, y1, x0, x1)
                                before[y0:y1, x0:x1] = got[y0:y1, x0:x1]
                                assert np.array_equal(before, got), ("written outside the rectangle", w, h, st, kind, m, early, y0, y1, x0, x1)
                                written[y0:y1, x0:x1] = True
                        assert written.all() and np.array_equal(got, whole2), (w, h, st, kind, m, early)


_STAT_POISON = np.int32(-0x5A5A5A5B)            # 0xA5A5A5A5


def _param_poison(n):
    p = np.zeros(n, T.SAO_CTU_DT)
    p["type"] = 1; p["bandPos"] = 0xA5; p["offset"] = 3; p["pad"] = 0xA5        # an enabled type with non-zero offsets
    return p


def test_sao_rdo_cols_equal_picture():
    """host code: the SAO decision chunk by chunk, one carry buffer per CTU row, equals the whole-picture decision (two frame threads); the statistics of the CTUs
    right of the chunk and the parameters not decided yet are poison (a CTU may read its own statistics and decided neighbours' parameters only)"""
    L = T.load_hip(8)
    L.lib.x265amd_sao_rdo.argtypes = L.lib.x265amd_sao_rdo_cols.argtypes = None
    enabled = 0
    for (W, H, seed, st, referenced) in ((264, 200, 3, 1, 1), (264, 200, 4, 0, 0), (264, 200, 5, 0, 1), (264, 200, 6, 2, 1), (648, 136, 7, 1, 1), (72, 200, 8, 1, 0)):
        c = T.cabac_case(seed, W, H, st)
        rng = np.random.default_rng(seed)
        ctuW, ctuH = (W + 63) // 64, (H + 63) // 64
        nctu = ctuW * ctuH
        count = rng.integers(0, 400, nctu * 3 * 5 * 32).astype(np.int32)
        org = (rng.integers(-3, 4, count.shape) * count).astype(np.int32)
        si = np.array([c["si"]], T.SLICE_INFO_DT)
        units = np.ascontiguousarray(c["units"].reshape(-1))
        want = np.zeros(nctu, T.SAO_CTU_DT); flags = np.zeros(2, np.int32); rate = np.zeros(8, np.float64)
        assert L.lib.x265amd_sao_rdo(_ptr(si), referenced, 2, 0, 69, _ptr(units), _ptr(count), _ptr(org), _ptr(rate), _ptr(want), _ptr(flags)) == 0
        enabled += int((want["type"] >= 0).sum())
        for k, kind in enumerate(T.FILTER_SCHEDULES):
            for m in CHUNK_MINIMA:
                sched = T.filter_schedule(kind, 70 + k, ctuW, ctuH)
                got = _param_poison(nctu)
                cnt = np.full_like(count, _STAT_POISON); og = np.full_like(org, _STAT_POISON)
                carry = np.full((ctuH, T.SAO_CARRY_BYTES), 0xA5, np.uint8)
                for sw in T.filter_sweeps(L, W, H, sched, *T.filter_min_chunks(m, ctuW), 1):
                    for s in sw["steps"]:
                        if s["kind"] != T.FILTER_FULL:
                            continue
                        r, c0, c1 = int(s["row"]), int(s["col_begin"]), int(s["col_end"])
                        sl = slice((r * ctuW + c0) * 480, (r * ctuW + c1) * 480)
                        cnt[sl] = count[sl]; og[sl] = org[sl]
                        fl = np.zeros(2, np.int32)
                        assert L.lib.x265amd_sao_rdo_cols(_ptr(si), referenced, 2, 0, 69, _ptr(units), _ptr(cnt), _ptr(og), _ptr(got), _ptr(fl), r, c0, c1, _ptr(carry[r])) == 0
                        assert fl.tolist() == flags.tolist()
                        a, b = r * ctuW + c0, r * ctuW + c1
                        assert got[a:b].tobytes() == want[a:b].tobytes(), "%dx%d slice type %d referenced %d, %s schedule, chunk minimum %s: row %d CTUs %d..%d: first differing CTU %d" % (
                            W, H, st, referenced, kind, m, r, c0, c1, c0 + int(np.nonzero(got[a:b] != want[a:b])[0][0]))
                assert got.tobytes() == want.tobytes(), (W, H, st, referenced, kind, m)
    assert enabled > 0, "the decision switched SAO off everywhere: the case tests nothing"


# ---------------------------------------------------------------- on the device ----------------------------------------------------------------
_RECORD_POISON = np.array([(1 | 2 | 8 | 16 | 32 | 64, 51, (-1, -1), ((0, 0), (0, 0)))], T.DB_UNIT_DT)      # every edge marked, intra, QP 51 (all table indices are clipped)


@functools.lru_cache(maxsize=4)
def _case(depth, geo):
    w, h, slice_b, bypass, seed = geo
    c = T.filter_case(depth, seed, w, h, slice_b=slice_b, bypass=bypass)
    return c, T.filter_case_expected(T.load_oracle(depth), T.load_hip(depth), c)


class _Device:
    """the picture's buffers on the device, poisoned, and the calls of one sweep"""

    def __init__(self, L, c, exp):
        import torch
        self.torch, self.L, self.c, self.exp = torch, L, c, exp
        self.isz = c["rec"][0].itemsize
        self.tdt = torch.uint8 if self.isz == 1 else torch.int16
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda().view(self.tdt)
        self.rec = [up(p) for p in c["rec"]]; self.fenc = [up(p) for p in c["fenc"]]; self.F = [up(p) for p in exp["F"]]
        self.fin = [torch.full_like(t, c["poison"]) for t in self.rec]
        self.w4, self.h4 = c["width"] // 4, c["height"] // 4
        self.units_src = torch.from_numpy(c["units"].view(np.uint8).reshape(self.h4, self.w4, 12).copy()).cuda()
        self.units = torch.from_numpy(np.tile(_RECORD_POISON.view(np.uint8), self.h4 * self.w4).reshape(self.h4, self.w4, 12).copy()).cuda()
        n = c["nctu"] * 480
        self.cnt = torch.full((n,), int(_STAT_POISON), dtype=torch.int32, device="cuda"); self.org = torch.full((n,), int(_STAT_POISON), dtype=torch.int32, device="cuda")
        self.h_cnt = np.full(n, _STAT_POISON, np.int32); self.h_org = np.full(n, _STAT_POISON, np.int32)
        self.h_par = _param_poison(c["nctu"])
        self.par = torch.from_numpy(self.h_par.view(np.uint8).copy()).cuda()
        self.carry = np.full((c["ctuH"], T.SAO_CARRY_BYTES), 0xA5, np.uint8)
        self.cu_units = c["cu_units"].copy()
        org = (c["org"][0], c["org"][1], c["org"][1])
        self.tab = lambda ts: np.array([t.data_ptr() + o * self.isz for t, o in zip(ts, org)], np.uint64)
        self.ptr = lambda ts, k: C.c_void_p(ts[k].data_ptr() + org[k] * self.isz)
        L.lib.x265amd_sao_rdo_cols.argtypes = None

    def deblock(self, s):
        c, L = self.c, self.L
        assert L.lib.x265amd_deblock_rows_cols(None, self.ptr(self.rec, 0), self.ptr(self.rec, 1), self.ptr(self.rec, 2), C.c_int64(c["stride"]), C.c_int64(c["cstride"]),
                                               c["width"], c["height"], C.c_void_p(self.units.data_ptr()), c["beta"], c["tc"], c["cb"], c["cr"], c["bypass"], 3,
                                               int(s["y4_begin"]), int(s["y4_end"]), int(s["col_begin"]), int(s["col_end"])) == 0

    def sweep(self, sw):
        """the calls of filterRowsCols for one sweep, two synchronisations"""
        c, L, torch = self.c, self.L, self.torch
        geom = (C.c_int64(c["stride"]), C.c_int64(c["cstride"]), c["width"], c["height"])
        fulls = []
        for s in sw["steps"]:
            if s["kind"] == T.FILTER_TOP:
                y0, y1, x0, x1 = int(s["y4_begin"]), int(s["rec_y4_end"]), int(s["rec_x4_begin"]), int(s["rec_x4_end"])
                self.units[y0:y1, x0:x1] = self.units_src[y0:y1, x0:x1]         # what x265amd_deblock_units_rect has produced at this step
                self.deblock(s)
            else:
                if s["y4_end"] > s["y4_begin"]:
                    self.deblock(s)
                assert L.lib.x265amd_sao_stats_rows_cols(None, _ptr(self.tab(self.rec)), _ptr(self.tab(self.fenc)), *geom, C.c_void_p(self.cnt.data_ptr()), C.c_void_p(self.org.data_ptr()),
                                                         int(s["row"]), int(s["row"]) + 1, int(s["col_begin"]), int(s["col_end"])) == 0
                fulls.append(s)
        if fulls:
            torch.cuda.synchronize()
            for s in fulls:
                r, c0, c1 = int(s["row"]), int(s["col_begin"]), int(s["col_end"])
                a, b = r * c["ctuW"] + c0, r * c["ctuW"] + c1
                self.h_cnt[a * 480:b * 480] = self.cnt[a * 480:b * 480].cpu().numpy(); self.h_org[a * 480:b * 480] = self.org[a * 480:b * 480].cpu().numpy()
                fl = np.zeros(2, np.int32)
                assert L.lib.x265amd_sao_rdo_cols(_ptr(c["si"]), c["referenced"], 2, 0, 69, _ptr(self.cu_units), _ptr(self.h_cnt), _ptr(self.h_org), _ptr(self.h_par), _ptr(fl),
                                                  r, c0, c1, _ptr(self.carry[r])) == 0
                self.par[a * 20:b * 20] = torch.from_numpy(self.h_par[a:b].view(np.uint8).copy()).cuda()
        mx, my = c["margin"]
        for f in sw["finish"]:
            k, x0, x1 = int(f["row"]), int(f["x_begin"]), int(f["x_end"])
            assert L.lib.x265amd_sao_apply_rows_cols(None, _ptr(self.tab(self.rec)), _ptr(self.tab(self.fin)), *geom, C.c_void_p(self.par.data_ptr()), k, k + 1, x0, x1) == 0
            assert L.lib.x265amd_extend_border_band_420(None, self.ptr(self.fin, 0), self.ptr(self.fin, 1), self.ptr(self.fin, 2), *geom, mx, my,
                                                        int(f["y_begin"]), int(f["y_end"]), x0, x1, int(x0 == 0), int(x1 == c["width"])) == 0
        torch.cuda.synchronize()

    def check_published(self, sw, what):
        """every sample the sweeps so far have published holds its final value: per padded line, the first column that differs lies beyond what is published"""
        c, torch = self.c, self.torch
        W, H = c["width"], c["height"]
        mx, my = c["margin"]
        for k in range(3):
            sh = 1 if k else 0
            st = self.fin[k].shape[1]
            ax, ay, h = mx >> sh, my >> sh, H >> sh
            need = np.zeros(h + 2 * ay, np.int64)
            for r, X in enumerate(sw["pub_x"]):
                if X <= 0:
                    continue
                n = st if X == W else ax + (int(X) >> sh)
                y0, y1 = ay + ((64 * r) >> sh), ay + (min(H, 64 * r + 64) >> sh)
                need[0 if r == 0 else y0:h + 2 * ay if r == c["ctuH"] - 1 else y1] = n
            cols = torch.arange(st, device="cuda", dtype=torch.int32)
            first = torch.where(self.fin[k] != self.F[k], cols, torch.tensor(st, device="cuda", dtype=torch.int32)).amin(1).cpu().numpy()
            bad = np.nonzero(first < need)[0]
            if len(bad):
                y, x = int(bad[0]), int(first[bad[0]])
                raise AssertionError("%s: plane %d x %d y %d (margins: negative / beyond the picture) is published but holds %d, final value %d; pub_x %s; steps %s; finish %s" % (
                    what, k, x - ax, y - ay, int(self.fin[k][y, x]), int(self.F[k][y, x]), sw["pub_x"].tolist(), sw["steps"].tolist(), sw["finish"].tolist()))

    def check_end(self, what):
        c, exp = self.c, self.exp
        dt = c["rec"][0].dtype
        dn = lambda t, like: t.cpu().numpy().view(np.uint8).view(dt).reshape(like.shape)
        for k in range(3):
            got = dn(self.rec[k], exp["D"][k])
            assert np.array_equal(got, exp["D"][k]), (what, "deblocked plane", k, _first_diff(got, exp["D"][k], c, k))
        cnt, org = self.cnt.cpu().numpy(), self.org.cpu().numpy()
        for name, got, want in (("count", cnt, exp["count"]), ("offsetOrg", org, exp["org"])):
            if not np.array_equal(got, want):
                i = int(np.nonzero(got != want)[0][0])
                raise AssertionError((what, name, "ctu %d plane %d type %d class %d" % (i // 480, i // 160 % 3, i // 32 % 5, i % 32), int(got[i]), int(want[i])))
        assert self.h_par.tobytes() == exp["params"].tobytes(), (what, "SAO parameters", np.nonzero(self.h_par != exp["params"])[0][:4].tolist())
        for k in range(3):
            got = dn(self.fin[k], exp["F"][k])
            assert np.array_equal(got, exp["F"][k]), (what, "final plane", k, _first_diff(got, exp["F"][k], c, k))


def _first_diff(got, want, c, k):
    ys, xs = np.nonzero(got != want)
    sh = 1 if k else 0
    return "first of %d at x %d y %d: %d, want %d" % (len(ys), xs[0] - (c["margin"][0] >> sh), ys[0] - (c["margin"][1] >> sh), got[ys[0], xs[0]], want[ys[0], xs[0]])


def _vacuity(c, exp):
    """(samples the deblocking changed, samples SAO changed, CTUs with SAO on)"""
    mx, my = c["margin"]
    db = sao = 0
    for k in range(3):
        sh = 1 if k else 0
        area = (slice(my >> sh, (my + c["height"]) >> sh), slice(mx >> sh, (mx + c["width"]) >> sh))
        db += int((exp["D"][k][area] != c["rec"][k][area]).sum()); sao += int((exp["F"][k][area] != exp["D"][k][area]).sum())
    return db, sao, int((exp["params"]["type"] >= 0).any(1).sum())


def _run(L, depth, geo, kind, m, early, seed, every=1, max_step=None):
    c, exp = _case(depth, geo)
    sched, sweeps = _sweeps(L, geo, kind, m, early, seed, max_step)
    what = "%dx%d depth %d %s schedule (seed %d), chunk minimum %s, early top %d" % (geo[0], geo[1], depth, kind, seed, m, early)
    dev = _Device(L, c, exp)
    for i, sw in enumerate(sweeps):
        dev.sweep(sw)
        if i % every == 0 or i == len(sweeps) - 1:
            dev.check_published(sw, "%s, sweep %d of %d" % (what, i, len(sweeps)))
    dev.check_end(what)
    return _vacuity(c, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_filter_columns_product(depth):
    """the geometries the encoder takes the column path for, under every schedule kind, chunk minimum and with the early TOP step on and off"""
    L = T.load_hip(depth)
    db = sao = 0
    for geo in PRODUCT_GEOMETRIES:
        for (g, kind, m, early, seed) in product_cases():
            if g != geo:
                continue
            d, s, on = _run(L, depth, geo, kind, m, early, seed)
        db += d; sao += s
        print("filter columns %dx%d depth %d: deblocking changed %d samples, SAO %d, SAO on in %d of %d CTUs" % (geo[0], geo[1], depth, d, s, on, _case(depth, geo)[0]["nctu"]))
        assert on > 0, (geo, "the decision switched SAO off everywhere: the case tests nothing")
    assert db > 5000 and sao > 1000, (db, sao)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", CONTRACT_GEOMETRIES, ids=lambda g: "%dx%d" % g[:2])
def test_filter_columns_contract_one_row_or_column(geo):
    """pictures of one CTU row or one CTU column: not the encoder's case (it filters those row by row), but nothing in include/x265amd.h excludes them"""
    L = T.load_hip(8)
    _run(L, 8, geo, "wavefront", 1, 1, 31)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_filter_columns_1080p(depth):
    """1920x1080 under one wavefront schedule with a P picture's chunk minima; what is published is checked every tenth sweep"""
    L = T.load_hip(depth)
    geo = (1920, 1080, False, False, 40 + depth)
    d, s, on = _run(L, depth, geo, "wavefront", 2, 1, 41, every=10, max_step=8)
    assert d > 5000 and s > 1000 and on > 0, (d, s, on)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_extend_border_band_equals_oracle(depth):
    """x265amd_extend_border_band (one plane): band after band, column range after column range over poisoned margins gives the oracle's extend_pic_border; after
    every call the margins of what is finished so far are final.  Odd widths and margins included (130x70)."""
    import torch
    L, O = T.load_hip(depth), T.load_oracle(depth)
    rng = np.random.default_rng(5)
    tdt = torch.uint8 if depth == 8 else torch.int16
    for c in T.plane_cases(depth, 12):
        w, h, mx, my, st = c["w"], c["h"], c["mx"], c["my"], c["stride"]
        buf = c["buf"].reshape(h + 2 * my, st).copy()
        poison = np.full_like(buf, 0xA5 if depth == 8 else 0x2A5)
        poison[my:my + h, mx:mx + w] = buf[my:my + h, mx:mx + w]
        want = poison.copy()
        O.lib.orc_extend_pic_border(T.off(want.reshape(-1), c["org"]), C.c_int64(st), w, h, mx, my)
        d_want = torch.from_numpy(want.view(np.uint8).copy()).cuda().view(tdt)
        d = torch.from_numpy(poison.view(np.uint8).copy()).cuda().view(tdt)
        cuts = sorted({0, w} | {int(x) for x in rng.integers(1, w, 3)})
        for y0 in range(0, h, 64):
            y1 = min(h, y0 + 64)
            for x0, x1 in zip(cuts, cuts[1:]):
                assert L.lib.x265amd_extend_border_band(None, C.c_void_p(d.data_ptr() + c["org"] * buf.itemsize), C.c_int64(st), w, h, mx, my, y0, y1, x0, x1, int(x0 == 0), int(x1 == w)) == 0
                torch.cuda.synchronize()
                ys = slice(0 if y0 == 0 else my + y0, h + 2 * my if y1 == h else my + y1)
                xs = slice(0, st if x1 == w else mx + x1)
                assert torch.equal(d[ys, xs], d_want[ys, xs]), (w, h, mx, my, y0, y1, x0, x1)
        got = d.cpu().numpy().view(np.uint8).view(buf.dtype).reshape(buf.shape)
        assert np.array_equal(got, want), (w, h, mx, my, _first_diff(got, want, dict(margin=(mx, my)), 0))
