"""The lookahead kernels beside their plainest form (csrc/lowres_kernels.hip): x265amd_lowres_frame_cost_batch in cooperative slices, with weighted search planes, with motion
fields that are read instead of searched, all of them mixed in one launch; x265amd_weight_buffer; x265amd_lowres_weight_costs / _many and x265amd_chroma_weight_costs with
motion vectors.  The estimates are compared with tests/golden/lowres_paths_golden.npz, which tests/golden/make_lowres_paths_golden.py made from the reference's own
estimateCUCost (oracle/refprims.cpp: ref_lowres_frame_cost_paths); the weight costs with the reference's mcLuma / mcChroma / weightCost written out from the oracle's pieces
(hevc_testlib.weight_cost_luma_expected, chroma_weight_cost_expected).  Everything is integer arithmetic and compared bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import hevc_testlib as T

SPECS = T.lowres_paths_specs()
COST_GOLD = os.path.join(T.GOLDEN_DIR, "lowres_cost_golden.npz")
# tests/test_lowres.py's COST_CASES that are scenes of this file: (golden index, entry here)
SAME_AS_COST_GOLDEN = [(2, "s8/B/u"), (4, "s10/P/u")]


def gold():
    return np.load(T.PATHS_GOLD)


def entry(g, name):
    return T.lowres_paths_golden_entry(g, name)


def geometry(scene):
    """(wcu, hcu) of a scene without building it"""
    depth, seed, crop, fade = T.PATHS_SCENES[scene]
    return ((T.MC_W - crop[0]) // 2 + 7) >> 3, ((T.MC_H - crop[1]) // 2 + 7) >> 3


def differing_blocks(a, b, nlists):
    """blocks whose vector differs in one of the lists"""
    return np.flatnonzero((a["mvs"][:nlists] != b["mvs"][:nlists]).any(axis=(0, 2)))


def check_golden_conditions(g):
    """what keeps the GPU tests from being vacuous, on the golden's arrays (a mapping name -> array)"""
    used_reuse = np.zeros(4, np.int64)
    for name, spec in SPECS.items():
        e = entry(g, name)
        wcu, hcu = geometry(spec["scene"])
        nlists = 1 + (spec["kind"] == "B")
        rps, ns = spec["slices"]
        plain = spec["search"] == (1, int(spec["kind"] == "B")) and not spec["weight"]
        if plain and ns:
            u = entry(g, "%s/%s/u" % (spec["scene"], spec["kind"]))
            if ns == 1:         # one slice is no slices
                for k in e:
                    assert np.array_equal(e[k], u[k]), (name, k)
            else:
                d = differing_blocks(e, u, nlists)
                bottom_first = T.lowres_slice_rows(hcu, spec["slices"])[-1][0]
                assert len(d) >= 5, (name, len(d))
                assert (d // wcu < bottom_first).all(), (name, "a vector of the bottom slice differs", d.tolist())     # the bottom slice is the unsliced chain's start
        if spec["weight"] and spec["kind"] == "B":
            assert int(((e["lowres_costs"] >> 14) == 3).sum()) >= 20, (name, "bi-prediction wins in too few blocks")
        if spec["src"] or name in ("s8/P/u", "s10/P/u"):
            used_reuse += np.bincount(e["lowres_costs"] >> 14, minlength=4)
        if name.endswith("/B/measure"):
            m = entry(g, spec["src"])
            for k in e:
                assert np.array_equal(e[k], m[k]), (name, k, "measuring again changes the estimate")
    for f in ("f8", "f10"):
        w, u = entry(g, f + "/P/w"), entry(g, f + "/P/u")
        changed = (w["mvs"][0] != u["mvs"][0]).any(1) | (w["mv_costs"][0] != u["mv_costs"][0]) | (w["lowres_costs"] != u["lowres_costs"])
        assert changed.mean() >= 0.10, (f, float(changed.mean()))
    assert (used_reuse > 20).all(), used_reuse        # intra, L0, L1, bi


def test_paths_golden_conditions():
    g = gold()
    assert sorted(k.rsplit("/", 1)[0] for k in g.files if k.endswith("/lowres_costs")) == sorted(SPECS)
    check_golden_conditions(g)


def test_paths_golden_repeats_the_plain_golden():
    """the recipe of this golden (estimateCUCost looped here) against the recipe of lowres_cost_golden.npz (estimateFrameCost itself) where the two cover the same estimate"""
    g, old = gold(), np.load(COST_GOLD)
    for k, name in SAME_AS_COST_GOLDEN:
        e = entry(g, name)
        nlists = 1 + (SPECS[name]["kind"] == "B")
        assert np.array_equal(e["lowres_costs"], old["%d/lowres_costs" % k]) and np.array_equal(e["row_satds"], old["%d/row_satds" % k]), name
        assert np.array_equal(e["mvs"][:nlists], old["%d/mvs" % k][:nlists]) and np.array_equal(e["mv_costs"][:nlists], old["%d/mv_costs" % k][:nlists]), name
        assert np.array_equal(g[SPECS[name]["scene"] + "/intra_cost"], old["%d/intra_cost" % k]), name
        assert int(e["slice_sums"][0, 1]) == int(old["%d/sums" % k][2]), name            # intraMbs
        if nlists == 1:
            assert int(e["slice_sums"][0, 0]) == int(old["%d/sums" % k][0]), name        # a P estimate's score is its costEst


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref not built (needs /root/reference)")
def test_paths_golden_vs_ref():
    g = gold()
    out = T.lowres_paths_compute_ref()
    assert sorted(out) == sorted(g.files)
    for k in out:
        assert out[k].dtype == g[k].dtype and np.array_equal(out[k], g[k]), k


# ---- the weight-cost fixtures (f, g) ----
LUMA_WC_SIZES = [(128, 96), (120, 92)]          # 16 x 12 blocks; 15 x 12 blocks with a last block row that is half inside the picture
# chroma plane (width, height), lowres grid (blocks): the grid of the picture the plane belongs to (4:2:0: the plane's own size / 8), and a larger one that puts more
# blocks inside mcChroma's condition
CHROMA_WC_CASES = [((64, 48), (8, 6)), ((120, 72), (15, 9)), ((64, 48), (40, 40))]


def test_weight_cost_fixtures_are_not_vacuous():
    for (w, h) in LUMA_WC_SIZES:
        mv = T.weight_cost_luma_mvs(500 + w, w, h)
        bw = w >> 3
        clipped = [tuple(mv[i]) != T.mv_clip_luma(mv[i], (i % bw) * 8, (i // bw) * 8, w, h) for i in range(len(mv))]
        after = [T.mv_clip_luma(mv[i], (i % bw) * 8, (i // bw) * 8, w, h) for i in range(len(mv))]
        assert np.mean(clipped) >= 0.25, np.mean(clipped)
        assert len({(x & 3, y & 3) for (x, y) in after}) == 16 and (0, 0) in after
        low, high = np.array(after).min(0), np.array(after).max(0)
        assert low[0] < -32 and low[1] < -32 and high[0] > 32 and high[1] > 32         # clipped at all four sides
        right, bottom = [i for i in range(len(mv)) if i % bw == bw - 1], [i for i in range(len(mv)) if i // bw == len(mv) // bw - 1]
        assert any(clipped[i] for i in right) and any(clipped[i] for i in bottom) and not all(clipped[i] for i in right) and not all(clipped[i] for i in bottom)
    for (w, h), (lw, lh) in CHROMA_WC_CASES:
        inside = [T.chroma_weight_inside(x, y, lw, lh) for y in range(0, h, 8) for x in range(0, w, 8)]
        assert any(inside) and not all(inside)
    (w, h), (lw, lh) = CHROMA_WC_CASES[2]
    mv = T.chroma_weight_mvs(900, w, h, lw)
    kinds = set()
    for y in range(0, h, 8):
        for bx in range(w >> 3):
            if T.chroma_weight_inside(bx * 8, y, lw, lh):
                mx, my = mv[y * lw + bx]
                mx = min(max(int(mx), (-bx * 8 - 8) * 4), (w - bx * 8 - 1 + 8) * 4); my = min(max(int(my), (-y - 8) * 4), (h - y - 1 + 8) * 4)
                kinds.add((bool(mx & 7), bool(my & 7)))
    assert len(kinds) == 4, kinds          # copy, horizontal, vertical and both filters


# ---- GPU ----
def device_scene(depth, scene):
    L = T.load_hip(depth)
    return T.LowresPathsDev(L, T.HipME(depth), T.lowres_paths_scene(scene))


def job_of(name, src=None, dev=None):
    s = SPECS[name]
    return dict(kind=s["kind"], slices=s["slices"], search=s["search"], weight=s["weight"], src=src, dev=dev, name=name)


def assert_fields_untouched(job, got):
    """a list that is read (do_search 0) leaves its field and MV costs byte for byte as they were handed in"""
    for l in range(1 + (job["kind"] == "B")):
        if not job["search"][l]:
            assert got["mvs"][l].tobytes() == job["src"]["mvs"][l].tobytes() and got["mv_costs"][l].tobytes() == job["src"]["mv_costs"][l].tobytes(), (job["name"], l)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["s8", "c8", "s10", "c10"])
def test_hip_sliced_estimates_match_reference(scene):
    """a: P and B estimates in every slice layout the reference can form on 12 and 10 block rows (and unsliced, and as one slice), one launch per scene"""
    g = gold()
    dev = device_scene(T.PATHS_SCENES[scene][0], scene)
    names = [n for n, s in SPECS.items() if s["scene"] == scene and not s["src"]]
    assert len(names) == 2 * (1 + len(T.PATHS_LAYOUTS[dev.c["hcu"]]))
    jobs = [job_of(n) for n in names]
    for job, got in zip(jobs, dev.run(jobs)):
        T.lowres_paths_assert(dev.c, job, got, entry(g, job["name"]), job["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_weight_buffer_matches_oracle(depth):
    """b: x265amd_weight_buffer against weight_pp_c (oracle) over the whole four-plane padded buffer of a scene, and over a buffer whose length is no multiple of the
    workgroup, full of the smallest and largest samples: denominators 0 and 7, negative offsets, the clip at both ends; nothing is written past the count"""
    import torch
    L, O = T.load_hip(depth), T.load_oracle(depth)
    dev = device_scene(depth, "c%d" % depth)
    dt = dev.dt
    pmax = (1 << depth) - 1
    rng = np.random.default_rng(3100 + depth)
    odd = rng.integers(0, pmax + 1, 100003).astype(dt)
    odd[rng.integers(0, odd.size, 20000)] = pmax
    odd[rng.integers(0, odd.size, 20000)] = 0
    assert odd.size % 256 and (odd == pmax).sum() > 1000
    for src in (dev.host_planes(dev.buf[0]).reshape(-1), odd):
        d_src = torch.from_numpy(src.view(np.uint8).copy()).cuda()
        for (scale, denom, off) in ((90, 7, 10), (2, 0, -5), (1, 0, 0), (127, 7, -128), (37, 5, 127), (64, 6, -1), (127, 0, 3)):
            cand = T.weight_cand(depth, scale, denom, off)
            want = np.zeros_like(src)
            O.lib.orc_weight_pp(T._ptr(src), T._ptr(want), C.c_int64(src.size), src.size, 1, cand[1], cand[2], cand[3], cand[4])
            guard = 64
            d_dst = torch.full(((src.size + guard) * dt.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
            assert L.lib.x265amd_weight_buffer(None, C.c_void_p(d_src.data_ptr()), C.c_void_p(d_dst.data_ptr()), C.c_size_t(src.size), cand[1], cand[2], cand[3], cand[4]) == 0
            torch.cuda.synchronize()
            got = d_dst.cpu().numpy()
            assert (got[src.size * dt.itemsize:] == 0xA5).all(), (scale, denom, off)
            got = got[:src.size * dt.itemsize].view(dt)
            assert np.array_equal(got, want), ((scale, denom, off), np.flatnonzero(got != want)[:6].tolist())
            if scale * pmax >> denom > pmax:
                assert (want == pmax).any()        # the upper clip acted
            if off < 0:
                assert (want == 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_weighted_estimates_match_reference(depth):
    """c: list 0 searched on the planes x265amd_weight_buffer made, P and B, unsliced and sliced.  In the B estimates bi-prediction wins in many blocks (checked on the golden):
    they are the reference's only if the bidirectional and the co-located average read the UNWEIGHTED planes"""
    g = gold()
    scene = "f%d" % depth
    dev = device_scene(depth, scene)
    names = [n for n, s in SPECS.items() if s["scene"] == scene and not s["src"]]
    assert len(names) == 5
    jobs = [job_of(n) for n in names]
    for job, got in zip(jobs, dev.run(jobs)):
        T.lowres_paths_assert(dev.c, job, got, entry(g, job["name"]), job["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_reused_fields_match_reference(depth):
    """d: a searched P estimate; a B estimate that READS that list-0 field and searches list 1; the same B estimate again with both fields read (it only measures) -- each the
    reference's in the same order, the last equal to the one before it, every field that is only read untouched; the mixed form again in slices; and as a fade runs it: the
    P estimate searched on weighted planes, the B estimate reads its field and has no weight (a search of list 0 there would find other vectors: the golden's P fields with and
    without the weight differ in a tenth of the blocks at least)"""
    g = gold()
    s = "s%d" % depth
    dev = device_scene(depth, s)
    lay = "%dx%d" % ((4, 3) if depth == 8 else (5, 2))
    f = "f%d" % depth
    for p_name, mixed_name, measure_name in ((s + "/P/u", s + "/B/mixed", s + "/B/measure"), ("%s/P/%s" % (s, lay), "%s/B/mixed%s" % (s, lay), None), (f + "/P/w", f + "/B/reuse", None)):
        if p_name.startswith(f):
            dev = device_scene(depth, f)
        assert SPECS[mixed_name]["src"] == p_name and SPECS[mixed_name]["search"] == (0, 1)
        job = job_of(p_name)
        p = dev.run([job])[0]
        T.lowres_paths_assert(dev.c, job, p, entry(g, p_name), p_name)
        job = job_of(mixed_name, src=p)
        mixed = dev.run([job])[0]
        T.lowres_paths_assert(dev.c, job, mixed, entry(g, mixed_name), mixed_name)
        assert_fields_untouched(job, mixed)
        if measure_name:
            assert SPECS[measure_name]["src"] == mixed_name and SPECS[measure_name]["search"] == (0, 0)
            job = job_of(measure_name, src=mixed)
            again = dev.run([job])[0]
            T.lowres_paths_assert(dev.c, job, again, entry(g, measure_name), measure_name)
            assert_fields_untouched(job, again)
            assert np.array_equal(again["lowres_costs"], mixed["lowres_costs"]) and np.array_equal(again["bcost"], mixed["bcost"])


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_mixed_batch_keeps_every_jobs_parameters(depth):
    """e: sliced, unsliced, weighted, reusing and measuring estimates of two scenes of one size in ONE launch, each with buffers of its own that start filled with a pattern:
    a parameter of one job applied to another (k_lowres_cost_batch copies its record per workgroup) shows in some estimate"""
    g = gold()
    s, f = "s%d" % depth, "f%d" % depth
    lay = "%dx%d" % ((4, 3) if depth == 8 else (5, 2))
    ds, df = device_scene(depth, s), device_scene(depth, f)
    assert (ds.c["wcu"], ds.c["hcu"], ds.lstride) == (df.c["wcu"], df.c["hcu"], df.lstride)
    names = [s + "/B/6x2", f + "/P/w", s + "/P/u", "%s/B/mixed%s" % (s, lay), s + "/B/u", "%s/B/w%s" % (f, lay), s + "/B/measure", s + "/P/4x3", f + "/P/u",
             s + "/B/mixed", f + "/B/w", s + "/P/12x1", f + "/B/reuse", s + "/B/5x2", "%s/P/w%s" % (f, lay)]
    jobs = [job_of(n, src=entry(g, SPECS[n]["src"]) if SPECS[n]["src"] else None, dev=df if SPECS[n]["scene"] == f else ds) for n in names]
    for job, got in zip(jobs, ds.run(jobs)):
        T.lowres_paths_assert(ds.c, job, got, entry(g, job["name"]), job["name"])
        assert_fields_untouched(job, got)


def _upload(a):
    import torch
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


CAND_DT = np.dtype([("present", "<i4"), ("w0", "<i4"), ("round", "<i4"), ("shift", "<i4"), ("offset", "<i4")])
WC_JOB_DT = np.dtype([("d_fenc", "<u8"), ("d_ref", "<u8", 4), ("d_mvs", "<u8"), ("d_intra_cost", "<u8"), ("cands", CAND_DT, 2)])


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_lowres_weight_costs_with_vectors(depth):
    """f: x265amd_lowres_weight_costs and _many with a motion field over all four planes -- every quarter-sample phase, vectors clipped at all four sides, the right column and
    the bottom row, a height that is no multiple of 8 --, with and without intra costs, unweighted and weighted candidates, against mcLuma + weightCost written out"""
    L, O = T.load_hip(depth), T.load_oracle(depth)
    assert WC_JOB_DT.itemsize == 96
    M = T.WEIGHT_MARGIN
    jobs, want_many, keep = [], [], []
    for (w, h) in LUMA_WC_SIZES:
        fenc, refs, stride = T.weight_cost_planes(depth, 7800 + depth + w, w, h, 4)
        mvs = T.weight_cost_luma_mvs(500 + w, w, h)
        nblk = (w >> 3) * ((h + 7) >> 3)
        intra = np.random.default_rng(w).integers(0, 5000 << (depth - 8), nblk).astype(np.int32)
        cands = [(0, 0, 0, 0, 0), T.weight_cand(depth, 90, 7, 10), T.weight_cand(depth, 45, 6, -12)]
        isz = fenc.itemsize
        d_f, d_r, d_mv, d_i = _upload(fenc), [_upload(r) for r in refs], _upload(mvs), _upload(intra)
        keep += [d_f, d_r, d_mv, d_i]
        o = (M * stride + M) * isz
        refs_p = (C.c_void_p * 4)(*[r.data_ptr() + o for r in d_r])
        for use_mv in (True, False):
            for use_intra in (True, False):
                want = [T.weight_cost_luma_expected(O, depth, fenc, refs, stride, w, h, mvs if use_mv else None, intra if use_intra else None, c) for c in cands]
                if use_mv:
                    assert len(set(want)) == len(want) and want != [T.weight_cost_luma_expected(O, depth, fenc, refs, stride, w, h, None, intra if use_intra else None, c) for c in cands]
                ca = np.array(cands, CAND_DT); costs = np.zeros(len(cands), np.uint32)
                assert L.lib.x265amd_lowres_weight_costs(None, C.c_void_p(d_f.data_ptr() + o), refs_p, C.c_void_p(d_mv.data_ptr()) if use_mv else None,
                                                         C.c_void_p(d_i.data_ptr()) if use_intra else None, C.c_int64(stride), w, h, ca.ctypes.data_as(C.c_void_p), len(cands),
                                                         costs.ctypes.data_as(C.c_void_p)) == 0, L.lib.x265amd_last_error()
                assert [int(v) for v in costs] == want, ((w, h), use_mv, use_intra, costs.tolist(), want)
                if (w, h) == LUMA_WC_SIZES[1]:      # the many-decisions form takes one size per call
                    jobs.append((d_f.data_ptr() + o, [r.data_ptr() + o for r in d_r], d_mv.data_ptr() if use_mv else 0, d_i.data_ptr() if use_intra else 0, cands[:2] if use_intra else cands[1:]))
                    want_many += want[:2] if use_intra else want[1:]
    w, h = LUMA_WC_SIZES[1]
    rec = np.zeros(len(jobs), WC_JOB_DT)
    for i, (pf, pr, pm, pi, c2) in enumerate(jobs):
        rec[i]["d_fenc"], rec[i]["d_ref"], rec[i]["d_mvs"], rec[i]["d_intra_cost"], rec[i]["cands"] = pf, pr, pm, pi, np.array(c2, CAND_DT)
    costs = np.zeros(2 * len(jobs), np.uint32)
    assert L.lib.x265amd_lowres_weight_costs_many(None, rec.ctypes.data_as(C.c_void_p), len(jobs), C.c_int64(stride), w, h, costs.ctypes.data_as(C.c_void_p)) == 0, L.lib.x265amd_last_error()
    assert [int(v) for v in costs] == want_many


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_hip_chroma_weight_costs_with_vectors(depth):
    """g: x265amd_chroma_weight_costs against mcChroma + weightCost's chroma branch written out: the vector of (the block's first sample row, the block's column), used only where
    the block's sample position lies inside the lowres grid, a quarter for the position and an eighth for the fraction, the oracle's chroma interpolation; with a field and
    without, unweighted and weighted candidates"""
    L, O = T.load_hip(depth), T.load_oracle(depth)
    M = T.WEIGHT_MARGIN
    for k, ((w, h), (lw, lh)) in enumerate(CHROMA_WC_CASES):
        fenc, (ref,), stride = T.weight_cost_planes(depth, 8800 + depth + k, w, h, 1)
        mvs = T.chroma_weight_mvs(900, w, h, lw)
        cands = [(0, 0, 0, 0, 0), T.weight_cand(depth, 90, 7, 10), T.weight_cand(depth, 33, 5, -9)]
        d_f, d_r, d_mv = _upload(fenc), _upload(ref), _upload(mvs)
        o = (M * stride + M) * fenc.itemsize
        for use_mv in (True, False):
            want = [T.chroma_weight_cost_expected(O, depth, fenc, ref, stride, w, h, mvs if use_mv else None, lw, lh, c) for c in cands]
            if use_mv:
                assert want != [T.chroma_weight_cost_expected(O, depth, fenc, ref, stride, w, h, None, lw, lh, c) for c in cands]
            ca = np.array(cands, CAND_DT); costs = np.zeros(len(cands), np.uint32)
            assert L.lib.x265amd_chroma_weight_costs(None, C.c_void_p(d_f.data_ptr() + o), C.c_void_p(d_r.data_ptr() + o), C.c_void_p(d_mv.data_ptr()) if use_mv else None,
                                                     C.c_int64(stride), w, h, lw, lh, ca.ctypes.data_as(C.c_void_p), len(cands), costs.ctypes.data_as(C.c_void_p)) == 0, \
                L.lib.x265amd_last_error()
            assert [int(v) for v in costs] == want, ((w, h), (lw, lh), use_mv, costs.tolist(), want)
