"""The job server's command bodies (csrc/device_queue.hip: xa_op_*), operation by operation, against the oracle.

This file is where the QUEUE transport of the block operations is pinned.  The kernel-level tests of the same operations (test_tu_golden, test_mc_golden,
test_intra_golden, test_inter_cost, test_intra_tu, test_hip_entropy, test_hip_me, test_inter_rd) launch kernels on the NULL stream; the encoder runs none of them
that way: every CTU row holds a device job queue and the resident k_job_server runs the operations as commands, dealing the jobs out over its workgroup by
rules of its own and, for some, through device functions no launched kernel calls (block_tu_chain_job, block_me_search_multi, the split-PU form of
wave_mc_job, LDS regions carved from xa_smem).  Each test here sends one operation through a held queue (hevc_testlib.held_queue: read its rules) with job
counts on either side of every split of its command body, compares every job with the oracle runner the launched test uses, and proves from
x265amd_queue_stats that the server ran the command.  (test_inter_rd, test_intra_rd, test_inter_search and test_intra_cu_bits reach a queue only under
X265AMD_TEST_QUEUE=1 and stay as they are.)"""
import numpy as np
import pytest

import hevc_testlib as T
from test_inter_rd import CASES as RD_CASES, GOLD_PATH as RD_GOLD_PATH, check_golden as rd_check_golden

pytestmark = pytest.mark.gpu


class server_ran:
    """around one runner call on a held queue: the job server's counters (valid only while no queue is held) are reset before and read after, and the command
    kinds in `want` have risen by exactly the number of commands the test sent"""

    def __init__(self, hip, what, **want):
        self.hip, self.what, self.want = hip, what, want
        self.bytes = {}

    def __enter__(self):
        T.queue_stats(self.hip, reset=1)
        return T.held_queue(self.hip)

    def __exit__(self, *exc):
        if exc[0] is None:
            got = T.queue_stats(self.hip)
            for op, k in self.want.items():
                assert got[op] == k, "%s: the job server ran %d %s commands, not %d (%s)" % (self.what, got[op], op, k, {o: v for o, v in got.items() if v})
            print("queue_stats %s: %s" % (self.what, {o: v for o, v in got.items() if v and o not in ("NOP", "EXIT")}))
            self.bytes = T.queue_stats(self.hip, algorithmic_bytes=True)
        return False


# ---- XA_OP_TU_CHAIN: n <= 4 * XA_SERVER_WAVES (32): units of 16x16 and 32x32 by the whole workgroup (block_tu_chain_job), the rest round-robin by a running
# counter that must skip them; above 32 every unit on a wavefront ----
def tu_compositions(depth):
    pool = T.tu_cases(depth, 4100, 400)
    large = [c for c in pool if c["log2"] >= 4]
    small = [c for c in pool if c["log2"] <= 3]
    assert {c["log2"] for c in large[:17]} == {4, 5} and {c["log2"] for c in small[:17]} == {2, 3}
    mixed, li, si = [], 0, 0
    for k in range(33):         # large and small interleaved irregularly: L S S L S L L S ...
        if "LSSLSLLS"[k % 8] == "L":
            mixed.append(large[li]); li += 1
        else:
            mixed.append(small[si]); si += 1
    return [("one 32x32", [c for c in pool if c["log2"] == 5][:1]), ("8 large", large[20:28]), ("32 mixed", mixed[:32]), ("33 mixed", mixed), ("32 small", small[20:52])]


@pytest.mark.parametrize("depth", [8, 10])
def test_tu_chain(depth):
    hip, orc = T.load_hip(depth), T.load_oracle(depth)
    for name, cases in tu_compositions(depth):
        what = "TU_CHAIN, %s (%d jobs, log2 %s)" % (name, len(cases), "".join(str(c["log2"]) for c in cases))
        ran = server_ran(hip, what, TU_CHAIN=1)
        with ran as q:
            got = T.tu_chain_run_hip(hip, cases, depth, stream=q)
        T.tu_chain_assert(got, T.tu_run_chain_oracle(orc, cases), cases, what)
        # every unit once: a unit taken by the workgroup AND by a wavefront gives the same samples twice, and only the byte count tells.  Both bodies count
        # (3 sizeof(pixel) + 4) N^2 per unit (tu_dev.h: block_tu_chain_job, wave_tu_chain_job)
        once = sum((3 * np.dtype(hip.pixel).itemsize + 4) << (2 * c["log2"]) for c in cases)
        assert ran.bytes["TU_CHAIN"] == once, "%s: the units' bytes add up to %d, the server counted %d: a unit ran twice or not at all" % (what, once, ran.bytes["TU_CHAIN"])


# ---- XA_OP_TU_CHAIN_RDOQ: W = XA_SERVER_LDS / (sizeof(TuLds) + sizeof(RdoqLds)) wavefronts, each with its own regions of xa_smem.  sizeof(TuLds) = 12288 + 1024
# samples (13312 / 14336 bytes at 8 / 10 bits), sizeof(RdoqLds) = 25824: W = 147456 / 39136 = 147456 / 40160 = 3 at both depths; the counts lie below, at,
# and above any W from 1 to 8 ----
@pytest.mark.parametrize("depth", [8, 10])
def test_tu_chain_rdoq(depth):
    hip, orc = T.load_hip(depth), T.load_oracle(depth)
    pool = T.rdoq_cases(depth, 4200, 53)
    at = 0
    for n in (1, 3, 9, 40):
        cases = pool[at:at + n]; at += n
        what = "TU_CHAIN_RDOQ, %d jobs" % n
        with server_ran(hip, what, TU_CHAIN_RDOQ=1) as q:
            got = T.tu_chain_rdoq_run_hip(hip, cases, stream=q)
        T.tu_chain_assert(got, T.rdoq_chain_oracle(orc, cases), cases, what)


# ---- XA_OP_INTRA_TU_CHAIN (8 wavefronts) and XA_OP_INTRA_TU_CHAIN_RDOQ (W = 147456 / (sizeof(TuLds) + sizeof(IntraTuLds) + sizeof(RdoqLds)) = 147456 / 40568
# at 8 bits, / 43024 at 10 bits = 3 wavefronts) ----
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("rdoq", [False, True])
def test_intra_tu_chain(depth, rdoq):
    hip, orc = T.load_hip(depth), T.load_oracle(depth)
    pool = T.intra_tu_cases(depth, 4300 + int(rdoq), 60, rdoq=rdoq)
    if rdoq:        # the one-job command must be an RDOQ job (a batch without any goes to the plain command)
        first = next(i for i, c in enumerate(pool) if c["rdoq"])
        pool[0], pool[first] = pool[first], pool[0]
    at = 0
    op = "INTRA_TU_CHAIN_RDOQ" if rdoq else "INTRA_TU_CHAIN"
    for n in (1, 9, 40):
        cases = pool[at:at + n]; at += n
        assert not rdoq or any(c["rdoq"] for c in cases)
        what = "%s, %d jobs" % (op, n)
        with server_ran(hip, what, **{op: 1}) as q:
            got = T.intra_tu_run_hip(hip, cases, stream=q)
        want = T.intra_tu_run_host(orc, cases)
        for i, (c, g, w) in enumerate(zip(cases, got, want)):
            tag = "%s: job %d (%dx%d, plane %d, mode %d, rdoq %d)" % (what, i, 1 << c["log2"], 1 << c["log2"], c["ttype"], c["mode"], c["rdoq"])
            assert g[0] == w[0], "%s: (numSig, dist0, energy0, dist, energy) %s, want %s" % (tag, g[0], w[0])
            for k, name in ((1, "prediction"), (2, "reconstruction"), (3, "levels"), (4, "residual")):
                assert np.array_equal(g[k], w[k]), "%s: %s" % (tag, name)


# ---- XA_OP_INTRA_SCAN: n <= 16 the whole workgroup on each block in turn (block_intra_scan_job), above a wavefront per block ----
@pytest.mark.parametrize("depth", [8, 10])
def test_intra_scan(depth):
    hip, orc = T.load_hip(depth), T.load_oracle(depth)
    pool = T.intra_cases(depth, 4400, 160)
    by_size = {l: [c for c in pool if c["log2"] == l] for l in (2, 3, 4, 5)}
    batches = [[by_size[l][0]] for l in (2, 3, 4, 5)]           # one job: once per block size
    at = 1
    for n in (16, 17, 40):
        per = (n + 3) // 4
        batches.append([by_size[2 + (k % 4)][at + k // 4] for k in range(n)])
        at += per
    for cases in batches:
        assert len(cases) == 1 or {c["log2"] for c in cases} == {2, 3, 4, 5}
        what = "INTRA_SCAN, %d jobs (log2 %s)" % (len(cases), "".join(str(c["log2"]) for c in cases))
        with server_ran(hip, what, INTRA_SCAN=1) as q:
            got = T.intra_run_hip(hip, cases, stream=q)
        want = T.intra_run_host(orc, cases)
        for i, (c, g, w) in enumerate(zip(cases, got, want)):
            tag = "%s: job %d (%dx%d)" % (what, i, 1 << c["log2"], 1 << c["log2"])
            assert np.array_equal(g[0], w[0]), tag + ": neighbours"
            assert (g[1] is None) == (w[1] is None) and (g[1] is None or np.array_equal(g[1], w[1])), tag + ": filtered neighbours"
            assert np.array_equal(g[2], w[2]), "%s: sa8d of the 35 modes %s, want %s" % (tag, g[2], w[2])


# ---- XA_OP_MC: below 8 jobs 8 / n wavefronts share a PU (wave_mc_job<false>(a, ji, sub * 64 + lane, wpj * 64)), then rounds of perRound jobs ----
def mc_batches():
    pool = T.mc_jobs(4500, 3000)
    special = lambda j: j["ref0"] >= 0 and j["ref1"] >= 0 and (j["flags"] & 4)        # bi-predicted and weighted
    def of_sizes(sizes):
        sel = [j for j in pool if (int(j["w"]), int(j["h"])) in sizes and (j["flags"] & 3) == 3]
        a, b = [j for j in sel if special(j)], [j for j in sel if not special(j)]
        assert len(a) >= 6 and len(b) >= 6
        out = []
        for x, y in zip(a, b):      # special and ordinary jobs in turn, a special one first
            out += [x, y]
        return out
    big, tiny = of_sizes({(64, 64)}), of_sizes({(8, 4), (4, 8)})
    batches = []
    at = 0
    for n in (1, 2, 3, 5):
        batches.append(("%d PUs of 64x64" % n, np.array(big[at:at + n], T.MC_JOB_DT)))
        batches.append(("%d PUs of 8x4 / 4x8" % n, np.array(tiny[at:at + n], T.MC_JOB_DT)))
        at += n
    at = 0
    for n in (8, 9, 40):
        batches.append(("%d PUs of all sizes" % n, pool[at:at + n].copy())); at += n
    return batches


def mc_assert(got, want, jobs, what):
    for i, (g, w) in enumerate(zip(got, want)):
        j = jobs[i]
        tag = "%s: job %d (%dx%d at %d,%d, refs %d %d, mv %s %s, flags %d)" % (what, i, j["w"], j["h"], j["x"], j["y"], j["ref0"], j["ref1"], j["mv0"], j["mv1"], j["flags"])
        for p, name in enumerate("YUV"):
            assert (g[p] is None) == (w[p] is None), tag
            assert g[p] is None or np.array_equal(g[p], w[p]), "%s: plane %s" % (tag, name)


@pytest.mark.parametrize("depth", [8, 10])
def test_mc(depth):
    hip, orc = T.load_hip(depth), T.load_oracle(depth)
    pics, stride, cstride, org = T.mc_make_refs(depth, 4500)
    seen_bi = seen_w = 0
    for name, jobs in mc_batches():
        what = "MC, %s" % name
        seen_bi += int(((jobs["ref0"] >= 0) & (jobs["ref1"] >= 0)).sum()); seen_w += int(((jobs["flags"] & 4) != 0).sum())
        with server_ran(hip, what, MC=1) as q:
            got = T.mc_run_hip(hip, pics, stride, cstride, org, jobs, stream=q)
        mc_assert(got, T.mc_run_host(orc, pics, stride, cstride, org, jobs), jobs, what)
    assert seen_bi > 10 and seen_w > 10


# ---- XA_OP_MC_COST: a wavefront per job, stride 8 ----
@pytest.mark.parametrize("depth", [8, 10])
def test_mc_cost(depth):
    hip, orc = T.load_hip(depth), T.load_oracle(depth)
    pics, stride, cstride, org = T.mc_make_refs(depth, 4600, nref=4)
    pics, fenc = pics[:3], pics[3]
    pool = T.inter_cost_jobs(4600, 58)
    at = 0
    for n in (1, 8, 9, 40):
        jobs = pool[at:at + n].copy(); at += n
        what = "MC_COST, %d jobs" % n
        with server_ran(hip, what, MC_COST=1) as q:
            cost, pred = T.inter_cost_run_hip(hip, pics, fenc, stride, cstride, org, jobs, stream=q)
        wcost, wpred = T.inter_cost_run_host(orc, pics, fenc, stride, cstride, org, jobs)
        for i in range(n):
            j = jobs[i]
            tag = "%s: job %d (%dx%d, metric %d, chroma %d)" % (what, i, j["w"], j["h"], j["metric"], j["chroma_cost"])
            assert np.array_equal(cost[i], wcost[i]), "%s: costs %s, want %s" % (tag, cost[i], wcost[i])
            assert np.array_equal(pred[i], wpred[i]), tag + ": luma prediction"


# ---- XA_OP_ME_SEARCH / _STAR: 2 to 8 groups of one job each that fit the LDS side by side (block_me_search_multi), otherwise the groups one after the other ----
ME_WIN = (128, 128)     # three regions of (128 * 128 + 16 + 64 * 64) samples fit XA_SERVER_LDS at 10 bits too (me_multi_fits)


def me_scene(depth):
    cur, ref, stride, origin = T.me_make_planes(depth, 46, motion=(5, -3))
    rng = np.random.default_rng(46)
    pmax = (1 << depth) - 1
    refs = [ref]
    for shift in ((2, -3), (-4, 1)):        # two more reference pictures: the first displaced, with noise of their own
        r = np.roll(ref.reshape(-1, stride), shift, (0, 1)).astype(np.int64)
        refs.append(np.ascontiguousarray(np.clip(r + rng.integers(-2, 3, r.shape), 0, pmax).astype(ref.dtype)).ravel())
    return cur, refs, stride, origin


def me_layouts(star):
    """name -> list of groups, a group = (reference picture, its jobs: PUs of one 64x64 tile)"""
    methods = (T.ME_STAR, T.ME_HEX) if star else (T.ME_HEX, T.ME_DIA)
    pool = T.me_jobs(4700 + int(star), 400, methods=methods, submes=(2, 3), merange=16)
    tile = lambda j: (j["x"] >> 6, j["y"] >> 6)
    tiles = {}
    for j in pool:
        tiles.setdefault(tile(j), []).append(j)
    keys = sorted(tiles)
    assert len(keys) == 12 and all(len(tiles[k]) >= 12 for k in keys)
    return [("one group of 12 jobs", [(0, tiles[keys[5]][:12])]),
            ("3 groups of one job on three reference pictures", [(r, [tiles[keys[2]][r]]) for r in range(3)]),
            ("9 groups of one job", [(k % 3, [tiles[keys[k]][3]]) for k in range(9)]),
            ("3 groups, one of two jobs", [(0, [tiles[keys[7]][4]]), (1, tiles[keys[8]][4:6]), (2, [tiles[keys[9]][4]])])]


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("star", [False, True])
def test_me_search(depth, star):
    orc = T.load_oracle(depth)
    me = T.HipME(depth)
    cur, refs, stride, origin = me_scene(depth)
    op = "ME_SEARCH_STAR" if star else "ME_SEARCH"
    for name, layout in me_layouts(star):
        what = "%s, %s" % (op, name)
        groups, ordered, want, jobs_flat = [], [], [], []
        for ref, jobs in layout:
            packed = T.me_pack_jobs(jobs)
            g, order = me.plan(packed, ref, ME_WIN)
            assert len(g) == 1 and g[0]["num_jobs"] == len(jobs)
            g["first_job"] += len(ordered)
            groups.append(g)
            ordered += [packed[k] for k in order]
            jobs_flat += [jobs[k] for k in order]
            want.append(T.me_run_host(orc, cur, refs[ref], stride, origin, [jobs[k] for k in order]))
        groups = np.concatenate(groups); ordered = np.array(ordered, T.ME_JOB_DT); want = np.concatenate(want)
        d_cur, d_refs = me.upload(cur), [me.upload(r) for r in refs]
        with server_ran(me.L, what, ME_DEFERRED=1, **{op: 1}) as q:
            d_out = me.search(d_cur, d_refs, stride, origin, cur.itemsize, groups, ordered, ME_WIN, stream=q, flags=None)
        res = d_out.cpu().numpy().view(T.ME_RESULT_DT)
        got = np.stack([res["mv"][:, 0], res["mv"][:, 1], res["cost"]], 1).astype(np.int32)
        for i in range(len(want)):
            assert np.array_equal(got[i], want[i]), "%s: job %d (%s): (mvx, mvy, cost) %s, want %s" % (what, i, jobs_flat[i], got[i], want[i])
    me.close()


# ---- x265amd_inter_residual_rd on a queue: one TU_CHAIN command with all transform chains, a CU_MEASURE command of the predictions, the host's walk, and a second
# CU_MEASURE command that assembles the reconstruction from the chosen residual layers (assemble = 1) ----
@pytest.mark.parametrize("k", [0, 3, 4])
def test_inter_residual_rd_golden(k):
    depth, seed, st, td, psy = RD_CASES[k]
    hip = T.load_hip(depth)
    c = T.rd_case(depth, seed, st, td, psy)
    what = "inter_residual_rd, case %d (%d bits, %d CUs)" % (k, depth, len(c["cus"]))
    with server_ran(hip, what, TU_CHAIN=1, CU_MEASURE=2) as q:
        got = T.rd_run_hip(hip, c, stream=q)
    rd_check_golden(got, c, np.load(RD_GOLD_PATH), k)


def test_inter_residual_rd_batch():
    hip = T.load_hip(8)
    c = T.rd_case(8, 401, 0, 3, 2.0, ncu=200)
    with server_ran(hip, "inter_residual_rd, 200 CUs", TU_CHAIN=1, CU_MEASURE=2) as q:
        got = T.rd_run_hip(hip, c, stream=q)
    T.rd_compare(got, T.rd_run_stages_cpu(hip, T.load_oracle(8), c), c, "inter_residual_rd on a queue, 200 CUs")
