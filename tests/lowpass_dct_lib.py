"""--lowpass-dct: what the tests of the low-pass transform and the scripts that record their fixtures share -- the inputs of the primitive cases, the selection
of the transform-unit cases (from the generators of hevc_testlib, by fixed seeds), runners that take the jobs' flags byte, and the packing of results.

The fixtures (tests/golden/lowpass_dct_golden.npz) hold the REFERENCE's outputs: its own lowpass_dct slots and its own Quant with the table switched the way
enableLowpassDCTPrimitives switches it (tests/golden/make_lowpass_dct_golden.py)."""
import ctypes as C
import os

import numpy as np

import hevc_testlib as T

TU_LOWPASS = 1              # X265AMD_TU_LOWPASS (include/x265amd.h)
OP_LOWPASS_DCT = 80         # X265AMD_OP_LOWPASS_DCT
GOLDEN = os.path.join(T.GOLDEN_DIR, "lowpass_dct_golden.npz")


# ---- the primitive: cu[].lowpass_dct ----
def prim_inputs(depth):
    """[(name, cu, stride, int16 array [N, stride])]: residual-range random blocks, a stride above N, the extremes, the wraps of the first coefficient and the floors
    of the shifts on negative sums, and one block over the whole int16 range (the 2x2 sums wrap)"""
    rng = np.random.default_rng(7700 + depth)
    pmax = (1 << depth) - 1
    out = []
    for cu in (1, 2, 3):
        N = 4 << cu
        for k in range(2):
            out.append(("random%d" % k, cu, N, rng.integers(-pmax, pmax + 1, (N, N)).astype(np.int16)))
        out.append(("stride", cu, N + 5, rng.integers(-pmax, pmax + 1, (N, N + 5)).astype(np.int16)))
        out.append(("pos_max", cu, N, np.full((N, N), pmax, np.int16)))
        out.append(("neg_max", cu, N, np.full((N, N), -pmax, np.int16)))
        for v in (1, 2, 3):
            # every 2x2 cell sums to -v: `>> 2` floors it to -1, and the total (-v * cells) goes through `>> 1` / `>> 3`
            b = np.zeros((N, N), np.int16)
            b[0::2, 0::2] = -1
            if v >= 2:
                b[1::2, 1::2] = -1
            if v >= 3:
                b[0::2, 1::2] = -1
            out.append(("cell_m%d" % v, cu, N, b))
        # one cell of -1, -2, -3 in a block of zeros: the total itself is -1, -2, -3
        for v in (1, 2, 3):
            b = np.zeros((N, N), np.int16)
            b[0, 0] = -v
            out.append(("total_m%d" % v, cu, N, b))
        out.append(("int16_range", cu, N, rng.integers(-32768, 32768, (N, N)).astype(np.int16)))
    b = np.full((16, 16), 256, np.int16)
    out.append(("mean256", 2, 16, b))
    b = b.copy()
    b[7, 9] = 255
    out.append(("mean256_less", 2, 16, b))
    return out


def prim_key(depth, name, cu):
    return "prim%d/%s/%d" % (depth, name, cu)


def lowpass_model(src, cu, dct_half):
    """numpy restatement of lowPassDct8_c / 16_c / 32_c (lowpassdct.cpp:34-112) over the standard transform of half the size: dct_half(int16 [H, H]) -> int16 [H, H]"""
    N = 4 << cu
    H = N // 2
    s = src[:, :N].astype(np.int32)
    cell = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]).astype(np.int16)          # int16_t sum
    avg = (cell >> 2).astype(np.int16)
    out = np.zeros((N, N), np.int16)
    out[:H, :H] = dct_half(np.ascontiguousarray(avg))
    total = int(cell.astype(np.int64).sum())
    if cu == 1:
        dc = (((total + 32768) % 65536 - 32768) << 1)                # an int16_t total, then `<< 1`
    else:
        dc = total >> (1 if cu == 2 else 3)
    out[0, 0] = (dc + 32768) % 65536 - 32768                          # the cast wraps
    return out


# ---- transform-unit cases ----
_KEYS_INTER = [(5, 0), (4, 0), (4, 1), (4, 2), (3, 0), (3, 1), (2, 0), (2, 2)]
_KEYS_INTRA = [(5, 0), (4, 0), (4, 1), (4, 2), (3, 0), (3, 2), (2, 0)]


def inter_cases(depth):
    """40 units of hevc_testlib.tu_cases: per (size, plane) three with sign hiding and two without"""
    pool = T.tu_cases(depth, 9001 + depth, 600)
    out = []
    for key in _KEYS_INTER:
        for sh, cnt in ((1, 3), (0, 2)):
            got = [c for c in pool if (c["log2"], c["ttype"]) == key and c["signhide"] == sh][:cnt]
            assert len(got) == cnt, key
            out += got
    return out


_INTRA_POOL = {}


def _intra_pool(depth):
    if depth not in _INTRA_POOL:
        _INTRA_POOL[depth] = T.intra_tu_cases(depth, 9002 + depth, 900, rdoq=True)
    return _INTRA_POOL[depth]


def intra_cases(depth, rdoq):
    """units of hevc_testlib.intra_tu_cases.  rdoq False: three per (size, plane), plain quantisation.  True: per (size, plane) two of RDOQ level 1 and two of level 2,
    a psy-RDOQ scale among the luma ones of every size"""
    pool = _intra_pool(depth)
    out = []
    for key in _KEYS_INTRA:
        if not rdoq:
            got = [dict(c, rdoq=0) for c in pool if (c["log2"], c["ttype"]) == key and c["rdoq"] == 0][:3]
            assert len(got) == 3, key
            out += got
        else:
            for lvl in (1, 2):
                got = [c for c in pool if (c["log2"], c["ttype"]) == key and c["rdoq"] == lvl and (key[1] != 0 or c["psyrdoq"] != 0)][:2]
                assert len(got) == 2, (key, lvl)
                out += got
    return out


def as_tu_cases(cases, preds):
    """intra units with their predictions given, as units of x265amd_tu_chain_rdoq (intra = 1, the mode selects the scan)"""
    return [dict(fenc=np.ascontiguousarray(c["fenc"]), pred=np.ascontiguousarray(p), log2=c["log2"], ttype=c["ttype"], intra=1, dir=c["mode"], slice=c["slice"], qp=c["qp"],
                 signhide=c["signhide"], rdoq=c["rdoq"], psyrdoq=c["psyrdoq"], tudepth=c["tudepth"], ctx=c["ctx"]) for c, p in zip(cases, preds)]


def flat(results, names):
    """list of per-unit tuples -> {name: one flat array}; names: the tuple's members in order ('stats' first)"""
    out = {}
    for k, name in enumerate(names):
        if name == "stats":
            out[name] = np.array([[int(v) for v in r[k]] for r in results], np.uint64)
        else:
            out[name] = np.concatenate([np.asarray(r[k]).ravel() for r in results])
    return out


INTER_NAMES = ("stats", "coeff", "resi", "recon")
INTRA_NAMES = ("stats", "pred", "recon", "coeff", "resi")


def assert_units(got, want, cases, names, what, only=None):
    """per unit and member; want: tuples like got.  only: indices to compare"""
    assert len(got) == len(want) == len(cases)
    for i, (c, g, w) in enumerate(zip(cases, got, want)):
        if only is not None and i not in only:
            continue
        for k, name in enumerate(names):
            a, b = np.asarray(g[k]).ravel().astype(np.int64), np.asarray(w[k]).ravel().astype(np.int64)
            assert a.shape == b.shape and np.array_equal(a, b), "%s: unit %d (%dx%d, plane %d): %s" % (what, i, 1 << c["log2"], 1 << c["log2"], c["ttype"], name)


def unflat(g, prefix, cases, names):
    """the tuples back from the fixture's flat arrays"""
    out = [[] for _ in cases]
    for name in names:
        a = g[prefix + name]
        if name == "stats":
            for i in range(len(cases)):
                out[i].append(a[i])
            continue
        o = 0
        for i, c in enumerate(cases):
            n = 1 << (2 * c["log2"])
            out[i].append(a[o:o + n])
            o += n
        assert o == len(a), (prefix, name)
    return [tuple(r) for r in out]


# ---- runners with the flags byte ----
def tu_run_ref(R, cases):
    """<prefix>tu_chain_batch on host memory (plain quantisation): list of (stats[5], coeff, resi, recon)"""
    n = len(cases)
    dt = cases[0]["fenc"].dtype
    isz = dt.itemsize
    per = 32 * 32 * (isz * 3 + 2 * 2)
    arena = np.zeros(n * per, np.uint8)
    jobs = np.zeros(n, T.TU_JOB_DT)
    a0 = arena.ctypes.data
    for i, c in enumerate(cases):
        N = 1 << c["log2"]
        base = i * per
        arena[base:base + 1024 * isz].view(dt).reshape(32, 32)[:N, :N] = c["fenc"]
        arena[base + 1024 * isz:base + 2048 * isz].view(dt).reshape(32, 32)[:N, :N] = c["pred"]
        b = a0 + base
        jobs[i] = (b, b + 1024 * isz, b + 3072 * isz, b + 3072 * isz + 2048, b + 2048 * isz, 32, 32, 32, 32,
                   c["log2"], c["ttype"], c["intra"], c["dir"], c["slice"], c["qp"], c["signhide"], 0)
    res = np.zeros(n, T.TU_RESULT_DT)
    assert getattr(R.lib, R.prefix + "tu_chain_batch")(T._ptr(jobs), n, T._ptr(res)) == n
    out = T.tu_chain_unpack(cases, res, arena, per, dt)
    # a unit without levels: the batch entry leaves reconstruction and residual alone; the device writes the prediction and zeros
    fixed = []
    for c, (st, coeff, resi, recon) in zip(cases, out):
        if int(st[0]) == 0:
            recon, resi = c["pred"].copy(), np.zeros_like(resi)
        fixed.append((st, coeff, resi, recon))
    return fixed


def tu_run_hip(L, cases, flags, rdoq=False, stream=None):
    """x265amd_tu_chain / x265amd_tu_chain_rdoq with flags[i] in the jobs' flags byte: list of (stats[5], coeff, resi, recon)"""
    import torch
    dt = L.pixel
    isz = np.dtype(dt).itemsize
    n = len(cases)
    per = 32 * 32 * (isz * 3 + 2 * 2)
    arena = np.zeros(n * per, np.uint8)
    for i, c in enumerate(cases):
        N = 1 << c["log2"]
        base = i * per
        arena[base:base + 1024 * isz].view(dt).reshape(32, 32)[:N, :N] = c["fenc"]
        arena[base + 1024 * isz:base + 2048 * isz].view(dt).reshape(32, 32)[:N, :N] = c["pred"]
    d_arena = torch.from_numpy(arena).cuda()
    a0 = d_arena.data_ptr()
    jobs = np.zeros(n, T.TU_JOB_DT)
    rq = np.zeros(n, T.TU_RDOQ_DT)
    d_est = None
    if rdoq:
        orc = T.load_oracle(L.depth)
        d_est = torch.from_numpy(np.stack([T.est_bit(orc, c["ctx"], c["log2"], int(c["ttype"] == 0)) for c in cases])).cuda()
    for i, c in enumerate(cases):
        b = a0 + i * per
        jobs[i] = (b, b + 1024 * isz, b + 3072 * isz, b + 3072 * isz + 2048, b + 2048 * isz, 32, 32, 32, 32,
                   c["log2"], c["ttype"], c["intra"], c["dir"], c["slice"], c["qp"], c["signhide"], int(flags[i]))
        if rdoq:
            l2, l1 = C.c_int64(0), C.c_int32(0)
            L.lib.x265amd_rdoq_lambda(c["qp"], C.byref(l2), C.byref(l1))
            rq[i] = (d_est.data_ptr() + i * T.EST_INTS * 4, l2.value, l1.value, c["psyrdoq"], c["rdoq"], c["tudepth"], 0)
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_rq = torch.from_numpy(rq.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(n * T.TU_RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    with T.stream_scope(stream) as st:
        if rdoq:
            rc = L.lib.x265amd_tu_chain_rdoq(st, C.c_void_p(d_jobs.data_ptr()), C.c_void_p(d_rq.data_ptr()), n, C.c_void_p(d_out.data_ptr()))
        else:
            rc = L.lib.x265amd_tu_chain(st, C.c_void_p(d_jobs.data_ptr()), n, C.c_void_p(d_out.data_ptr()))
    assert rc == 0, L.lib.x265amd_last_error()
    return T.tu_chain_unpack(cases, d_out.cpu().numpy().view(T.TU_RESULT_DT), d_arena.cpu().numpy(), per, dt)


def intra_run_hip(L, cases, flags, stream=None):
    """x265amd_intra_tu_chain (its RDOQ form when a unit asks for it) with flags[i] in the jobs' flags byte: list of (stats, pred, recon, coeff, resi)"""
    import torch
    n = len(cases)
    dt = cases[0]["plane"].dtype
    isz = dt.itemsize
    per = T.INTRA_TU_OUT_BYTES(isz)
    orc = T.load_oracle(L.depth)
    ests = np.stack([T.est_bit(orc, c["ctx"], c["log2"], int(c["ttype"] == 0)) for c in cases])
    planes = np.concatenate([c["plane"].view(np.uint8) for c in cases])
    fencs = np.concatenate([c["fenc"].ravel().view(np.uint8) for c in cases])
    po = np.cumsum([0] + [c["plane"].nbytes for c in cases])
    fo = np.cumsum([0] + [c["fenc"].nbytes for c in cases])
    d_planes, d_fencs, d_est = torch.from_numpy(planes).cuda(), torch.from_numpy(fencs).cuda(), torch.from_numpy(ests).cuda()
    d_arena = torch.zeros(n * per, dtype=torch.uint8, device="cuda")
    jobs, rq = T.intra_tu_pack(cases, lambda i: d_planes.data_ptr() + int(po[i]), lambda i: d_fencs.data_ptr() + int(fo[i]), lambda i: d_arena.data_ptr() + i * per,
                               lambda i: d_est.data_ptr() + i * T.EST_INTS * 4, L)
    jobs["tu"]["reserved"] = np.asarray(flags, np.uint8)           # (the flags byte, by the name the record's mirror gave it when it was reserved)
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_rq = torch.from_numpy(rq.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(n * T.TU_RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    with T.stream_scope(stream) as st:
        rc = L.lib.x265amd_intra_tu_chain(st, C.c_void_p(d_jobs.data_ptr()), C.c_void_p(d_rq.data_ptr()) if any(c["rdoq"] for c in cases) else None, n,
                                          C.c_void_p(d_out.data_ptr()))
    assert rc == 0, L.lib.x265amd_last_error()
    return T.intra_tu_unpack(cases, d_out.cpu().numpy().view(T.TU_RESULT_DT), d_arena.cpu().numpy(), per)
