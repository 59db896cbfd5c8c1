"""Every slot x265amd_setup_primitives() installs, called THROUGH the table with the slot's typedef signature and compared with the oracle.

tests/golden/primitive_slots.json is the slot map: for every slot the function is meant to fill, its index, kind, size index, field and variant.  It is the output
of tests/native/slot_map_dump.cpp (this project's own header, x265-amod_amd/host/primitive_table.h); a non-GPU test builds that program again and requires the
same text, so the fixture cannot rot.  The GPU test reads only the JSON: it fills a zeroed table, requires the installed set to be exactly the fixture's, calls every
entry on random / min / max inputs (the buffers and value ranges of hevc_testlib's case_* functions) and requires the set of slots it has called to be the installed set,
so that a slot installed later without a case here fails.  Integer paths: the tolerance is zero."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import hevc_testlib as T

FIXTURE = os.path.join(T.GOLDEN_DIR, "primitive_slots.json")
TABLE_SLOTS = 2281
PTR, ISTRIDE, INT = C.c_void_p, C.c_int64, C.c_int          # pointer, intptr_t, int
GARBAGE_DIRMODE = 0x5A17                                    # what the planar / DC slots must ignore


def slot_map():
    with open(FIXTURE) as f:
        return json.load(f)


def test_slot_map_fixture_is_current(tmp_path):
    exe = str(tmp_path / "slot_map_dump")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(T.PKG_DIR, "host"), os.path.join(T.ROOT, "tests", "native", "slot_map_dump.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    with open(FIXTURE) as f:
        assert out == f.read(), "tests/golden/primitive_slots.json is not the output of tests/native/slot_map_dump.cpp"
    slots = json.loads(out)
    assert len(slots) == 943 and len({e["slot"] for e in slots}) == 943
    assert all(0 <= e["slot"] < TABLE_SLOTS for e in slots)
    assert {e["kind"] for e in slots} == {"pu", "cu", "misc", "chroma_pu", "chroma_cu"}
    assert {(e["kind"], e["field"]) for e in slots} == set(ORACLE_NAME), "a field without a case in this file (or a case without a field)"


# (kind, field) -> the oracle's function; its leading arguments are the size index (and the colour space)
ORACLE_NAME = {("pu", f): f for f in ("sad", "sad_x3", "sad_x4", "satd", "luma_hpp", "luma_hps", "luma_vpp", "luma_vps", "luma_vsp", "luma_vss", "luma_hvpp", "pixelavg_pp", "addAvg")}
ORACLE_NAME[("pu", "convert_p2s")] = "luma_p2s"
ORACLE_NAME.update({("cu", f): f for f in ("dct", "idct", "sub_ps", "add_ps", "copy_cnt", "count_nonzero", "cpy2Dto1D_shl", "cpy2Dto1D_shr", "cpy1Dto2D_shl", "cpy1Dto2D_shr",
                                          "var", "sse_pp", "sse_ss", "psy_cost_pp", "ssd_s", "sa8d", "transpose", "intra_filter", "intra_pred")})
ORACLE_NAME[("cu", "standard_dct")] = "dct"
ORACLE_NAME[("cu", "intra_pred_allangs")] = "intra_allangs"
ORACLE_NAME.update({("misc", f): f for f in ("dst4x4", "idst4x4", "quant", "nquant", "dequant_scaling", "dequant_normal", "scale1D_128to64", "scale2D_64to32", "weight_sp", "weight_pp")})
ORACLE_NAME.update({("chroma_pu", "filter_" + f): "chroma_" + f for f in ("vpp", "vps", "vsp", "vss", "hpp", "hps")})
ORACLE_NAME.update({("chroma_pu", "satd"): "chroma_satd", ("chroma_pu", "addAvg"): "chroma_addAvg", ("chroma_pu", "p2s"): "chroma_p2s", ("chroma_cu", "sa8d"): "chroma_sa8d"})


def signature(field, depth):
    """(restype, argtypes) of the slot's typedef (reference: primitives.h:133-236; locally the Thunk members of csrc/table_setup.hip)"""
    sse_t = C.c_uint64 if depth > 8 else C.c_uint32           # common/common.h:142-146
    cmp4 = [PTR, ISTRIDE, PTR, ISTRIDE]
    if field in ("sad", "satd", "sa8d", "psy_cost_pp"):
        return C.c_int, cmp4
    if field in ("sse_pp", "sse_ss"):
        return sse_t, cmp4
    if field == "ssd_s":
        return sse_t, [PTR, ISTRIDE]
    if field == "var":
        return C.c_uint64, [PTR, ISTRIDE]
    if field == "sad_x3":
        return None, [PTR] * 4 + [ISTRIDE, PTR]
    if field == "sad_x4":
        return None, [PTR] * 5 + [ISTRIDE, PTR]
    if field in ("luma_hpp", "luma_vpp", "luma_vps", "luma_vsp", "luma_vss", "filter_hpp", "filter_vpp", "filter_vps", "filter_vsp", "filter_vss"):
        return None, cmp4 + [INT]
    if field in ("luma_hps", "filter_hps", "luma_hvpp"):
        return None, cmp4 + [INT, INT]
    if field in ("convert_p2s", "p2s"):
        return None, cmp4
    if field == "pixelavg_pp":
        return None, [PTR, ISTRIDE, PTR, ISTRIDE, PTR, ISTRIDE, INT]
    if field == "addAvg":
        return None, [PTR, PTR, PTR, ISTRIDE, ISTRIDE, ISTRIDE]
    if field in ("dct", "idct", "standard_dct", "dst4x4", "idst4x4", "transpose", "scale2D_64to32"):
        return None, [PTR, PTR, ISTRIDE]
    if field in ("sub_ps", "add_ps"):
        return None, [PTR, ISTRIDE, PTR, PTR, ISTRIDE, ISTRIDE]
    if field == "copy_cnt":
        return C.c_uint32, [PTR, PTR, ISTRIDE]
    if field == "count_nonzero":
        return C.c_int, [PTR]
    if field.startswith("cpy"):
        return None, [PTR, PTR, ISTRIDE, INT]
    if field == "intra_pred_allangs":
        return None, [PTR, PTR, PTR, INT]
    if field in ("intra_filter", "scale1D_128to64"):
        return None, [PTR, PTR]
    if field == "intra_pred":
        return None, [PTR, ISTRIDE, PTR, INT, INT]
    if field == "quant":
        return C.c_uint32, [PTR] * 4 + [INT] * 3
    if field == "nquant":
        return C.c_uint32, [PTR] * 3 + [INT] * 3
    if field == "dequant_scaling":
        return None, [PTR] * 3 + [INT] * 3
    if field == "dequant_normal":
        return None, [PTR] * 2 + [INT] * 3
    if field == "weight_sp":
        return None, [PTR, PTR, ISTRIDE, ISTRIDE] + [INT] * 6
    if field == "weight_pp":
        return None, [PTR, PTR, ISTRIDE] + [INT] * 6
    raise KeyError(field)


def through_table(addr, field, depth):
    restype, argtypes = signature(field, depth)
    fn = C.CFUNCTYPE(restype, *argtypes)(addr)
    return lambda *args: fn(*[T._ptr(a) for a in args])


def through_oracle(orc, e):
    """the oracle's function for the entry, taking the arguments of the slot's typedef"""
    kind, field, size = e["kind"], e["field"], e["size"]
    name = ORACLE_NAME[(kind, field)]
    lead = () if kind == "misc" else ((T.CSP_I420, size) if kind.startswith("chroma") else (size,))
    if field == "pixelavg_pp":          # the slot's trailing weight argument is not the oracle's
        return lambda dst, ds, s0, ss0, s1, ss1, weight: orc.call(name, *lead, dst, ds, s0, ss0, s1, ss1)
    if field == "intra_pred":           # the slot decides the mode: planar and DC whatever dirMode says, and the angular slots are called with their own mode
        return lambda dst, ds, src, dirMode, bFilter: orc.call(name, size, e["variant"], dst, ds, src, bFilter)
    return lambda *args: orc.call(name, *lead, *args)


def block_size(e):
    if e["kind"] in ("pu", "chroma_pu"):
        w, h = T.PU_SIZES[e["size"]]
    else:
        w = h = 4 << e["size"]
    return (w // 2, h // 2) if e["kind"].startswith("chroma") else (w, h)


def exercise(e, call, P, rng, mode):
    """one call of the entry's function type (the installed thunk, or the oracle) on buffers drawn from rng: every output, as a list of arrays"""
    field, (w, h) = e["field"], block_size(e)
    opp = "random" if mode == "random" else ("max" if mode == "min" else "min")
    lim = P.pmax
    pad = lambda n=9: 2 * int(rng.integers(0, n))
    if field in ("sad", "satd", "sa8d", "psy_cost_pp", "sse_pp"):
        sa, sb, o = w + pad(), w + pad(40), int(rng.integers(0, 16))
        a, b = T.pix_buf(P, rng, sa * h, mode), T.pix_buf(P, rng, sb * h + 16, opp)
        return [np.array([call(a, sa, T.off(b, o), sb)], np.uint64 if field == "sse_pp" else np.int64)]
    if field in ("sse_ss", "ssd_s"):
        sa, sb = w + pad(), w + pad(40)
        a, b = T.s16_buf(rng, sa * h, -lim, lim, mode), T.s16_buf(rng, sb * h, -lim, lim, opp)
        return [np.array([call(a, sa, b, sb) if field == "sse_ss" else call(a, sa)], np.uint64)]
    if field == "var":
        sa = w + pad()
        return [np.array([call(T.pix_buf(P, rng, sa * h, mode), sa)], np.uint64)]
    if field in ("sad_x3", "sad_x4"):
        sb, o = 64 + pad(40), int(rng.integers(0, 16))
        a, b = T.pix_buf(P, rng, 64 * 64, mode), T.pix_buf(P, rng, sb * 80 + 80, opp)
        res = np.zeros(4, np.int32)
        refs = [T.off(b, o), T.off(b, o + 1), T.off(b, o + sb), T.off(b, o + 3 * sb + 1)]
        call(a, *refs[:3 if field == "sad_x3" else 4], sb, res)
        return [res]
    if field in ("luma_hpp", "luma_hps", "luma_vpp", "luma_vps", "luma_vsp", "luma_vss", "luma_hvpp", "convert_p2s",
                 "filter_hpp", "filter_hps", "filter_vpp", "filter_vps", "filter_vsp", "filter_vss", "p2s"):
        chroma = e["kind"] == "chroma_pu"
        ss, ds = w + 8 + pad(), w + pad(5)
        from16, to16 = field[-3:] in ("vsp", "vss"), field[-3:] in ("hps", "vps", "vss", "p2s")
        src = T.s16_buf(rng, ss * (h + 8) + 16, -8192, 8191, mode) if from16 else T.pix_buf(P, rng, ss * (h + 8) + 16, mode)
        dst = np.zeros(ds * (h + 8), np.int16 if to16 else P.pixel)
        idx = int(rng.integers(0, 8 if chroma else 4))
        if field == "luma_hvpp":
            tail = (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
        elif field[-3:] == "hps":
            tail = (idx, int(rng.integers(0, 2)))          # isRowExt
        elif field[-3:] == "p2s":
            tail = ()
        else:
            tail = (idx,)
        call(T.off(src, 4 * ss + 4), ss, dst, ds, *tail)
        return [dst]
    if field == "pixelavg_pp":
        s0, s1, ds = w + pad(), w + pad(), w + pad()
        a, b, d = T.pix_buf(P, rng, s0 * h, mode), T.pix_buf(P, rng, s1 * h, mode), np.zeros(ds * h, P.pixel)
        call(d, ds, a, s0, b, s1, 32)                   # the trailing argument: the averaging weight, 32 from every caller of the reference
        return [d]
    if field == "addAvg":
        s0, s1, ds = w + pad(), w + pad(), w + pad()
        x, y, d = T.s16_buf(rng, s0 * h, -8192, 8191, mode), T.s16_buf(rng, s1 * h, -8192, 8191, mode), np.zeros(ds * h, P.pixel)
        call(x, y, d, s0, s1, ds)
        return [d]
    if field in ("dct", "standard_dct", "dst4x4"):
        st = w + 8 * int(rng.integers(0, 3))
        d = np.zeros(w * w, np.int16)
        call(T.s16_buf(rng, st * w, -lim, lim, mode), d, st)
        return [d]
    if field in ("idct", "idst4x4"):
        st = w + 8 * int(rng.integers(0, 3))
        d = np.zeros(st * w, np.int16)
        call(T.s16_buf(rng, w * w, -32768, 32767, mode), d, st)
        return [d]
    if field in ("sub_ps", "add_ps"):
        s0, s1, ds = w + pad(), w + pad(), w + pad()
        a = T.pix_buf(P, rng, s0 * w, mode)
        b = T.pix_buf(P, rng, s1 * w, opp) if field == "sub_ps" else T.s16_buf(rng, s1 * w, -lim, lim, mode)
        d = np.zeros(ds * w, np.int16 if field == "sub_ps" else P.pixel)
        call(d, ds, a, b, s0, s1)
        return [d]
    if field == "copy_cnt":
        st = w + pad()
        d = np.zeros(w * w, np.int16)
        n = call(d, T.s16_buf(rng, st * w, -3, 3, mode), st)
        return [np.array([n], np.int64), d]
    if field == "count_nonzero":
        return [np.array([call(T.s16_buf(rng, w * w, -3, 3, mode))], np.int64)]
    if field.startswith("cpy"):
        st, shift = w + pad(), int(rng.integers(1, 3))
        to1d = field.startswith("cpy2Dto1D")
        s = T.s16_buf(rng, st * w, -4096, 4095, mode)
        d = np.zeros(w * w if to1d else st * w, np.int16)
        call(d, s, st, shift)
        return [d]
    if field == "transpose":
        st = w + pad()
        d = np.zeros(w * w, P.pixel)
        call(d, T.pix_buf(P, rng, st * w, mode), st)
        return [d]
    if field in ("intra_filter", "intra_pred", "intra_pred_allangs"):
        nb = T.pix_buf(P, rng, 4 * w + 1 + 16, mode)
        if mode == "random" and rng.integers(0, 2):
            nb = np.clip(np.cumsum(rng.integers(-3, 4, nb.size)) + P.pmax // 2, 0, P.pmax).astype(P.pixel)
        if field == "intra_filter":
            d = np.zeros_like(nb)
            call(nb, d)
        elif field == "intra_pred":
            ds = w + 8 * int(rng.integers(0, 3))
            d = np.zeros(ds * w, P.pixel)
            call(d, ds, nb, GARBAGE_DIRMODE if e["variant"] < 2 else e["variant"], int(rng.integers(0, 2)))
        else:
            d = np.zeros(33 * w * w, P.pixel)
            call(d, nb, T.pix_buf(P, rng, nb.size, mode), int(rng.integers(0, 2)))
        return [d]
    if field in ("quant", "nquant", "dequant_normal", "dequant_scaling"):
        cu = int(rng.integers(0, 4))
        n, qp = (4 << cu) ** 2, int(rng.integers(0, 52))
        per, rem, tshift = qp // 6, qp % 6, 15 - P.depth - (cu + 2)
        qbits, shift = 14 + per + tshift, 20 - 14 - tshift
        add = (171 if rng.integers(0, 2) else 85) << (qbits - 9)
        coef = T.s16_buf(rng, n, -32768, 32767, mode)
        qc = np.full(n, T.QUANT_SCALES[rem], np.int32)
        dq = np.full(n, T.INV_QUANT_SCALES[rem] * 16, np.int32)
        if mode == "random":
            qc = (qc.astype(np.int64) * 16 // rng.integers(8, 40, n)).astype(np.int32)
            dq = (T.INV_QUANT_SCALES[rem] * rng.integers(8, 40, n)).astype(np.int32)
        q = np.zeros(n, np.int16)
        if field == "quant":
            du = np.zeros(n, np.int32)
            return [np.array([call(coef, qc, du, q, qbits, add, n)], np.int64), du, q]
        if field == "nquant":
            return [np.array([call(coef, qc, q, qbits, add, n)], np.int64), q]
        if field == "dequant_normal":
            call(coef, q, n, T.INV_QUANT_SCALES[rem] << per, shift)
        else:
            call(coef, dq, q, n, per, shift)
        return [q]
    if field == "scale1D_128to64":
        d = np.zeros(128, P.pixel)
        call(d, T.pix_buf(P, rng, 256, mode))
        return [d]
    if field == "scale2D_64to32":
        st = 64 + pad()
        d = np.zeros(32 * 32, P.pixel)
        call(d, T.pix_buf(P, rng, st * 64, mode), st)
        return [d]
    if field in ("weight_pp", "weight_sp"):
        corr = 14 - P.depth
        ww, hh, st = 16 * int(rng.integers(1, 5)), int(rng.integers(1, 17)), 64 + 16 * int(rng.integers(0, 3))
        w0, shift, offset = int(rng.integers(1, 128)), int(rng.integers(0, 7)) + corr, int(rng.integers(-20, 21))
        rnd = ((1 << (shift - 1)) if shift else 0) & ~((1 << corr) - 1)
        d = np.zeros(st * 16, P.pixel)
        if field == "weight_pp":                        # widths that are multiples of 16
            call(T.pix_buf(P, rng, st * 16, mode), d, st, ww, hh, w0, rnd, shift, offset)
        else:
            call(T.s16_buf(rng, st * 16, -8192, 8191, mode), d, st, st, ww - 1, hh, w0, rnd, shift, offset)
        return [d]
    raise KeyError(field)


@pytest.mark.parametrize("depth", [8, 10])
def test_slot_cases_on_the_oracle(depth):
    """without a GPU: every entry of the map has a signature and a case, and the case is deterministic (the same seed gives the same inputs to both sides)"""
    orc = T.load_oracle(depth)
    for e in slot_map():
        restype, argtypes = signature(e["field"], depth)
        seed = T.case_seed("slot%d" % e["slot"], depth, "random", 0)
        one = exercise(e, through_oracle(orc, e), orc, np.random.default_rng(seed), "random")
        two = exercise(e, through_oracle(orc, e), orc, np.random.default_rng(seed), "random")
        T.assert_same(one, two, "slot %d" % e["slot"])
        assert any(a.any() for a in one) or e["field"] in ("count_nonzero", "copy_cnt"), e


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_every_installed_slot(depth):
    hip, orc = T.load_hip(depth), T.load_oracle(depth)
    slots = slot_map()
    table = (C.c_void_p * TABLE_SLOTS)()
    hip.lib.x265amd_primitives_table_bytes.restype = C.c_size_t
    assert hip.lib.x265amd_primitives_table_bytes() == TABLE_SLOTS * 8
    nset = hip.lib.x265amd_setup_primitives(table, C.c_size_t(TABLE_SLOTS * 8))
    installed = {i for i in range(TABLE_SLOTS) if table[i]}
    assert len(installed) == nset == 943
    assert installed == {e["slot"] for e in slots}, "installed slots and tests/golden/primitive_slots.json differ"      # and everything else is still NULL
    # the NULL holes of the 4:2:0 sub-table: nothing but addAvg for part 0, chroma_satd only where the half partition is a multiple of 4x4
    have = {(e["kind"], e["size"], e["field"]) for e in slots}
    assert {f for k, s, f in have if k == "chroma_pu" and s == 0} == {"addAvg"}
    assert {s for k, s, f in have if k == "chroma_pu" and f == "satd"} == {p for p in range(25) if T.chroma_satd_defined(p)}
    called = set()
    for e in slots:
        for mode in T.MODES:
            seed = T.case_seed("slot%d" % e["slot"], depth, mode, 0)
            got = exercise(e, through_table(table[e["slot"]], e["field"], depth), hip, np.random.default_rng(seed), mode)
            want = exercise(e, through_oracle(orc, e), orc, np.random.default_rng(seed), mode)
            T.assert_same(got, want, "slot %d (%s[%d].%s variant %s) depth %d %s" % (e["slot"], e["kind"], e["size"], e["field"], e["variant"], depth, mode))
        called.add(e["slot"])
    assert called == installed, "installed slots without a call: %s" % sorted(installed - called)


@pytest.mark.gpu
def test_sse_ss_beyond_32_bits():
    """10 bits: cu[4].sse_ss of +1023 against -1023 is 4096 * 2046^2 > 2^32 and comes back whole through the slot's 64-bit sse_t; at 8 bits sse_t is 32 bits wide
    and the same call through a uint32 return gives the oracle's value (+255 against -255: 4096 * 510^2 fits)"""
    slot = next(e["slot"] for e in slot_map() if (e["kind"], e["size"], e["field"]) == ("cu", 4, "sse_ss"))
    for depth in (8, 10):
        hip, orc = T.load_hip(depth), T.load_oracle(depth)
        table = (C.c_void_p * TABLE_SLOTS)()
        assert hip.lib.x265amd_setup_primitives(table, C.c_size_t(TABLE_SLOTS * 8)) == 943
        a, b = np.full(64 * 64, hip.pmax, np.int16), np.full(64 * 64, -hip.pmax, np.int16)
        got = through_table(table[slot], "sse_ss", depth)(a, 64, b, 64)
        assert got == orc.call("sse_ss", 4, a, 64, b, 64) == 4096 * (2 * hip.pmax) ** 2
        assert (got > 1 << 32) == (depth == 10)
