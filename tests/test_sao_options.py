"""The SAO options on the CPU (--sao-non-deblock, --limit-sao, --selective-sao): the host model of the statistics (x265amd_sao_stats_model, host/sao_stats_model.cpp)
against a restatement of the reference's two functions written from sao.cpp line by line (tests/sao_options_lib.py) and, in its default form, against the oracle path
the existing SAO tests use; the refusals of the model and of the decision's option forms; the layout of x265amd_param_ext and of x265_param.bLimitSAO; x265_param_parse
of the three options member by member against the reference library's own.  The rules of x265amd_encoder_open_ext need a device to open an encoder on: they are in
tests/test_encoder_sao_options.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import hevc_testlib as T
import sao_options_lib as S


def lib(depth):
    return T.load_hip(depth).lib


@functools.lru_cache(maxsize=None)
def planes(content, w, h, depth):
    return S.plane_set(content, w, h, depth)


@functools.lru_cache(maxsize=None)
def model_of(content, w, h, depth, flags):
    rec, fenc, pre = planes(content, w, h, depth)
    return S.model(lib(depth), rec, fenc, pre, w, h, flags, want_pre=True)


# the restatement walks every sample in Python: every content on the two shapes with partial CTUs at 8 bits, the noise set alone on the others and at 10 bits
RESTATED = [(c, w, h, 8) for c in S.CONTENTS for (w, h) in ((136, 72), (200, 152))] + [("noise", 64, 64, 8), ("noise", 128, 128, 8), ("noise", 64, 64, 10), ("noise", 136, 72, 10)]


@pytest.mark.parametrize("content,w,h,depth", RESTATED)
def test_model_equals_the_restated_reference_functions(content, w, h, depth):
    """(a) calcSaoStatsCTU with the non-deblock skips and (b) calcSaoStatsCu_BeforeDblk, word for word"""
    rec, fenc, pre = planes(content, w, h, depth)
    m = model_of(content, w, h, depth, S.NON_DEBLOCK)
    cnt, org = S.restated_picture(rec, fenc, w, h, depth, lambda r, f, cx, cy, pl: S.calc_sao_stats_ctu(r, f, w, h, cx, cy, pl, True, False, depth))
    assert np.array_equal(m["count"], cnt) and np.array_equal(m["org"], org)
    pcnt, porg = S.restated_picture(pre, fenc, w, h, depth, lambda r, f, cx, cy, pl: S.calc_sao_stats_cu_before_dblk(r, f, w, h, cx, cy, pl, depth))
    assert np.array_equal(m["pre_count"], pcnt) and np.array_equal(m["pre_org"], porg)


@pytest.mark.parametrize("w,h", [(136, 72), (200, 152)])
def test_model_without_eo2_eo3_equals_the_restated_b_slice_form(w, h):
    """--limit-sao in a B slice (sao.cpp:861), with and without the non-deblock skips"""
    rec, fenc, pre = planes("noise", w, h, 8)
    for nd in (False, True):
        m = model_of("noise", w, h, 8, S.EO01_ONLY | (S.NON_DEBLOCK if nd else 0))
        cnt, org = S.restated_picture(rec, fenc, w, h, 8, lambda r, f, cx, cy, pl: S.calc_sao_stats_ctu(r, f, w, h, cx, cy, pl, nd, True, 8))
        assert np.array_equal(m["count"], cnt) and np.array_equal(m["org"], org)
        assert not m["count"].reshape(-1, 5, 32)[:, 2:4].any() and not m["org"].reshape(-1, 5, 32)[:, 2:4].any()


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", S.SHAPES)
def test_default_form_equals_the_oracle_path(depth, w, h):
    """flags 0 = SAO::calcSaoStatsCTU as the existing tests check it: the C oracle always, the reference's own SAO class (ref_sao_stats_picture) where it is built"""
    for content in ("noise", "checker", "ramp_d45"):
        rec, fenc, pre = planes(content, w, h, depth)
        m = model_of(content, w, h, depth, 0)
        case = dict(rec=rec, fenc=fenc, stride=w, cstride=w // 2, org=(0, 0), width=w, height=h, nctu=S.nctu(w, h))
        oracles = [T.load_oracle(depth)] + ([T.load_ref(depth)] if T.have_ref() else [])
        for O in oracles:
            # the oracle path applies offsets, too: parameters that switch every CTU off
            case["params"] = np.zeros(case["nctu"], T.SAO_CTU_DT); case["params"]["type"] = -1
            cnt, org, _ = T.sao_run_host(O, case)
            assert np.array_equal(m["count"], cnt) and np.array_equal(m["org"], org), (content, O.prefix)
        # the pre-deblock record does not depend on the flags
        assert np.array_equal(m["pre_count"], model_of(content, w, h, depth, S.NON_DEBLOCK)["pre_count"])


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", S.SHAPES)
def test_noise_set_fills_every_class(depth, w, h):
    """the condition tests/test_hip_sao_options.py asserts before it compares a kernel: no class of the noise set is empty in either record"""
    m = model_of("noise", w, h, depth, S.NON_DEBLOCK)
    assert S.classes_covered(m["count"])
    if (w, h) == (64, 64):
        # one CTU at the right and bottom edge at once: every start of calcSaoStatsCu_BeforeDblk collapses onto its end (sao.cpp:997-998, :1024-1028, :1060-1064), so the
        # reference's own pre-deblock record of this picture is all zero -- which is what the shape is there to show
        assert not m["pre_count"].any() and not m["pre_org"].any()
    else:
        assert S.classes_covered(m["pre_count"])
    # the two regions are not a partition: together they hold more BO samples than the picture has where CTUs meet, fewer at none
    area = w * h + 2 * (w // 2) * (h // 2)
    total = int(m["count"].reshape(-1, 5, 32)[:, 4].sum() + m["pre_count"].reshape(-1, 5, 32)[:, 4].sum())
    assert total == area, (total, area)          # (BO's two regions do partition the CTU: x < endX && y < endY against x >= startX || y >= startY with equal bounds)


def test_model_refusals():
    L = lib(8)
    rec, fenc, pre = planes("flat", 64, 64, 8)
    fn = L.x265amd_sao_stats_model
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = S.nctu(64, 64) * 3 * S.WORDS
    a, b, c, d = (np.zeros(n, np.int32) for _ in range(4))
    R, F, P = S._tab(rec), S._tab(fenc), S._tab(pre)
    p = lambda x: x.ctypes.data
    assert fn(R, F, P, 64, 32, 64, 64, 0, p(a), p(b), p(c), p(d)) == 0
    assert fn(R, F, P, 64, 32, 64, 64, 4, p(a), p(b), p(c), p(d)) != 0                # an unknown flag
    assert fn(R, None, P, 64, 32, 64, 64, 0, p(a), p(b), p(c), p(d)) != 0             # no source planes
    assert fn(None, F, P, 64, 32, 64, 64, 0, p(a), p(b), p(c), p(d)) != 0             # statistics wanted without the deblocked planes
    assert fn(R, F, None, 64, 32, 64, 64, 0, p(a), p(b), p(c), p(d)) != 0             # the pre-deblock record wanted without its planes
    assert fn(R, F, P, 64, 32, 64, 64, 0, p(a), None, p(c), p(d)) != 0                # half a record
    assert fn(R, F, P, 64, 32, 64, 64, 0, None, None, None, None) != 0                # nothing wanted
    assert fn(R, F, P, 64, 32, 60, 64, 0, p(a), p(b), p(c), p(d)) != 0                # a width that is no multiple of 8
    assert fn(R, F, None, 64, 32, 64, 64, 0, None, None, p(c), p(d)) == 0             # the post-deblock record alone


def test_decision_option_forms_refuse_inconsistent_records():
    """x265amd_sao_rdo_opt: the pre-deblock record comes with X265AMD_SAO_NON_DEBLOCK and only with it; unknown flags are refused -- before anything else is looked at"""
    L = lib(8)
    si = np.zeros(1, T.SLICE_INFO_DT); si["pic_width"] = 64; si["pic_height"] = 64; si["slice_type"] = 1; si["slice_qp"] = 30
    n = S.nctu(64, 64) * 3 * S.WORDS
    cnt, org = np.zeros(n, np.int32), np.zeros(n, np.int32)
    units = np.zeros(16 * 16, T.CU_UNIT_DT)
    rate = np.zeros(8, np.float64); par = np.zeros(1, T.SAO_CTU_PROD_DT); flags = np.zeros(2, np.int32)
    fn = L.x265amd_sao_rdo_opt
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    p = lambda x: x.ctypes.data
    base = (p(si), 1, 1, 0, 69, p(units), p(cnt), p(org), p(rate), p(par), p(flags))
    assert fn(*base, S.NON_DEBLOCK, 0, None, None) != 0
    assert fn(*base, S.NON_DEBLOCK, 0, p(cnt), None) != 0
    assert fn(*base, 0, 0, p(cnt), p(org)) != 0
    assert fn(*base, 8, 0, None, None) != 0


def test_layout_of_the_extension_record_and_of_bLimitSAO():
    """tests/native/abi_layout_sao_check.cpp: x265amd_param_ext as the ctypes mirror has it and -- where the reference's headers are built -- the offset of bLimitSAO"""
    assert C.sizeof(S.ParamExt) == 64 and S.ParamExt.bSaoNonDeblocked.offset == 4 and S.ParamExt.bLimitSAO.offset == 8 and S.ParamExt.selectiveSAO.offset == 12
    assert S.ParamExt.reserved.offset == 16
    ref_src = os.path.join(T.REF_DIR, "include")
    cmd = ["g++", "-std=gnu++11", "-fsyntax-only", "-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.PKG_DIR, "host")]
    if os.path.isdir(ref_src):
        cmd += ["-DWITH_REFERENCE_HEADER", "-I" + os.path.join(T.REF_DIR, "cfg"), "-I" + ref_src]
    r = subprocess.run(cmd + [os.path.join(T.ROOT, "tests", "native", "abi_layout_sao_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _sao_layout():
    import test_x265_api_abi as A
    for line in open(os.path.join(T.PKG_DIR, "host", "x265_abi_layout_sao.h")):
        if line.startswith("#define X265ABI_PARAM_bLimitSAO"):
            return {"bLimitSAO": int(line.split()[2]), "bSaoNonDeblocked": A.LAYOUT["PARAM_bSaoNonDeblocked"], "selectiveSAO": A.LAYOUT["PARAM_selectiveSAO"]}
    raise AssertionError("x265_abi_layout_sao.h: no offset")


def _i32(p, off):
    return int.from_bytes(bytes((C.c_ubyte * 4).from_address(p + off)), "little", signed=True)


@pytest.mark.parametrize("depth", [8, 10])
def test_param_parse_knows_the_three_options(depth):
    import test_x265_api_abi as A
    off = _sao_layout()
    f = A._fns(A.table(depth), depth)
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0
    assert [_i32(p, off[k]) for k in ("bSaoNonDeblocked", "bLimitSAO", "selectiveSAO")] == [0, 0, 0]           # param.cpp:241-243
    assert f["parse"](p, b"sao-non-deblock", None) == 0 and f["parse"](p, b"limit-sao", b"1") == 0 and f["parse"](p, b"selective-sao", b"3") == 0
    assert [_i32(p, off[k]) for k in ("bSaoNonDeblocked", "bLimitSAO", "selectiveSAO")] == [1, 1, 3]
    assert f["parse"](p, b"no-sao-non-deblock", None) == 0 and f["parse"](p, b"no-limit-sao", None) == 0
    assert [_i32(p, off[k]) for k in ("bSaoNonDeblocked", "bLimitSAO", "selectiveSAO")] == [0, 0, 3]
    assert f["parse"](p, b"no-selective-sao", None) != 0 and f["parse"](p, b"selective-sao", b"x") != 0
    f["free"](p)


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref (the reference build) is not present")
def test_param_parse_of_the_three_options_matches_the_references():
    """x265_param_parse through our table against the reference library's own: the same return code, the same three members (bLimitSAO is not among the generated
    layout's members: read at its own offset), the same other members"""
    import test_x265_api_abi as A
    R, f = A._reference_api(), A._fns(A.table(8))
    off = _sao_layout()
    three = lambda p: [_i32(p, off[k]) for k in ("bSaoNonDeblocked", "bLimitSAO", "selectiveSAO")]
    a, b = R.x265_param_alloc(), f["alloc"]()
    R.x265_param_default_preset(a, b"medium", None); f["preset"](b, b"medium", None)
    assert three(a) == three(b) == [0, 0, 0]
    steps = [(b"sao-non-deblock", None), (b"limit-sao", None), (b"selective-sao", b"2"), (b"no-sao-non-deblock", None), (b"sao-non-deblock", b"1"), (b"limit-sao", b"0"),
             (b"no-limit-sao", b"0"), (b"selective-sao", b"0"), (b"selective-sao", b"4"), (b"selective-sao", b"7"), (b"selective-sao", b"x"), (b"selective-sao", None),
             (b"limit-sao", b"maybe"), (b"no-sao", None), (b"selective-sao", b"1")]
    for name, value in steps:
        ra, rb = R.x265_param_parse(a, name, value), f["parse"](b, name, value)
        assert ra == rb, (name, value, ra, rb)
        assert three(a) == three(b), (name, value, three(a), three(b))
        assert A._members(a) == A._members(b), (name, value)
    R.x265_param_free(a); f["free"](b)
