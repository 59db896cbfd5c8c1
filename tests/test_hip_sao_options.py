"""The statistics kernels of the SAO options on the GPU: k_sao_stats in its compile-time forms (x265amd_sao_stats_opt: the --sao-non-deblock skips, no EO_2 / EO_3 for
B pictures under --limit-sao) and k_sao_stats_pre (x265amd_sao_stats_pre: SAO::calcSaoStatsCu_BeforeDblk) against the host model (x265amd_sao_stats_model), word for
word, 8 and 10 bits.  tests/test_sao_options.py compares that model with a line-by-line restatement of the reference's functions.

Shapes (tests/sao_options_lib.py): one CTU at the right and bottom edge at once; no partial CTU; a last column and row of 8; of 8 and 24.  Contents: LCG noise with
an independent field before deblocking (a kernel reading the wrong planes shows), flat, a min / max checkerboard (the largest sums), ramps along both axes and both
diagonals (ties).  Every plane lies at its exact size between guard rows that must come back untouched; the row and column forms must give the full picture's words for
their CTUs and leave a guard pattern in every other word."""
import ctypes as C
import functools

import numpy as np
import pytest

import hevc_testlib as T
import sao_options_lib as S

pytestmark = pytest.mark.gpu
GUARD_ROWS = 3
GUARD_WORD = -0x5a5a5a5


def _guarded(planes, depth):
    """device copies of the planes, each between GUARD_ROWS rows of alternating 0 / largest sample on either side; (tensors, host images, table of sample (0,0))"""
    import torch
    pmax = (1 << depth) - 1
    tensors, images, ptrs = [], [], []
    for p in planes:
        h, w = p.shape
        full = np.empty((h + 2 * GUARD_ROWS, w), p.dtype)
        full[:] = np.where(np.arange(w) & 1, pmax, 0).astype(p.dtype)
        full[GUARD_ROWS:GUARD_ROWS + h] = p
        t = torch.from_numpy(full.view(np.uint8).copy()).cuda()
        tensors.append(t); images.append(full); ptrs.append(t.data_ptr() + GUARD_ROWS * w * p.itemsize)
    return tensors, images, np.array(ptrs, np.uint64)


def _untouched(tensors, images):
    return all(np.array_equal(t.cpu().numpy(), im.view(np.uint8)) for t, im in zip(tensors, images))


def _lib(depth):
    lib = T.load_hip(depth).lib
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    lib.x265amd_sao_stats_opt.argtypes = [P, P, P, L, L, I, I, P, P, I]
    lib.x265amd_sao_stats_opt_rows.argtypes = [P, P, P, L, L, I, I, P, P, I, I, I]
    lib.x265amd_sao_stats_opt_rows_cols.argtypes = [P, P, P, L, L, I, I, P, P, I, I, I, I, I]
    lib.x265amd_sao_stats_pre.argtypes = [P, P, P, L, L, I, I, P, P]
    lib.x265amd_sao_stats_pre_rows.argtypes = [P, P, P, L, L, I, I, P, P, I, I]
    return lib


@functools.lru_cache(maxsize=None)
def _reference(content, w, h, depth, flags):
    rec, fenc, pre = S.plane_set(content, w, h, depth)
    return S.model(T.load_hip(depth).lib, rec, fenc, pre, w, h, flags, want_pre=True)


def _words(w, h):
    import torch
    n = S.nctu(w, h) * 3 * S.WORDS
    return torch.full((n,), GUARD_WORD, dtype=torch.int32, device="cuda"), torch.full((n,), GUARD_WORD, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", S.SHAPES)
def test_every_form_equals_the_model(depth, w, h):
    import torch
    lib = _lib(depth)
    for content in S.CONTENTS:
        rec, fenc, pre = S.plane_set(content, w, h, depth)
        d_rec, i_rec, t_rec = _guarded(rec, depth); d_fenc, i_fenc, t_fenc = _guarded(fenc, depth); d_pre, i_pre, t_pre = _guarded(pre, depth)
        if content == "noise":
            # the condition that keeps this test from passing on empty classes (the one-CTU picture's pre-deblock record is all zero in the reference itself)
            m = _reference(content, w, h, depth, S.NON_DEBLOCK)
            assert S.classes_covered(m["count"])
            assert S.classes_covered(m["pre_count"]) if (w, h) != (64, 64) else not m["pre_count"].any()
        for flags in (0, S.NON_DEBLOCK, S.EO01_ONLY, S.NON_DEBLOCK | S.EO01_ONLY):
            want = _reference(content, w, h, depth, flags)
            cnt, org = _words(w, h)
            assert lib.x265amd_sao_stats_opt(None, T._ptr(t_rec), T._ptr(t_fenc), w, w // 2, w, h, cnt.data_ptr(), org.data_ptr(), flags) == 0
            torch.cuda.synchronize()
            assert np.array_equal(cnt.cpu().numpy(), want["count"]) and np.array_equal(org.cpu().numpy(), want["org"]), (content, flags)
        want = _reference(content, w, h, depth, 0)
        cnt, org = _words(w, h)
        assert lib.x265amd_sao_stats_pre(None, T._ptr(t_pre), T._ptr(t_fenc), w, w // 2, w, h, cnt.data_ptr(), org.data_ptr()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy(), want["pre_count"]) and np.array_equal(org.cpu().numpy(), want["pre_org"]), content
        assert _untouched(d_rec, i_rec) and _untouched(d_fenc, i_fenc) and _untouched(d_pre, i_pre), content


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", S.SHAPES[1:])
def test_row_and_column_forms_give_the_pictures_words_and_nothing_else(depth, w, h):
    import torch
    lib = _lib(depth)
    ctu_w, ctu_h = (w + 63) // 64, (h + 63) // 64
    rec, fenc, pre = S.plane_set("noise", w, h, depth)
    d_rec, i_rec, t_rec = _guarded(rec, depth); d_fenc, i_fenc, t_fenc = _guarded(fenc, depth); d_pre, i_pre, t_pre = _guarded(pre, depth)

    def check(got_c, got_o, want_c, want_o, rows, cols, what):
        gc, go = got_c.cpu().numpy().reshape(ctu_h, ctu_w, -1), got_o.cpu().numpy().reshape(ctu_h, ctu_w, -1)
        wc, wo = want_c.reshape(ctu_h, ctu_w, -1), want_o.reshape(ctu_h, ctu_w, -1)
        inside = np.zeros((ctu_h, ctu_w), bool); inside[rows[0]:rows[1], cols[0]:cols[1]] = True
        assert np.array_equal(gc[inside], wc[inside]) and np.array_equal(go[inside], wo[inside]), what
        assert (gc[~inside] == GUARD_WORD).all() and (go[~inside] == GUARD_WORD).all(), what

    last_row, last_col = (ctu_h - 1, ctu_h), (ctu_w - 1, ctu_w)
    for flags in (S.NON_DEBLOCK, S.EO01_ONLY, S.NON_DEBLOCK | S.EO01_ONLY):
        want = _reference("noise", w, h, depth, flags)
        for rows in ((0, 1), last_row):
            cnt, org = _words(w, h)
            assert lib.x265amd_sao_stats_opt_rows(None, T._ptr(t_rec), T._ptr(t_fenc), w, w // 2, w, h, cnt.data_ptr(), org.data_ptr(), flags, rows[0], rows[1]) == 0
            torch.cuda.synchronize()
            check(cnt, org, want["count"], want["org"], rows, (0, ctu_w), ("rows", flags, rows))
            for cols in ((0, 1), last_col):
                cnt, org = _words(w, h)
                assert lib.x265amd_sao_stats_opt_rows_cols(None, T._ptr(t_rec), T._ptr(t_fenc), w, w // 2, w, h, cnt.data_ptr(), org.data_ptr(), flags, rows[0], rows[1], cols[0], cols[1]) == 0
                torch.cuda.synchronize()
                check(cnt, org, want["count"], want["org"], rows, cols, ("rows_cols", flags, rows, cols))
    want = _reference("noise", w, h, depth, 0)
    for rows in ((0, 1), last_row):
        cnt, org = _words(w, h)
        assert lib.x265amd_sao_stats_pre_rows(None, T._ptr(t_pre), T._ptr(t_fenc), w, w // 2, w, h, cnt.data_ptr(), org.data_ptr(), rows[0], rows[1]) == 0
        torch.cuda.synchronize()
        check(cnt, org, want["pre_count"], want["pre_org"], rows, (0, ctu_w), ("pre rows", rows))
    assert _untouched(d_rec, i_rec) and _untouched(d_fenc, i_fenc) and _untouched(d_pre, i_pre)


def test_flags_and_null_pointers_are_refused():
    import torch
    lib = _lib(8)
    rec, fenc, pre = S.plane_set("flat", 64, 64, 8)
    d_rec, _, t_rec = _guarded(rec, 8); d_fenc, _, t_fenc = _guarded(fenc, 8)
    cnt, org = _words(64, 64)
    args = (None, T._ptr(t_rec), T._ptr(t_fenc), 64, 32, 64, 64, cnt.data_ptr(), org.data_ptr())
    assert lib.x265amd_sao_stats_opt(*args, 4) != 0 and lib.x265amd_sao_stats_opt(*args, -1) != 0
    assert lib.x265amd_sao_stats_opt(None, None, T._ptr(t_fenc), 64, 32, 64, 64, cnt.data_ptr(), org.data_ptr(), 1) != 0
    assert lib.x265amd_sao_stats_opt(None, T._ptr(t_rec), T._ptr(t_fenc), 64, 32, 64, 64, None, org.data_ptr(), 1) != 0
    assert lib.x265amd_sao_stats_opt_rows(*args, 1, 0, 2) != 0 and lib.x265amd_sao_stats_opt_rows_cols(*args, 1, 0, 1, 1, 1) != 0
    assert lib.x265amd_sao_stats_pre(None, T._ptr(t_rec), None, 64, 32, 64, 64, cnt.data_ptr(), org.data_ptr()) != 0
    assert lib.x265amd_sao_stats_pre(None, T._ptr(t_rec), T._ptr(t_fenc), 64, 32, 64, 64, cnt.data_ptr(), None) != 0
    assert lib.x265amd_sao_stats_pre_rows(*args, 1, 1) != 0 and lib.x265amd_sao_stats_pre_rows(*args, 0, 2) != 0
    torch.cuda.synchronize()
    assert (cnt.cpu().numpy() == GUARD_WORD).all() and (org.cpu().numpy() == GUARD_WORD).all()         # a refused call launches nothing
