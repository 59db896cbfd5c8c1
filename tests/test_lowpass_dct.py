"""The low-pass approximation of the forward transform (--lowpass-dct; reference: source/common/lowpassdct.cpp:34-112) below the encoder: x265amd_lowpass_dct and the
job op X265AMD_OP_LOWPASS_DCT against the reference's own cu[].lowpass_dct outputs (tests/golden/lowpass_dct_golden.npz, cut by tests/golden/make_lowpass_dct_golden.py,
which asserts every one of them against a numpy restatement over the reference's transform of half the size); without a GPU: the fixtures, the layout check and
x265_param_parse."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import hevc_testlib as T
import lowpass_dct_lib as LP


def _golden():
    return np.load(LP.GOLDEN)


def test_fixtures_present_and_complete():
    g = _golden()
    for depth in (8, 10):
        inputs = LP.prim_inputs(depth)
        assert {cu for _, cu, _, _ in inputs} == {1, 2, 3}
        for name, cu, stride, src in inputs:
            N = 4 << cu
            k = LP.prim_key(depth, name, cu)
            assert np.array_equal(g[k + "/in"], src) and g[k + "/out"].shape == (N * N,) and g[k + "/out"].dtype == np.int16, k
            out = g[k + "/out"].reshape(N, N)
            assert not out[N // 2:, :].any() and not out[:, N // 2:].any(), k          # everything outside the top-left quadrant is zero
        for name, n in (("inter", 40), ("intra", 21), ("intra_rdoq", 28)):
            assert g["%s%d/stats" % (name, depth)].shape == (n, 5), name
    # the numbers the wraps come to (10 bits; 8 bits never wraps: 256 * 255 >> 1 = 32640)
    for cu in (1, 2, 3):
        assert g[LP.prim_key(10, "pos_max", cu) + "/out"][0] == -128 and g[LP.prim_key(10, "neg_max", cu) + "/out"][0] == 128
    assert g[LP.prim_key(10, "mean256", 2) + "/out"][0] == -32768 and g[LP.prim_key(10, "mean256_less", 2) + "/out"][0] == 32767
    assert g[LP.prim_key(8, "pos_max", 2) + "/out"][0] == 32640
    # the floors: a total of -1, -2, -3 through `>> 1` (16x16) and `>> 3` (32x32), and `<< 1` of the 8x8 form
    for depth in (8, 10):
        assert [int(g[LP.prim_key(depth, "total_m%d" % v, 2) + "/out"][0]) for v in (1, 2, 3)] == [-1, -1, -2]
        assert [int(g[LP.prim_key(depth, "total_m%d" % v, 3) + "/out"][0]) for v in (1, 2, 3)] == [-1, -1, -1]
        assert [int(g[LP.prim_key(depth, "total_m%d" % v, 1) + "/out"][0]) for v in (1, 2, 3)] == [-2, -4, -6]
    e = json.load(open(os.path.join(T.GOLDEN_DIR, "encoder_lowpass_dct_golden.json")))
    assert len(e) == 10


def test_the_restatement_over_the_oracle_transform_gives_the_fixtures():
    """lowpass_dct_lib.lowpass_model over the C oracle's standard transform of half the size: the reference's outputs"""
    g = _golden()
    for depth in (8, 10):
        O = T.load_oracle(depth)

        def half(cu):
            def f(avg):
                d = np.zeros(avg.shape, np.int16)
                O.call("dct", cu - 1, avg, d, avg.shape[1])
                return d
            return f
        for name, cu, stride, src in LP.prim_inputs(depth):
            N = 4 << cu
            assert np.array_equal(LP.lowpass_model(src, cu, half(cu)).ravel(), g[LP.prim_key(depth, name, cu) + "/out"]), (depth, name, cu)


def test_layout_of_the_tools_record_and_of_bLowPassDct():
    """tests/native/abi_layout_lowpass_check.cpp: x265amd_param_tools, the flags byte and the op number and -- where the reference's headers are built -- the offset
    of x265_param.bLowPassDct"""
    ref_src = os.path.join(T.REF_DIR, "include")
    cmd = ["g++", "-std=gnu++11", "-fsyntax-only", "-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.PKG_DIR, "host")]
    if os.path.isdir(ref_src):
        cmd += ["-DWITH_REFERENCE_HEADER", "-I" + os.path.join(T.REF_DIR, "cfg"), "-I" + ref_src]
    r = subprocess.run(cmd + [os.path.join(T.ROOT, "tests", "native", "abi_layout_lowpass_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _i32(p, off):
    return int.from_bytes(bytes((C.c_ubyte * 4).from_address(p + off)), "little", signed=True)


@pytest.mark.parametrize("depth", [8, 10])
def test_param_parse_knows_the_option(depth):
    """x265_param_parse("lowpass-dct") / ("no-lowpass-dct") set the member at the pinned offset (param.cpp:1322, atobool)"""
    import test_x265_api_abi as A
    off = A.LAYOUT["PARAM_bLowPassDct"]
    f = A._fns(A.table(depth), depth)
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0
    assert _i32(p, off) == 0
    assert f["parse"](p, b"lowpass-dct", None) == 0 and _i32(p, off) == 1
    assert f["parse"](p, b"no-lowpass-dct", None) == 0 and _i32(p, off) == 0
    assert f["parse"](p, b"lowpass-dct", b"1") == 0 and _i32(p, off) == 1
    assert f["parse"](p, b"lowpass-dct", b"0") == 0 and _i32(p, off) == 0
    assert f["parse"](p, b"lowpass-dct", b"maybe") != 0
    f["free"](p)


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref (the reference build) is not present")
def test_param_parse_of_the_option_matches_the_references():
    import test_x265_api_abi as A
    R, f = A._reference_api(), A._fns(A.table(8))
    off = A.LAYOUT["PARAM_bLowPassDct"]
    a, b = R.x265_param_alloc(), f["alloc"]()
    R.x265_param_default_preset(a, b"medium", None); f["preset"](b, b"medium", None)
    for name, value in ((b"lowpass-dct", None), (b"no-lowpass-dct", None), (b"lowpass-dct", b"1"), (b"lowpass-dct", b"false"), (b"no-lowpass-dct", b"0"), (b"lowpass-dct", b"maybe")):
        ra, rb = R.x265_param_parse(a, name, value), f["parse"](b, name, value)
        assert ra == rb and _i32(a, off) == _i32(b, off), (name, value, ra, rb, _i32(a, off), _i32(b, off))
        assert A._members(a) == A._members(b), (name, value)
    R.x265_param_free(a); f["free"](b)


# ---- on the GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_the_plain_entry(depth):
    """x265amd_lowpass_dct(cu, src, dst, srcStride), cu 1..3, bit for bit"""
    g = _golden()
    L = T.load_hip(depth)
    L.lib.x265amd_lowpass_dct.restype = None
    for name, cu, stride, src in LP.prim_inputs(depth):
        N = 4 << cu
        dst = np.full(N * N, 0x55AA, np.uint16).view(np.int16)
        L.lib.x265amd_lowpass_dct(cu, T._ptr(np.ascontiguousarray(src)), T._ptr(dst), C.c_int64(stride))
        want = g[LP.prim_key(depth, name, cu) + "/out"]
        assert np.array_equal(dst, want), "%s cu %d: first difference at %d" % (name, cu, int(np.flatnonzero(dst != want)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_the_job_op_mixed_with_standard_transforms(depth):
    """one x265amd_run_jobs launch of family 2: every low-pass case as an X265AMD_OP_LOWPASS_DCT job, standard DCT jobs of the same blocks between them (more than one
    workgroup; neighbouring wavefronts of a workgroup hold different ops and sizes); every output block right, the guard words round them untouched"""
    import torch
    g = _golden()
    L, O = T.load_hip(depth), T.load_oracle(depth)
    inputs = LP.prim_inputs(depth)
    specs = []          # (op, cu, input index)
    for i, (name, cu, stride, src) in enumerate(inputs):
        specs.append((LP.OP_LOWPASS_DCT, cu, i))
        if i % 2 == 0:
            specs.append((T.JOB_OPS["DCT"], cu, i))
    assert len(specs) > 8
    in_off, o = [], 0
    for name, cu, stride, src in inputs:
        in_off.append(o)
        o += src.size
    inb = np.concatenate([src.ravel() for _, _, _, src in inputs])
    GUARD = 16
    out_off, o = [], GUARD
    for op, cu, i in specs:
        out_off.append(o)
        o += (4 << cu) ** 2 + GUARD
    outb = np.full(o, 0x7A7A, np.int16)
    d_in, d_out = torch.from_numpy(inb).cuda(), torch.from_numpy(outb.copy()).cuda()
    recs = np.zeros(len(specs), T.JOB_DT)
    want = outb.copy()
    for k, (op, cu, i) in enumerate(specs):
        name, _, stride, src = inputs[i]
        N = 4 << cu
        recs[k]["op"], recs[k]["size"], recs[k]["sa"] = op, cu, stride
        recs[k]["a"], recs[k]["d"] = d_in.data_ptr() + 2 * in_off[i], d_out.data_ptr() + 2 * out_off[k]
        if op == LP.OP_LOWPASS_DCT:
            want[out_off[k]:out_off[k] + N * N] = g[LP.prim_key(depth, name, cu) + "/out"]
        else:
            d = np.zeros(N * N, np.int16)
            O.call("dct", cu, np.ascontiguousarray(src), d, stride)
            want[out_off[k]:out_off[k] + N * N] = d
    d_jobs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    assert L.lib.x265amd_run_jobs(None, C.c_void_p(d_jobs.data_ptr()), len(specs), 2) == 0
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    for k, (op, cu, i) in enumerate(specs):
        N = 4 << cu
        assert np.array_equal(got[out_off[k]:out_off[k] + N * N], want[out_off[k]:out_off[k] + N * N]), "job %d (op %d, %s, cu %d)" % (k, op, inputs[i][0], cu)
    assert np.array_equal(got, want), "a guard word between the blocks changed"
    assert np.array_equal(d_in.cpu().numpy(), inb), "the inputs changed"


@pytest.mark.gpu
def test_a_job_of_a_size_without_a_low_pass_form_writes_nothing():
    import torch
    L = T.load_hip(8)
    src = torch.ones(64 * 64, dtype=torch.int16, device="cuda")
    dst = torch.full((64 * 64 + 32,), 0x1234, dtype=torch.int16, device="cuda")
    recs = np.zeros(2, T.JOB_DT)
    for k, size in enumerate((0, 4)):
        recs[k]["op"], recs[k]["size"], recs[k]["sa"], recs[k]["a"], recs[k]["d"] = LP.OP_LOWPASS_DCT, size, 64, src.data_ptr(), dst.data_ptr()
    d_jobs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    assert L.lib.x265amd_run_jobs(None, C.c_void_p(d_jobs.data_ptr()), 2, 2) == 0
    torch.cuda.synchronize()
    assert bool((dst == 0x1234).all())
