"""The picture ingest pass on the device (csrc/ingest_kernels.hip: x265amd_ingest_picture) against its host model (x265amd_ingest_model, tests/test_ingest.py) over the
whole flat picture buffer, and -- for same-depth planar pictures -- against what the encoder's existing device path leaves (a 2-D copy and x265amd_extend_pic_border twice
per plane over a zeroed buffer).  The buffer is pre-filled with 0xA5, so a byte the pass does not write fails; a guard behind every source plane and around the destination
has to stay as it was."""
import ctypes as C

import numpy as np
import pytest

import hevc_testlib as T
import test_ingest as TI

pytestmark = pytest.mark.gpu

GUARD = 256          # bytes
GUARD_BYTE = 0x5C
ENCODER_MARGINS = (96, 80)


def _device_source(raw):
    """every stored plane in an allocation of its own with a guard behind it: (tensors, device addresses)"""
    import torch
    tensors = [torch.from_numpy(np.concatenate([buf, np.full(GUARD, GUARD_BYTE, np.uint8)])).cuda() for buf, _, _ in raw]
    return tensors, [t.data_ptr() for t in tensors]


def run_device(lib_depth, raw, depth, layout, clip, sw, sh, W, H, mx, my, stream=None):
    """x265amd_ingest_picture on device copies of the planes; returns the flat buffer.  Guards are checked here"""
    import torch
    lib = T.load_hip(lib_depth).lib
    lib.x265amd_ingest_picture.argtypes = [C.c_void_p, C.POINTER(TI.Surface), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.x265amd_last_error.restype = C.c_char_p
    isz = 1 if lib_depth == 8 else 2
    total = TI.geometry(W, H, mx, my)["total"] * isz
    tensors, addr = _device_source(raw)
    dst = torch.full((GUARD + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dst[:GUARD] = GUARD_BYTE
    dst[GUARD + total:] = GUARD_BYTE
    torch.cuda.synchronize()
    s = TI.surface_of(raw, depth, layout, clip, addr=addr)
    handle = C.c_void_p(stream.cuda_stream) if stream is not None else None
    assert lib.x265amd_ingest_picture(handle, C.byref(s), sw, sh, C.c_void_p(dst.data_ptr() + GUARD), W, H, mx, my) == 0, lib.x265amd_last_error()
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[:GUARD] == GUARD_BYTE).all() and (out[GUARD + total:] == GUARD_BYTE).all(), "the guards around the destination"
    for t, (buf, _, _) in zip(tensors, raw):
        back = t.cpu().numpy()
        assert (back[len(buf):] == GUARD_BYTE).all() and np.array_equal(back[:len(buf)], buf), "a source plane or the guard behind it"
    return out[GUARD:GUARD + total].view(np.uint8 if lib_depth == 8 else np.uint16)


def compare_with_model(lib_depth, seed, shape, depth, layout, stride_kind, clip, margins, lead=0, stream=None):
    sw, sh, W, H = shape
    mx, my = margins
    planes, raw = TI.make_source(seed, sw, sh, depth, layout, stride_kind, lead=lead)
    rc, want, err = TI.run_model(lib_depth, TI.surface_of(raw, depth, layout, clip), sw, sh, W, H, mx, my)
    assert rc == 0, err
    got = run_device(lib_depth, raw, depth, layout, clip, sw, sh, W, H, mx, my, stream)
    assert np.array_equal(got, want), (shape, depth, layout, stride_kind, clip, margins, lead, np.flatnonzero(got != want)[:8])
    return want


@pytest.mark.parametrize("lib_depth", [8, 10])
def test_device_pass_equals_the_model(lib_depth):
    """the matrix of tests/test_ingest.py: every shape, picture depth and layout, the three stride kinds, the luma bounds on and off"""
    for n, (shape, depth, layout, stride_kind, clip_on) in enumerate(TI.matrix()):
        compare_with_model(lib_depth, 2000 + n, shape, depth, layout, stride_kind, TI.clip_bounds(lib_depth, clip_on), TI.MARGINS)


@pytest.mark.parametrize("lib_depth", [8, 10])
@pytest.mark.parametrize("depth", TI.PIC_DEPTHS)
@pytest.mark.parametrize("layout", [0, 1])
def test_the_encoders_own_margins(lib_depth, depth, layout):
    """200x152 with margins of 96 / 80: rows of more than one block of lanes, several blocks of rows; and 198x150 padded to it"""
    compare_with_model(lib_depth, 31, (200, 152, 200, 152), depth, layout, "w+6", TI.clip_bounds(lib_depth, layout == 1), ENCODER_MARGINS)
    compare_with_model(lib_depth, 32, (198, 150, 200, 152), depth, layout, "w", TI.clip_bounds(lib_depth, layout == 0), ENCODER_MARGINS)


@pytest.mark.parametrize("lib_depth", [8, 10])
@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("layout", [0, 1])
def test_planes_at_odd_element_offsets(lib_depth, depth, layout):
    """the planes start 1 and 3 elements into their allocations: no source run is aligned to a vector load, and with margins of 5 / 3 no destination row to a vector store
    (odd margins: the chroma planes keep a column and a row outside the padded area, which must be zero)"""
    for lead in (1, 3):
        compare_with_model(lib_depth, 40 + lead, (70, 38, 72, 40), depth, layout, "w+6", (-1, -1), (8, 4), lead=lead)
    want = compare_with_model(lib_depth, 44, (70, 38, 72, 40), depth, layout, "w", (-1, -1), (5, 3), lead=1)
    g = TI.geometry(72, 40, 5, 3)
    chroma = want[g["ysz"]:g["ysz"] + g["csz"]].reshape(-1, g["cstride"])
    assert (chroma[:, -1] == 0).all() and (chroma[-1] == 0).all() and chroma[:-1, :-1].any()


@pytest.mark.parametrize("lib_depth", [8, 10])
def test_on_a_stream_of_its_own(lib_depth):
    import torch
    st = torch.cuda.Stream()
    for depth, layout in ((8, 1), (16, 1), (10, 0)):
        compare_with_model(lib_depth, 60 + depth, (198, 150, 200, 152), depth, layout, "3w", TI.clip_bounds(lib_depth, True), ENCODER_MARGINS, stream=st)


@pytest.mark.parametrize("lib_depth", [8, 10])
@pytest.mark.parametrize("size", [(200, 152), (198, 150)])
def test_same_depth_planar_is_the_existing_device_path(lib_depth, size):
    """what x265amd_encoder::uploadPicture(onDevice) leaves in Pic::dSrc, built from the same calls: a zeroed buffer, per plane a 2-D copy, the pad up to the coded size
    with x265amd_extend_pic_border (when there is one) and the margins with it again"""
    import torch
    sw, sh = size
    W, H = (sw + 7) & ~7, (sh + 7) & ~7
    mx, my = ENCODER_MARGINS
    planes, raw = TI.make_source(70, sw, sh, lib_depth, 0, "w", in_range=True)
    got = run_device(lib_depth, raw, lib_depth, 0, (-1, -1), sw, sh, W, H, mx, my)
    lib = T.load_hip(lib_depth).lib
    lib.x265amd_extend_pic_border.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    g = TI.geometry(W, H, mx, my)
    isz = 1 if lib_depth == 8 else 2
    dt = torch.uint8 if lib_depth == 8 else torch.int16
    buf = torch.zeros(g["total"], dtype=dt, device="cuda")
    for k, pl in enumerate(planes):
        w, h, pmx, pmy, st = (W >> (k > 0)), (H >> (k > 0)), (mx >> (k > 0)), (my >> (k > 0)), (g["cstride"] if k else g["stride"])
        psw, psh = pl.shape[1], pl.shape[0]
        rows = buf[g["org"][k] - pmx:g["org"][k] - pmx + h * st].view(h, st)
        rows[:psh, pmx:pmx + psw] = torch.from_numpy(pl.astype(np.uint8) if lib_depth == 8 else pl.view(np.int16)).cuda()
        torch.cuda.synchronize()
        org = C.c_void_p(buf.data_ptr() + g["org"][k] * isz)
        if (psw, psh) != (w, h):
            assert lib.x265amd_extend_pic_border(None, org, st, psw, psh, w - psw, h - psh) == 0
        assert lib.x265amd_extend_pic_border(None, org, st, w, h, pmx, pmy) == 0
    torch.cuda.synchronize()
    want = buf.cpu().numpy().view(np.uint8 if lib_depth == 8 else np.uint16)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_refusals_launch_nothing():
    """the refusals of tests/test_ingest.py come from the same check in front of the launch: one of them here, on device memory, and the destination keeps its fill"""
    import torch
    lib = T.load_hip(8).lib
    lib.x265amd_ingest_picture.argtypes = [C.c_void_p, C.POINTER(TI.Surface), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.x265amd_last_error.restype = C.c_char_p
    (sw, sh, W, H), (mx, my) = TI.SHAPES[0], TI.MARGINS
    planes, raw = TI.make_source(5, sw, sh, 8, 0, "w")
    tensors, addr = _device_source(raw)
    dst = torch.full((TI.geometry(W, H, mx, my)["total"],), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for depth, word in ((7, b"bitDepth"), (17, b"bitDepth")):
        s = TI.surface_of(raw, depth, 0, addr=addr)
        assert lib.x265amd_ingest_picture(None, C.byref(s), sw, sh, C.c_void_p(dst.data_ptr()), W, H, mx, my) != 0 and word in lib.x265amd_last_error()
    s = TI.surface_of(raw, 8, 0, addr=addr)
    assert lib.x265amd_ingest_picture(None, C.byref(s), sw, sh, C.c_void_p(dst.data_ptr()), W - 8, H, mx, my) != 0 and b"srcW" in lib.x265amd_last_error()
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all()
