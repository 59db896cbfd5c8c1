"""Picture ingest without a GPU: x265amd_ingest_model, the host model of the one-launch pass that turns a caller's surface -- any depth from 8 to 16
bits, planar or semi-planar -- into the padded source picture, against a numpy restatement of PicYuv::copyFromPicture's conversion table; its refusals; the reference ABI's
x265_dither_image against the reference library's own (tests/golden/ingest_golden.npz, cut by tests/golden/make_ingest_golden.py); min-luma / max-luma in x265_param_parse
and the picture forms x265_encoder_encode takes.  tests/test_hip_ingest.py compares the device pass with this model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hevc_testlib as T
import test_x265_api_abi as A

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "ingest_golden.npz")


class Surface(C.Structure):         # x265amd_surface (include/x265amd.h; tests/native/abi_layout_ingest_check.cpp pins the layout)
    _fields_ = [("planes", C.c_void_p * 3), ("stride", C.c_int32 * 3), ("bitDepth", C.c_int32), ("layout", C.c_int32), ("clipMin", C.c_int32), ("clipMax", C.c_int32),
                ("reserved", C.c_int32)]


# (srcW, srcH, W, H): a pad in both directions, no pad, the smallest picture
SHAPES = [(18, 10, 24, 16), (16, 16, 16, 16), (2, 2, 8, 8)]
MARGINS = (8, 4)
STRIDES = ("w", "w+6", "3w")
PIC_DEPTHS = (8, 10, 12, 16)


def geometry(W, H, mx, my):
    """the flat Y | U | V buffer of the encoder (csrc/encoder_api.hip: x265amd_encoder_open): strides, plane sizes and the picture origins, in elements"""
    stride, cstride = W + 2 * mx, W // 2 + mx
    ysz, csz = (H + 2 * my) * stride, (H // 2 + my) * cstride
    org = (my * stride + mx, ysz + (my // 2) * cstride + mx // 2, ysz + csz + (my // 2) * cstride + mx // 2)
    return dict(stride=stride, cstride=cstride, ysz=ysz, csz=csz, org=org, total=ysz + 2 * csz)


def make_source(seed, sw, sh, depth, layout, stride_kind, in_range=False, lead=0):
    """a surface in host memory.  Samples use every bit of their words (8 or 16) unless in_range.  Returns the logical planes (uint16 Y, U, V as the words were read) and
    the raw byte buffers [(bytes, offset of the plane's first sample, stride)] per stored plane; lead: elements in front of each plane inside its buffer"""
    rng = np.random.default_rng(seed)
    isz = 2 if depth > 8 else 1
    top = (1 << depth) if in_range else (1 << (8 * isz))
    planes = [rng.integers(0, top, (sh, sw)).astype(np.uint16), rng.integers(0, top, (sh // 2, sw // 2)).astype(np.uint16), rng.integers(0, top, (sh // 2, sw // 2)).astype(np.uint16)]
    stored = [planes[0], np.stack([planes[1], planes[2]], axis=2).reshape(sh // 2, sw)] if layout else planes
    raw = []
    for pl in stored:
        row_bytes = pl.shape[1] * isz
        stride = {"w": row_bytes, "w+6": row_bytes + 6, "3w": 3 * row_bytes}[stride_kind]
        buf = rng.integers(0, 256, lead * isz + stride * pl.shape[0] + 16).astype(np.uint8)          # (garbage between the rows and behind the last)
        for y in range(pl.shape[0]):
            buf[lead * isz + y * stride:lead * isz + y * stride + row_bytes] = pl[y].astype(np.uint16 if isz == 2 else np.uint8).view(np.uint8)
        raw.append((buf, lead * isz, stride))
    return planes, raw


def surface_of(raw, depth, layout, clip=(-1, -1), addr=None):
    s = Surface()
    for k, (buf, at, stride) in enumerate(raw):
        s.planes[k] = (addr[k] if addr else buf.ctypes.data) + at
        s.stride[k] = stride
    s.bitDepth, s.layout, s.clipMin, s.clipMax = depth, layout, clip[0], clip[1]
    return s


def conv(v, depth, lib_depth):
    """the conversion table of PicYuv::copyFromPicture (picyuv.cpp:298-396), on uint32 arrays"""
    v = v.astype(np.uint32)
    mask = (1 << lib_depth) - 1
    if depth == 8:
        return v << (lib_depth - 8) if lib_depth > 8 else v          # planecopy_cp: no mask (an 8-bit word shifted by 2 cannot pass 10 bits: masked and unmasked agree)
    if depth > lib_depth:
        return (v >> (depth - lib_depth)) & mask                    # planecopy_sp
    return (v << (lib_depth - depth)) & mask                        # planecopy_sp_shl, depth == lib_depth too


def expected(planes, depth, lib_depth, W, H, mx, my, clip=(-1, -1)):
    """dst(x, y) = conv(src(clamp(x, 0, sw - 1), clamp(y, 0, sh - 1))) over the padded area of each plane; zero elsewhere"""
    g = geometry(W, H, mx, my)
    out = np.zeros(g["total"], np.uint8 if lib_depth == 8 else np.uint16)
    for k, pl in enumerate(planes):
        w, h, pmx, pmy, st = (W >> (k > 0)), (H >> (k > 0)), (mx >> (k > 0)), (my >> (k > 0)), (g["cstride"] if k else g["stride"])
        v = conv(pl, depth, lib_depth)
        if k == 0 and (clip[0] >= 0 or clip[1] >= 0):
            v = np.maximum(np.minimum(v, clip[1] if clip[1] >= 0 else (1 << lib_depth) - 1), max(clip[0], 0))
        ys = np.clip(np.arange(-pmy, h + pmy), 0, pl.shape[0] - 1)
        xs = np.clip(np.arange(-pmx, w + pmx), 0, pl.shape[1] - 1)
        padded = v[ys][:, xs]
        first = (0, g["ysz"], g["ysz"] + g["csz"])[k]
        rows = first + np.arange(padded.shape[0])[:, None] * st + np.arange(padded.shape[1])[None, :]
        out[rows] = padded.astype(out.dtype)
    return out


def run_model(lib_depth, surf, sw, sh, W, H, mx, my, fill=0xA5):
    lib = T.load_hip(lib_depth).lib
    lib.x265amd_ingest_model.argtypes = [C.POINTER(Surface), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.x265amd_last_error.restype = C.c_char_p
    out = np.full(geometry(W, H, mx, my)["total"], fill * 0x0101 if lib_depth > 8 else fill, np.uint8 if lib_depth == 8 else np.uint16)
    rc = lib.x265amd_ingest_model(C.byref(surf), sw, sh, out.ctypes.data, W, H, mx, my)
    return rc, out, lib.x265amd_last_error()


def matrix():
    """(shape, picture depth, layout, stride kind, clip): every shape, depth and layout, the stride kinds and the luma bounds taking turns so that each meets each"""
    cases = []
    for i, shape in enumerate(SHAPES):
        for j, depth in enumerate(PIC_DEPTHS):
            for layout in (0, 1):
                cases.append((shape, depth, layout, STRIDES[(i + j + layout) % 3], (i + j + layout) % 2 == 1))
    return cases


def clip_bounds(lib_depth, on):
    return ((16 << (lib_depth - 8)), (200 << (lib_depth - 8))) if on else (-1, -1)


@pytest.mark.parametrize("lib_depth", [8, 10])
def test_model_equals_the_conversion_table(lib_depth):
    mx, my = MARGINS
    seen = set()
    for n, ((sw, sh, W, H), depth, layout, stride_kind, clip_on) in enumerate(matrix()):
        for clip in (clip_bounds(lib_depth, clip_on),) + ((clip_bounds(lib_depth, not clip_on),) if sw == 18 else ()):
            planes, raw = make_source(1000 + n, sw, sh, depth, layout, stride_kind)
            rc, got, err = run_model(lib_depth, surface_of(raw, depth, layout, clip), sw, sh, W, H, mx, my)
            assert rc == 0, err
            want = expected(planes, depth, lib_depth, W, H, mx, my, clip)
            assert np.array_equal(got, want), ((sw, sh, W, H), depth, layout, stride_kind, clip, np.flatnonzero(got != want)[:8])
            seen.add((depth, layout, stride_kind, clip[0] >= 0))
    assert {s[0] for s in seen} == set(PIC_DEPTHS) and {s[2] for s in seen} == set(STRIDES) and {s[3] for s in seen} == {True, False}


def test_the_masks_matter():
    """16-bit words with bits above the picture's depth: the 10-bit library masks them off for a 10-bit picture (planecopy_sp_shl by 0 bits), where the same-depth planar
    path copies them; and the bounds are applied to luma alone"""
    (sw, sh, W, H), (mx, my) = SHAPES[0], MARGINS
    planes, raw = make_source(7, sw, sh, 10, 0, "w")
    assert planes[0].max() > 1023
    rc, got, err = run_model(10, surface_of(raw, 10, 0), sw, sh, W, H, mx, my)
    assert rc == 0 and got.max() <= 1023
    g = geometry(W, H, mx, my)
    assert np.array_equal(got[g["org"][0]:g["org"][0] + sw], planes[0][0] & 1023)
    rc, clipped, err = run_model(10, surface_of(raw, 10, 0, (300, 700)), sw, sh, W, H, mx, my)
    assert rc == 0 and clipped[:g["ysz"]].min() == 300 and clipped[:g["ysz"]].max() == 700
    assert np.array_equal(clipped[g["ysz"]:], got[g["ysz"]:]) and got[g["ysz"]:].max() > 700


def upload_style(planes, lib_depth, W, H, mx, my):
    """the buffer as x265amd_encoder::uploadPicture's host branch puts it together (csrc/encoder_api.hip): rows copied, the pad from the last column, rows below from the
    last row, the side margins, then whole rows above and below -- over a zeroed buffer"""
    g = geometry(W, H, mx, my)
    out = np.zeros(g["total"], np.uint8 if lib_depth == 8 else np.uint16)
    for k, pl in enumerate(planes):
        w, h, pmx, pmy, st = (W >> (k > 0)), (H >> (k > 0)), (mx >> (k > 0)), (my >> (k > 0)), (g["cstride"] if k else g["stride"])
        sh, sw = pl.shape
        base = g["org"][k]
        for y in range(h):
            row = out[base + y * st - pmx:base + y * st + w + pmx]
            row[pmx:pmx + sw] = pl[min(y, sh - 1)]
            row[pmx + sw:pmx + w] = row[pmx + sw - 1]
            row[:pmx] = row[pmx]
            row[pmx + w:] = row[pmx + w - 1]
        for y in range(1, pmy + 1):
            out[base - y * st - pmx:base - y * st + w + pmx] = out[base - pmx:base + w + pmx]
            out[base + (h - 1 + y) * st - pmx:base + (h - 1 + y) * st + w + pmx] = out[base + (h - 1) * st - pmx:base + (h - 1) * st + w + pmx]
    return out


@pytest.mark.parametrize("lib_depth", [8, 10])
def test_same_depth_planar_is_the_upload_buffer(lib_depth):
    mx, my = MARGINS
    for n, (sw, sh, W, H) in enumerate(SHAPES + [(198, 150, 200, 152)]):
        planes, raw = make_source(50 + n, sw, sh, lib_depth, 0, STRIDES[n % 3], in_range=True)
        rc, got, err = run_model(lib_depth, surface_of(raw, lib_depth, 0), sw, sh, W, H, mx, my)
        assert rc == 0, err
        assert np.array_equal(got, upload_style(planes, lib_depth, W, H, mx, my)), (sw, sh)


REFUSALS = [("null plane", dict(null=1), b"plane"), ("depth 7", dict(depth=7), b"bitDepth"), ("depth 17", dict(depth=17), b"bitDepth"),
            ("short stride", dict(stride0=17), b"stride"), ("odd stride, 16-bit", dict(depth=10, stride0=37), b"alignment"), ("odd address, 16-bit", dict(depth=10, shift=1), b"alignment"),
            ("odd srcW", dict(sw=17), b"srcW"), ("odd srcH", dict(sh=9), b"srcH"), ("W < srcW", dict(W=16), b"srcW"), ("bound above the range", dict(clip=(0, 1 << 10)), b"clip"),
            ("bounds crossed", dict(clip=(90, 80)), b"clip"), ("layout 2", dict(layout=2), b"layout")]


@pytest.mark.parametrize("what,change,word", REFUSALS, ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("lib_depth", [8, 10])
def test_refusals_are_named_and_leave_the_destination_alone(lib_depth, what, change, word):
    (sw, sh, W, H), (mx, my) = SHAPES[0], MARGINS
    depth = change.get("depth", 8)
    planes, raw = make_source(3, sw, sh, 16 if depth > 8 else 8, 0, "w", lead=2)
    s = surface_of(raw, depth, change.get("layout", 0), change.get("clip", (-1, -1)))
    if "null" in change:
        s.planes[change["null"]] = None
    if "stride0" in change:
        s.stride[0] = change["stride0"]
    if "shift" in change:
        s.planes[0] = s.planes[0] + change["shift"]
    rc, got, err = run_model(lib_depth, s, change.get("sw", sw), change.get("sh", sh), change.get("W", W), H, mx, my)
    assert rc != 0 and word in err, (what, err)
    assert (got.view(np.uint8) == 0xA5).all()


# ---- x265_dither_image ----
DITHER_SIZES = ((34, 6), (2, 2))
DITHER_PAIRS = ((10, 8), (12, 8), (12, 10), (16, 8), (16, 10))


def dither_input(kind, w, h, depth):
    """three planes of a 4:2:0 picture of `depth` bits in 16-bit words, stride == width (the reference's up-conversion assumes it)"""
    rng = np.random.default_rng(depth * 1000 + w * 10 + h)
    planes = []
    for k in range(3):
        pw, ph = (w >> (k > 0)), (h >> (k > 0))
        if kind == "random":
            planes.append(rng.integers(0, 1 << depth, (ph, pw)).astype(np.uint16))
        else:
            planes.append(((np.arange(ph * pw, dtype=np.int64).reshape(ph, pw) * ((1 << depth) - 1)) // max(ph * pw - 1, 1) + k).clip(0, (1 << depth) - 1).astype(np.uint16))
    return planes


def dither_cases():
    return [(kind, w, h, depth, target) for kind in ("random", "ramp") for (w, h) in DITHER_SIZES for (depth, target) in DITHER_PAIRS]


def dither_key(kind, w, h, depth, target):
    return "dither/%s/%dx%d/%dto%d" % (kind, w, h, depth, target)


def dither_call(fn, planes, w, h, depth, target, csp=1):
    """x265_dither_image(x265_picture*, width, height, errorBuf, bitDepth) on a picture put together at the generated offsets: every plane's bytes afterwards (the packed
    bytes towards 8 bits and what is left behind them) and the error row"""
    L = A.LAYOUT
    pic = np.zeros(L["SIZEOF_PICTURE"], np.uint8)
    bufs = [np.ascontiguousarray(p).copy() for p in planes]
    for k, b in enumerate(bufs):
        pic[L["PIC_planes"] + 8 * k:L["PIC_planes"] + 8 * k + 8] = np.frombuffer(int(b.ctypes.data).to_bytes(8, "little"), np.uint8)
        pic[L["PIC_stride"] + 4 * k:L["PIC_stride"] + 4 * k + 4] = np.frombuffer(int(b.strides[0]).to_bytes(4, "little"), np.uint8)
    pic[L["PIC_bitDepth"]:L["PIC_bitDepth"] + 4] = np.frombuffer(int(depth).to_bytes(4, "little"), np.uint8)
    pic[L["PIC_colorSpace"]:L["PIC_colorSpace"] + 4] = np.frombuffer(int(csp).to_bytes(4, "little"), np.uint8)
    errors = np.full(w + 1, 0x5555, np.int16)
    fn(pic.ctypes.data, w, h, errors.ctypes.data, target)
    return [b.view(np.uint8).reshape(-1) for b in bufs], errors


def our_dither(target):
    api = A._fns(A.table(target), target)["api"]
    return C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int)(api.fn2[7])


def reference_dither(target):
    R = C.CDLL(os.path.join(T.REF_DIR, "libx265_ref%d.so" % target))
    R.x265_dither_image.restype = None
    R.x265_dither_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return R.x265_dither_image


def test_dither_golden_is_complete():
    gold = np.load(GOLD_PATH)
    want = sorted(dither_key(*c) + "/" + leaf for c in dither_cases() for leaf in ("plane0", "plane1", "plane2", "errors"))
    assert sorted(gold.files) == want


@pytest.mark.parametrize("case", dither_cases(), ids=[dither_key(*c) for c in dither_cases()])
def test_dither_image_equals_the_references(case):
    kind, w, h, depth, target = case
    gold = np.load(GOLD_PATH)
    bufs, errors = dither_call(our_dither(target), dither_input(kind, w, h, depth), w, h, depth, target)
    for k in range(3):
        assert np.array_equal(bufs[k], gold[dither_key(*case) + "/plane%d" % k]), (case, k)
    assert np.array_equal(errors, gold[dither_key(*case) + "/errors"]), case


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref (the reference build) is not present")
def test_dither_golden_is_the_reference():
    """cut again through the reference library's own x265_dither_image (oracle/_ref), the committed results come out"""
    gold = np.load(GOLD_PATH)
    for case in dither_cases():
        kind, w, h, depth, target = case
        bufs, errors = dither_call(reference_dither(target), dither_input(kind, w, h, depth), w, h, depth, target)
        for k in range(3):
            assert np.array_equal(bufs[k], gold[dither_key(*case) + "/plane%d" % k]), (case, k)
        assert np.array_equal(errors, gold[dither_key(*case) + "/errors"]), case


@pytest.mark.parametrize("depth,target", [(8, 8), (8, 10), (10, 10), (16, 16)])
def test_dither_image_leaves_these_alone(depth, target):
    """pictures of 8 bits, and pictures of the target's depth: nothing is touched, as in the reference"""
    lib_depth = 8 if target == 8 else 10
    planes = dither_input("random", 34, 6, max(depth, 9))
    before = [p.copy() for p in planes]
    bufs, errors = dither_call(our_dither(lib_depth), planes, 34, 6, depth, target)
    assert all(np.array_equal(b, p.view(np.uint8).reshape(-1)) for b, p in zip(bufs, before)) and (errors == 0x5555).all()


# ---- the reference ABI ----
def _u16(p, name_off):
    buf = (C.c_ubyte * A.LAYOUT["SIZEOF_PARAM"]).from_address(p)
    return int.from_bytes(bytes(buf[name_off:name_off + 2]), "little")


def _ingest_layout():
    out = {}
    for line in open(os.path.join(T.PKG_DIR, "host", "x265_abi_layout_ingest.h")):
        if line.startswith("#define X265ABI_"):
            k, v = line.split()[1:3]
            out[k[8:]] = int(v)
    return out


def test_layout_of_the_new_members_in_both_headers():
    """tests/native/abi_layout_ingest_check.cpp: x265amd_surface as the ctypes mirror has it and -- where the reference's headers are built -- the offsets of minLuma / maxLuma"""
    assert C.sizeof(Surface) == 56 and Surface.bitDepth.offset == 36 and Surface.clipMax.offset == 48
    ref_src = os.path.join(T.REF_DIR, "include")
    cmd = ["g++", "-std=gnu++11", "-fsyntax-only", "-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.PKG_DIR, "host")]
    if os.path.isdir(ref_src):
        cmd += ["-DWITH_REFERENCE_HEADER", "-I" + os.path.join(T.REF_DIR, "cfg"), "-I" + ref_src]
    r = subprocess.run(cmd + [os.path.join(T.ROOT, "tests", "native", "abi_layout_ingest_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("depth", [8, 10])
def test_param_parse_knows_the_luma_bounds(depth):
    I = _ingest_layout()
    f = A._fns(A.table(depth), depth)
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0
    assert (_u16(p, I["PARAM_minLuma"]), _u16(p, I["PARAM_maxLuma"])) == (0, (1 << depth) - 1)          # param.cpp:334-335
    assert f["parse"](p, b"min-luma", b"64") == 0 and f["parse"](p, b"max-luma", b"200") == 0
    assert (_u16(p, I["PARAM_minLuma"]), _u16(p, I["PARAM_maxLuma"])) == (64, 200)
    f["free"](p)


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref (the reference build) is not present")
def test_param_parse_of_the_luma_bounds_matches_the_references():
    I = _ingest_layout()
    R, f = A._reference_api(), A._fns(A.table(8))
    a, b = R.x265_param_alloc(), f["alloc"]()
    R.x265_param_default_preset(a, b"medium", None); f["preset"](b, b"medium", None)
    for name, value in ((b"min-luma", b"16"), (b"max-luma", b"235"), (b"min_luma", b"0"), (b"max-luma", b"70000"), (b"min-luma", None)):
        ra, rb = R.x265_param_parse(a, name, value), f["parse"](b, name, value)
        assert ra == rb == (0 if value is not None else -2), (name, value, ra, rb)
        assert A._members(a) == A._members(b) and [_u16(a, I[k]) for k in ("PARAM_minLuma", "PARAM_maxLuma")] == [_u16(b, I[k]) for k in ("PARAM_minLuma", "PARAM_maxLuma")], (name, value)
    R.x265_param_free(a); f["free"](b)


def _encode_complaint(depth_lib, pic_depth, csp):
    """x265_encoder_encode through the table WITHOUT an encoder (x265_encoder_open refused one: lossless coding, so that nothing touches a device): the picture's form is
    looked at first, and the complaint says what is wrong with the call"""
    lib = A.table(depth_lib)
    f = A._fns(lib, depth_lib)
    lib.x265amd_last_error.restype = C.c_char_p
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0 and f["parse"](p, b"input-res", b"128x128") == 0 and f["parse"](p, b"lossless", None) == 0
    enc = f["open"](p)
    assert not enc and b"lossless" in lib.x265amd_last_error()
    encode = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(f["api"].fn[15])
    L = A.LAYOUT
    pic = np.zeros(L["SIZEOF_PICTURE"], np.uint8)
    pic[L["PIC_bitDepth"]:L["PIC_bitDepth"] + 4] = np.frombuffer(int(pic_depth).to_bytes(4, "little"), np.uint8)
    pic[L["PIC_colorSpace"]:L["PIC_colorSpace"] + 4] = np.frombuffer(int(csp).to_bytes(4, "little"), np.uint8)
    rc = encode(enc, None, None, pic.ctypes.data, None)
    f["free"](p)
    return rc, lib.x265amd_last_error()


def test_the_table_no_longer_refuses_other_depths_by_name():
    for lib_depth, pic_depth, csp in ((8, 10, 1), (8, 16, 4), (10, 8, 1), (10, 12, 4)):
        rc, err = _encode_complaint(lib_depth, pic_depth, csp)
        assert rc == -1 and b"null encoder" in err and b"depth" not in err.lower() and b"colorSpace" not in err, err
    for lib_depth, pic_depth, csp, word in ((8, 7, 1, b"bitDepth"), (10, 17, 1, b"bitDepth"), (8, 8, 2, b"colorSpace"), (10, 10, 3, b"colorSpace"), (8, 8, 0, b"colorSpace")):
        rc, err = _encode_complaint(lib_depth, pic_depth, csp)
        assert rc == -1 and word in err, err
