"""Input pictures as they come, through the encoder: other depths than the library's, NV12 / P010 surfaces in device and host memory, --dither and the luma bounds give the
reference program's bytes for the same pictures (tests/golden/encoder_ingest_golden.json, cut by tests/golden/make_ingest_golden.py from oracle/_ref/x265_ref8 and
x265_ref10, in the record layout of encoder_me_full_golden.json).  The clip is 198x150: coded padded to 200x152, with partial CTUs right and below."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import hevc_testlib as T
import test_ingest as TI
import test_x265_api_abi as A

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "encoder_ingest_golden.json")
CLI = os.path.join(os.path.dirname(T.GOLDEN_DIR), "..", "x265-amod_amd", "bin", "x265amd")
W, H, N = 198, 150, 4
BASE_CLI = ["--preset", "medium"]
RAW16 = ["--input-res", "%dx%d" % (W, H), "--fps", "30", "--input-depth", "16"]

# tag -> (the reference binary's depth, the clip's depth, "y4m" or "raw16" (the 10-bit clip as MSB-aligned 16-bit words), the command line; T.PRESET_CLI follows it)
CASES = {
    "a_8_into_8/": (8, 8, "y4m", BASE_CLI),
    "b_8_into_10/": (10, 8, "y4m", BASE_CLI + ["-D", "10"]),
    "c_10_into_8/": (8, 10, "y4m", BASE_CLI + ["-D", "8"]),
    "d_10_into_8_dither/": (8, 10, "y4m", BASE_CLI + ["-D", "8", "--dither"]),
    "e_16_into_8/": (8, 10, "raw16", BASE_CLI + RAW16 + ["-D", "8"]),
    "e_16_into_10/": (10, 10, "raw16", BASE_CLI + RAW16 + ["-D", "10"]),
    "f_10_luma_bounds/": (10, 10, "y4m", BASE_CLI + ["--min-luma", "300", "--max-luma", "700"]),
    "plain_10_into_10/": (10, 10, "y4m", BASE_CLI),
    # (survey_clip's 10-bit samples are its 8-bit samples times four: c and d above never see a low bit.  The same clip with two low bits of a fixed pattern:)
    "g_10_low_bits_into_8/": (8, 10, "y4m+low", BASE_CLI + ["-D", "8"]),
    "g_10_low_bits_into_8_dither/": (8, 10, "y4m+low", BASE_CLI + ["-D", "8", "--dither"]),
}
# what the generator asserts between the records: the same stream, or another one
# (the low bits are cut off, not rounded: planecopy_sp.  Only the dither sees them)
SAME = (("e_16_into_10/", "plain_10_into_10/"), ("e_16_into_8/", "c_10_into_8/"), ("g_10_low_bits_into_8/", "c_10_into_8/"))
DIFFERENT = (("f_10_luma_bounds/", "plain_10_into_10/"), ("g_10_low_bits_into_8_dither/", "g_10_low_bits_into_8/"))
# the library's fields for `--preset medium` on these files: the frame rate as `--fps 30` stores it (30000 / 1000, param.cpp:936-941; the clip files' headers say the same),
# no sample aspect ratio (a raw file has none, and the clip files' headers name none)
BASE = dict(T.PRESET_BASE, fpsNum=30000, fpsDenom=1000, aspectRatioIdc=0)


def clip(depth, low_bits=False):
    frames = T.survey_clip(W, H, depth, 2, 0, N)
    if low_bits:
        for t, fr in enumerate(frames):
            for k, pl in enumerate(fr):
                y, x = np.indices(pl.shape)
                pl[...] = np.minimum(pl + ((x * 7 + y * 13 + t * 5 + k) & 3), (1 << depth) - 1).astype(pl.dtype)
    return frames


def _write_y4m(path, frames, depth):
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30000:1000 Ip %s\n" % (W, H, b"C420p10" if depth == 10 else b"C420"))
        for fr in frames:
            f.write(b"FRAME\n")
            for pl in fr:
                f.write(np.ascontiguousarray(pl).tobytes())


def _write_raw16(path, frames):
    with open(path, "wb") as f:
        for fr in frames:
            for pl in fr:
                f.write((np.ascontiguousarray(pl).astype(np.uint16) << 6).tobytes())


def write_input(d, tag):
    _, depth, form, _ = CASES[tag]
    if form == "raw16":
        _write_raw16(os.path.join(d, "clip.yuv"), clip(10))
        return "clip.yuv"
    _write_y4m(os.path.join(d, "clip.y4m"), clip(depth, form == "y4m+low"), depth)
    return "clip.y4m"


def frame_bytes(lib_depth):
    return W * H * 3 // 2 * (2 if lib_depth > 8 else 1)


def read_recon(path, lib_depth):
    """the pictures of a YUV4MPEG2 reconstruction file in display order.  (The reference program's raw .yuv writer mistakes the sample size whenever the input's depth and the
    library's differ -- source/output/yuv.cpp:60-105 --, its y4m writer does not: the records are cut from rec.y4m)"""
    data = open(path, "rb").read()
    at, fsz = data.index(b"\n") + 1, frame_bytes(lib_depth)
    assert data.startswith(b"YUV4MPEG2") and len(data) == at + N * (6 + fsz), (len(data), at, fsz)
    frames = []
    for k in range(N):
        assert data[at + k * (6 + fsz):at + k * (6 + fsz) + 6] == b"FRAME\n"
        frames.append(data[at + k * (6 + fsz) + 6:at + (k + 1) * (6 + fsz)])
    return frames


def check(tag, stream, recons):
    """stream: bytes; recons: the reconstructed pictures in display order, each the bytes of its three planes"""
    g = json.load(open(GOLD_PATH))[tag]
    assert len(recons) == N
    for k in range(N):
        assert hashlib.md5(recons[k]).hexdigest() == g["recon_md5"][k], "%s: reconstruction of picture %d in display order" % (tag, k)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"], tag


def test_fixtures_present_and_complete():
    g = json.load(open(GOLD_PATH))
    assert sorted(g) == sorted(CASES)
    for tag, (_, _, _, cli) in CASES.items():
        assert len(g[tag]["recon_md5"]) == N and g[tag]["reference_command_line"] == " ".join(cli + T.PRESET_CLI), tag
        assert len(g[tag]["stream_md5"]) == 32 and g[tag]["stream_bytes"] > 0, tag
    key = lambda t: (g[t]["stream_md5"], g[t]["stream_bytes"], g[t]["recon_md5"])
    for a, b in SAME:
        assert key(a) == key(b), (a, b)
    for a, b in DIFFERENT:
        assert g[a]["stream_md5"] != g[b]["stream_md5"], (a, b)
    assert os.path.exists(TI.GOLD_PATH)


# ---- the command line program ----
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["b_8_into_10/", "c_10_into_8/", "d_10_into_8_dither/", "f_10_luma_bounds/", "g_10_low_bits_into_8/", "g_10_low_bits_into_8_dither/"])
def test_command_lines(tag, tmp_path):
    """the stream and every reconstructed picture equal the reference program's for the SAME arguments"""
    lib_depth, _, _, cli = CASES[tag]
    name = write_input(str(tmp_path), tag)
    cmd = [CLI, "--input", str(tmp_path / name), "-o", str(tmp_path / "out.hevc"), "--recon", str(tmp_path / "rec.y4m")] + cli + T.PRESET_CLI
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    check(tag, open(tmp_path / "out.hevc", "rb").read(), read_recon(tmp_path / "rec.y4m", lib_depth))


# ---- the library: x265amd_encoder_encode_surface ----
def nv12(frame):
    """(Y, UV) of a planar frame: U,V pairs, U first"""
    return [np.ascontiguousarray(frame[0]), np.ascontiguousarray(np.stack([frame[1], frame[2]], axis=2).reshape(frame[1].shape[0], -1))]


def surface_run(lib_depth, frames, bit_depth, layout, on_device, clip_bounds=(-1, -1), before_each=None, **overrides):
    """x265amd_encoder_open -> headers -> x265amd_encoder_encode_surface for every frame -> flush -> close.  frames: per picture the stored planes (two for semi-planar).
    before_each(lib, enc, surface): called in front of every picture.  Returns (stream bytes, reconstructed pictures' bytes in display order)"""
    lib = T.load_hip(lib_depth).lib
    NalPP, U32P, PicP = C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32), C.POINTER(T.EncPicture)
    lib.x265amd_encoder_open.restype = C.c_void_p
    lib.x265amd_encoder_open.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_encoder_headers.argtypes = [C.c_void_p, NalPP, U32P]
    lib.x265amd_encoder_encode.argtypes = [C.c_void_p, NalPP, U32P, PicP, PicP]
    lib.x265amd_encoder_encode_surface.argtypes = [C.c_void_p, NalPP, U32P, C.POINTER(TI.Surface), C.c_int, PicP]
    lib.x265amd_encoder_close.argtypes = [C.c_void_p]
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight = W, H
    for k, v in dict(BASE, **overrides).items():
        assert hasattr(prm, k), k
        setattr(prm, k, v)
    enc = lib.x265amd_encoder_open(C.byref(prm))
    assert enc, lib.x265amd_last_error()
    stream = bytearray()
    nal = C.POINTER(T.EncNal)(); nnal = C.c_uint32(0)
    assert lib.x265amd_encoder_headers(enc, C.byref(nal), C.byref(nnal)) > 0
    for i in range(nnal.value):
        stream += bytes(nal[i].payload[:nal[i].sizeBytes])
    dt = np.uint8 if lib_depth == 8 else np.uint16
    recons = {}

    def out_picture():
        bufs = [np.zeros((H, W), dt), np.zeros((H // 2, W // 2), dt), np.zeros((H // 2, W // 2), dt)]
        out = T.EncPicture()
        for k in range(3):
            out.planes[k] = bufs[k].ctypes.data; out.stride[k] = bufs[k].strides[0]
        return out, bufs

    def take(ret, out, bufs):
        assert ret >= 0, lib.x265amd_last_error()
        if ret:
            for i in range(nnal.value):
                stream.extend(bytes(nal[i].payload[:nal[i].sizeBytes]))
            recons[out.poc] = b"".join(b.tobytes() for b in bufs)
        return ret

    try:
        for planes in frames:
            keep = [np.ascontiguousarray(pl) for pl in planes]
            s = TI.Surface()
            s.bitDepth, s.layout, s.clipMin, s.clipMax = bit_depth, layout, clip_bounds[0], clip_bounds[1]
            if on_device:
                import torch
                keep = [torch.from_numpy(k.view(np.uint8).reshape(k.shape[0], -1)).cuda() for k in keep]
                torch.cuda.synchronize()
                for k in range(len(keep)):
                    s.planes[k] = keep[k].data_ptr(); s.stride[k] = keep[k].stride(0)
            else:
                for k in range(len(keep)):
                    s.planes[k] = keep[k].ctypes.data; s.stride[k] = keep[k].strides[0]
            if before_each:
                before_each(lib, enc, s)
            out, bufs = out_picture()
            take(lib.x265amd_encoder_encode_surface(enc, C.byref(nal), C.byref(nnal), C.byref(s), int(on_device), C.byref(out)), out, bufs)
        while True:
            out, bufs = out_picture()
            if not take(lib.x265amd_encoder_encode_surface(enc, C.byref(nal), C.byref(nnal), None, 0, C.byref(out)), out, bufs):
                break
    finally:
        lib.x265amd_encoder_close(enc)
    return bytes(stream), [recons[k] for k in sorted(recons)]


@pytest.mark.gpu
def test_nv12_device_surface():
    """a) an 8-bit NV12 surface in device memory: the 8-bit reference's stream for the planar clip"""
    check("a_8_into_8/", *surface_run(8, [nv12(f) for f in clip(8)], 8, 1, True))


@pytest.mark.gpu
def test_planar_host_surface():
    """a) the same pictures as three host planes through the surface entry: the same stream again"""
    check("a_8_into_8/", *surface_run(8, clip(8), 8, 0, False))


@pytest.mark.gpu
def test_8_bit_pictures_into_the_10_bit_library():
    """b) planecopy_cp: << 2"""
    check("b_8_into_10/", *surface_run(10, clip(8), 8, 0, False))


@pytest.mark.gpu
@pytest.mark.parametrize("lib_depth,tag", [(8, "e_16_into_8/"), (10, "e_16_into_10/")])
def test_p010_device_surface(lib_depth, tag):
    """e) the 10-bit clip as a P010-style surface in device memory (16-bit words, MSB-aligned, U,V pairs; bitDepth 16): into the 10-bit library the plain 10-bit stream, into
    the 8-bit library the stream of the 10-bit clip under -D 8 (the generator asserts both equalities between the reference's own runs)"""
    frames = [nv12([(pl.astype(np.uint16) << 6) for pl in f]) for f in clip(10)]
    check(tag, *surface_run(lib_depth, frames, 16, 1, True))


@pytest.mark.gpu
def test_luma_bounds_through_the_library():
    """f) clipMin / clipMax of the surface: --min-luma 300 --max-luma 700"""
    check("f_10_luma_bounds/", *surface_run(10, clip(10), 10, 0, True, clip_bounds=(300, 700)))


# ---- the reference ABI ----
@pytest.mark.gpu
def test_nv12_host_surface_through_the_abi():
    """a) x265_encoder_encode with colorSpace X265_CSP_NV12 and host planes"""
    lib = A.table(8)
    f = A._fns(lib)
    api = f["api"]
    L = A.LAYOUT
    lib.x265amd_last_error.restype = C.c_char_p
    headers = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32))(api.fn[14])
    encode = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p)(api.fn[15])
    close = C.CFUNCTYPE(None, C.c_void_p)(api.fn[18])
    pic_alloc = C.CFUNCTYPE(C.c_void_p)(api.fn[7]); pic_init = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)(api.fn[9])
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0 and f["parse"](p, b"input-res", b"%dx%d" % (W, H)) == 0 and f["parse"](p, b"fps", b"30") == 0 and f["parse"](p, b"no-info", None) == 0
    enc = f["open"](p)
    assert enc, lib.x265amd_last_error()
    nal = C.POINTER(T.EncNal)(); nnal = C.c_uint32(0)
    out = bytearray()
    assert headers(enc, C.byref(nal), C.byref(nnal)) > 0
    for i in range(nnal.value):
        out += bytes(nal[i].payload[:nal[i].sizeBytes])
    pic, rec = pic_alloc(), pic_alloc()
    pic_init(p, pic); pic_init(p, rec)
    pbuf = (C.c_ubyte * L["SIZEOF_PICTURE"]).from_address(pic)
    rbuf = (C.c_ubyte * L["SIZEOF_PICTURE"]).from_address(rec)
    pbuf[L["PIC_colorSpace"]:L["PIC_colorSpace"] + 4] = list(int(4).to_bytes(4, "little"))
    recons = {}

    def take(r):
        assert r >= 0, lib.x265amd_last_error()
        if r:
            for i in range(nnal.value):
                out.extend(bytes(nal[i].payload[:nal[i].sizeBytes]))
            word = lambda off, n: int.from_bytes(bytes(rbuf[off:off + n]), "little", signed=True)
            planes = []
            for k in range(3):
                w, h, st = (W >> (k > 0)), (H >> (k > 0)), word(L["PIC_stride"] + 4 * k, 4)
                a = np.ctypeslib.as_array((C.c_ubyte * (st * h)).from_address(word(L["PIC_planes"] + 8 * k, 8))).reshape(h, st)
                planes.append(a[:, :w].tobytes())
            recons[word(L["PIC_poc"], 4)] = b"".join(planes)
        return r

    for t, fr in enumerate(clip(8)):
        keep = nv12(fr)
        for k in range(2):
            pbuf[L["PIC_planes"] + 8 * k:L["PIC_planes"] + 8 * k + 8] = list(int(keep[k].ctypes.data).to_bytes(8, "little"))
            pbuf[L["PIC_stride"] + 4 * k:L["PIC_stride"] + 4 * k + 4] = list(int(keep[k].strides[0]).to_bytes(4, "little"))
        pbuf[L["PIC_pts"]:L["PIC_pts"] + 8] = list(int(t).to_bytes(8, "little"))
        take(encode(enc, C.byref(nal), C.byref(nnal), pic, rec))
    while take(encode(enc, C.byref(nal), C.byref(nnal), None, rec)):
        pass
    close(enc); f["free"](p)
    check("a_8_into_8/", bytes(out), [recons[k] for k in sorted(recons)])


# ---- refusals ----
@pytest.mark.gpu
def test_refused_surfaces_are_named_and_the_encoder_goes_on():
    """depth 7, depth 17 and a layout that is not 4:2:0 planar or semi-planar are refused by name by the surface entry, take no place in display order, and the pictures
    that follow are coded as if nothing had been asked"""
    calls = []

    def refused(lib, enc, s):
        for depth, layout, word in ((7, 0, b"bitDepth"), (17, 0, b"bitDepth"), (8, 2, b"layout")):
            bad = TI.Surface.from_buffer_copy(s)
            bad.bitDepth, bad.layout = depth, layout
            assert lib.x265amd_encoder_encode_surface(enc, None, None, C.byref(bad), 0, None) == -1 and word in lib.x265amd_last_error(), (depth, layout, lib.x265amd_last_error())
            calls.append(word)

    stream, recons = surface_run(8, clip(8), 8, 0, False, before_each=refused)
    assert len(calls) == 3 * N
    check("a_8_into_8/", stream, recons)


def test_422_pictures_and_depths_outside_8_to_16_are_refused_by_name():
    """x265_encoder_encode: 4:2:2 and 4:4:4 pictures, 4:0:0, depth 7 and depth 17 (no GPU: tests/test_ingest.py's way of asking)"""
    for lib_depth, pic_depth, csp, word in ((8, 8, 2, b"colorSpace"), (10, 10, 3, b"colorSpace"), (8, 7, 1, b"bitDepth"), (10, 17, 1, b"bitDepth"), (8, 17, 4, b"bitDepth")):
        rc, err = TI._encode_complaint(lib_depth, pic_depth, csp)
        assert rc == -1 and word in err, err
