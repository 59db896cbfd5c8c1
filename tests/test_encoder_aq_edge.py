"""--aq-mode 4 and 5 through the encoder: the command line program, the library's own interface and the x265_api table give the reference program's bytes for the same
arguments (tests/golden/encoder_aq_edge_golden.json, cut by tests/golden/make_aq_edge_golden.py); what stays refused round them is refused by name."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import hevc_testlib as T

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "encoder_aq_edge_golden.json")
CLI = os.path.join(T.PKG_DIR, "bin", "x265amd")

# tag -> (size, pictures, depth, clip, the command line behind the file names; T.PRESET_CLI follows it).  clip: survey_clip's configuration, or "fade" for T.wp_fade_frames
CASES = {
    "aq4_medium_wqvga/": ((416, 240), 10, 8, 2, ["--preset", "medium", "--aq-mode", "4"]),
    "aq5_medium_hbd/": ((416, 240), 8, 10, 2, ["--preset", "medium", "--aq-mode", "5"]),
    "aq4_strength_nocutree/": ((416, 240), 10, 8, 2, ["--preset", "medium", "--aq-mode", "4", "--aq-strength", "1.5", "--no-cutree"]),
    # coded size 424 x 240: the right blocks of the edge picture hang over it, and the source's padding columns are part of the picture the filter sees
    "aq4_odd_size/": ((420, 236), 8, 8, 2, ["--preset", "medium", "--aq-mode", "4"]),
    # a fade: the reference's analysis picks weights (the fixture counts the weighted pictures) from luma sums that hold the edge picture's as well.  That the stream would
    # differ without the edge picture's sums is not shown by this case; the addition itself is pinned at kernel level (the `sums` of tests/test_aq_edge.py)
    "aq4_fade/": ((416, 240), 12, 8, "fade", ["--preset", "medium", "--aq-mode", "4", "--bframes", "3", "--rc-lookahead", "8"]),
}
LIB_TAG = "aq4_medium_wqvga/"


def case_frames(tag):
    (w, h), n, depth, clip, _ = CASES[tag]
    return T.wp_fade_frames(w, h, n, depth) if clip == "fade" else T.survey_clip(w, h, depth, clip, 0, n)


def write_y4m(path, frames, w, h, depth):
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 %s\n" % (w, h, b"C420p10" if depth == 10 else b"C420"))
        for fr in frames:
            f.write(b"FRAME\n")
            for pl in fr:
                f.write(np.ascontiguousarray(pl).tobytes())


def test_fixtures_present_and_complete():
    g = json.load(open(GOLD_PATH))
    assert sorted(g) == sorted(CASES)
    for tag, ((w, h), n, depth, _, cli) in CASES.items():
        assert len(g[tag]["recon_md5"]) == n and g[tag]["reference_command_line"] == " ".join(cli + T.PRESET_CLI), tag
        assert len(g[tag]["stream_md5"]) == 32 and g[tag]["stream_bytes"] > 0, tag
    assert g["aq4_fade/"]["reference_weighted_pictures"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(CASES))
def test_aq_edge_command_lines(tag, tmp_path):
    """the stream and every reconstructed picture equal the reference program's for the SAME arguments"""
    g = json.load(open(GOLD_PATH))[tag]
    (w, h), n, depth, _, cli = CASES[tag]
    write_y4m(tmp_path / "clip.y4m", case_frames(tag), w, h, depth)
    cmd = [CLI, "--input", str(tmp_path / "clip.y4m"), "-o", str(tmp_path / "out.hevc"), "--recon", str(tmp_path / "rec.yuv")] + cli + T.PRESET_CLI
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.fromfile(tmp_path / "out.hevc", np.uint8)
    rec = np.fromfile(tmp_path / "rec.yuv", np.uint8)
    fsz = w * h * 3 // 2 * (2 if depth == 10 else 1)
    assert len(rec) == n * fsz
    for k in range(n):
        assert hashlib.md5(rec[k * fsz:(k + 1) * fsz].tobytes()).hexdigest() == g["recon_md5"][k], "reconstruction of picture %d in display order" % k
    assert len(got) == g["stream_bytes"] and hashlib.md5(got.tobytes()).hexdigest() == g["stream_md5"]


@pytest.mark.gpu
def test_aq_edge_through_the_library():
    """x265amd_encoder_open with aqMode 4: the bytes of `--preset medium --aq-mode 4`"""
    g = json.load(open(GOLD_PATH))[LIB_TAG]
    (w, h), n, depth, _, _ = CASES[LIB_TAG]
    stream, coded = T.encoder_run(T.load_hip(depth), case_frames(LIB_TAG), w, h, **dict(T.PRESET_BASE, aqMode=4))          # (aspectRatioIdc 1, as the clip file's header says: A1:1)
    assert len(coded) == n
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream.tobytes()).hexdigest() == g["stream_md5"]


def _api(depth):
    import test_x265_api_abi as A
    lib = A.table(depth)
    return A, lib, A._fns(lib, depth)


@pytest.mark.gpu
def test_aq_edge_through_the_api_table():
    """x265_api_get_209: param_default_preset + param_parse("aq-mode", "4") + encoder_open + encoder_encode give the same bytes"""
    g = json.load(open(GOLD_PATH))[LIB_TAG]
    (w, h), n, depth, _, _ = CASES[LIB_TAG]
    A, lib, f = _api(depth)
    api = f["api"]
    lib.x265amd_last_error.restype = C.c_char_p
    headers = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32))(api.fn[14])
    encode = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p)(api.fn[15])
    close = C.CFUNCTYPE(None, C.c_void_p)(api.fn[18])
    pic_alloc = C.CFUNCTYPE(C.c_void_p)(api.fn[7]); pic_init = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)(api.fn[9])
    frames = case_frames(LIB_TAG)
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0
    for name, value in ((b"input-res", b"%dx%d" % (w, h)), (b"fps", b"30/1"), (b"sar", b"1"), (b"aq-mode", b"4"), (b"no-info", None)):
        assert f["parse"](p, name, value) == 0, name
    enc = f["open"](p)
    assert enc, lib.x265amd_last_error()
    nal = C.POINTER(T.EncNal)(); nnal = C.c_uint32(0)
    out = bytearray()

    def take():
        for i in range(nnal.value):
            out.extend(bytes(nal[i].payload[:nal[i].sizeBytes]))
    assert headers(enc, C.byref(nal), C.byref(nnal)) > 0
    take()
    pic = pic_alloc(); pic_init(p, pic)
    L = A.LAYOUT
    pbuf = (C.c_ubyte * L["SIZEOF_PICTURE"]).from_address(pic)
    for t in range(n):
        keep = [np.ascontiguousarray(pl) for pl in frames[t]]
        for k in range(3):
            pbuf[L["PIC_planes"] + 8 * k:L["PIC_planes"] + 8 * k + 8] = list(int(keep[k].ctypes.data).to_bytes(8, "little"))
            pbuf[L["PIC_stride"] + 4 * k:L["PIC_stride"] + 4 * k + 4] = list(int(keep[k].strides[0]).to_bytes(4, "little"))
        pbuf[L["PIC_pts"]:L["PIC_pts"] + 8] = list(int(t).to_bytes(8, "little"))
        r = encode(enc, C.byref(nal), C.byref(nnal), pic, None)
        assert r >= 0, lib.x265amd_last_error()
        if r:
            take()
    while True:
        r = encode(enc, C.byref(nal), C.byref(nnal), None, None)
        assert r >= 0, lib.x265amd_last_error()
        if not r:
            break
        take()
    close(enc); f["free"](p)
    assert len(out) == g["stream_bytes"] and hashlib.md5(bytes(out)).hexdigest() == g["stream_md5"]


@pytest.mark.gpu
def test_api_table_opens_mode_5():
    A, lib, f = _api(8)
    lib.x265amd_last_error.restype = C.c_char_p
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0
    for name, value in ((b"input-res", b"128x128"), (b"fps", b"30/1"), (b"aq-mode", b"5")):
        assert f["parse"](p, name, value) == 0
    enc = f["open"](p)
    assert enc, lib.x265amd_last_error()
    C.CFUNCTYPE(None, C.c_void_p)(f["api"].fn[18])(enc)
    f["free"](p)


def _open_refused(word, **fields):
    lib = T.load_hip(8).lib
    lib.x265amd_encoder_open.restype = C.c_void_p
    lib.x265amd_encoder_open.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight = 128, 128
    for k, v in dict(T.PRESET_RC, **fields).items():
        setattr(prm, k, v)
    enc = lib.x265amd_encoder_open(C.byref(prm))
    if enc:
        lib.x265amd_encoder_close.argtypes = [C.c_void_p]
        lib.x265amd_encoder_close(enc)
    assert not enc and word in lib.x265amd_last_error(), lib.x265amd_last_error()


@pytest.mark.gpu
def test_what_stays_refused_round_the_edge_modes():
    _open_refused(b"aqMode", aqMode=6)
    _open_refused(b"recursionSkipMode", aqMode=4, recursionSkipMode=2)
    _open_refused(b"qgSize", aqMode=4, qgSize=16)
