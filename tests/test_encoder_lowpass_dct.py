"""--lowpass-dct through the encoder: the command line program, the library's own interface (x265amd_encoder_open_tools) and the x265_api table give the reference
program's bytes for the same arguments (tests/golden/encoder_lowpass_dct_golden.json, cut by tests/golden/make_encoder_lowpass_dct_golden.py in the record layout of
encoder_sao_options_golden.json); what is refused round the option is refused by name; with the option off every byte is the plain encoder's.

Every case's fixture also holds the md5 of the reference's stream for the same line WITHOUT --lowpass-dct: the generator asserts that it differs from the case's, so no
case can pass with the option ignored."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import hevc_testlib as T
import sao_options_lib as S
from test_encoder_sao_options import write_y4m

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "encoder_lowpass_dct_golden.json")
CLI = os.path.join(T.PKG_DIR, "bin", "x265amd")
OPT = "--lowpass-dct"

# tag -> (size, pictures, depth, survey_clip's configuration, the command line; T.PRESET_CLI follows it)
M = ["--preset", "medium"]
CASES = {
    "medium/": ((416, 240), 16, 8, 2, M + [OPT]),
    "medium_ft1/": ((416, 240), 16, 8, 2, M + [OPT, "--frame-threads", "1"]),
    "tu1/": ((416, 240), 16, 8, 2, M + [OPT, "--tu-inter-depth", "1", "--tu-intra-depth", "1"]),           # 32x32 units wherever a 32x32 CU wins
    "all_intra/": ((416, 240), 8, 8, 2, M + [OPT, "--keyint", "1"]),                                        # intra 32x32 units and chroma 16x16
    "veryfast/": ((416, 240), 16, 8, 2, ["--preset", "veryfast", OPT]),                                     # rd 2
    "slow/": ((416, 240), 12, 8, 2, ["--preset", "slow", OPT]),                                             # RDOQ 2, psy-RDOQ
    "hbd_slow/": ((416, 240), 12, 10, 2, ["--preset", "slow", OPT]),                                        # the source block's wrapped first coefficient
    "veryslow/": ((416, 240), 8, 8, 2, ["--preset", "veryslow", OPT]),                                      # rd 6, TU depth 3
    "hbd_medium/": ((416, 240), 12, 10, 2, M + [OPT]),
    "small/": ((200, 152), 12, 8, 2, M + [OPT]),                                                            # a last CTU column of 8, a last row of 24
}
LIB_TAGS = ["medium/", "hbd_medium/", "small/"]         # through x265amd_encoder_open_tools (the lines that are T.PRESET_BASE and nothing else)
API_TAG = "medium/"


class ParamTools(C.Structure):          # x265amd_param_tools (include/x265amd_encoder.h; tests/native/abi_layout_lowpass_check.cpp pins the layout)
    _fields_ = [("size", C.c_uint32), ("bLowPassDct", C.c_int32), ("reserved", C.c_int32 * 14)]


def plain_cli(cli):
    return [o for o in cli if o != OPT]


def case_frames(tag):
    (w, h), n, depth, clip, _ = CASES[tag]
    return T.survey_clip(w, h, depth, clip, 0, n)


def open_tools(lib, prm, ext, tools):
    lib.x265amd_encoder_open_tools.restype = C.c_void_p
    lib.x265amd_encoder_open_tools.argtypes = [C.POINTER(T.EncParam), C.c_void_p, C.c_void_p]
    return lib.x265amd_encoder_open_tools(C.byref(prm), C.byref(ext) if ext is not None else None, C.byref(tools) if tools is not None else None)


def encoder_run_tools(L, frames, width, height, tools, **overrides):
    """sao_options_lib.encoder_run_ext with the encoder opened by x265amd_encoder_open_tools(p, NULL, tools)"""
    keep = S.open_ext
    S.open_ext = lambda lib, prm, ext: open_tools(lib, prm, None, tools)
    try:
        return S.encoder_run_ext(L, frames, width, height, None, **overrides)
    finally:
        S.open_ext = keep


def _tools(size=None, reserved=None, **fields):
    t = ParamTools(size=C.sizeof(ParamTools) if size is None else size, **fields)
    for k, v in (reserved or {}).items():
        t.reserved[k] = v
    return t


def test_fixtures_present_and_complete():
    g = json.load(open(GOLD_PATH))
    assert sorted(g) == sorted(CASES)
    for tag, ((w, h), n, depth, _, cli) in CASES.items():
        assert len(g[tag]["recon_md5"]) == n and g[tag]["reference_command_line"] == " ".join(cli + T.PRESET_CLI), tag
        assert len(g[tag]["stream_md5"]) == 32 and g[tag]["stream_bytes"] > 0, tag
        assert len(g[tag]["plain_stream_md5"]) == 32 and g[tag]["plain_stream_md5"] != g[tag]["stream_md5"], tag
        assert g[tag]["plain_command_line"] == " ".join(plain_cli(cli) + T.PRESET_CLI), tag
    assert C.sizeof(ParamTools) == 64 and ParamTools.bLowPassDct.offset == 4 and ParamTools.reserved.offset == 8


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(CASES))
def test_lowpass_dct_command_lines(tag, tmp_path):
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
    md5 = hashlib.md5(got.tobytes()).hexdigest()
    print(tag, "stream", len(got), md5, "reference", g["stream_bytes"], g["stream_md5"], "without the option", g["plain_stream_md5"])
    bad = [k for k in range(n) if hashlib.md5(rec[k * fsz:(k + 1) * fsz].tobytes()).hexdigest() != g["recon_md5"][k]]
    assert not bad, "reconstruction of pictures %s in display order" % bad
    assert len(got) == g["stream_bytes"] and md5 == g["stream_md5"]


def test_the_client_has_no_negative_form(tmp_path):
    """the reference's option table has --lowpass-dct and no --no-lowpass-dct (x265cli.h:341): refused as an unknown option, before any encoder is opened"""
    write_y4m(tmp_path / "clip.y4m", T.survey_clip(128, 128, 8, 2, 0, 1), 128, 128, 8)
    r = subprocess.run([CLI, "--input", str(tmp_path / "clip.y4m"), "-o", str(tmp_path / "out.hevc"), "--preset", "medium", "--no-lowpass-dct"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "unknown option --no-lowpass-dct" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(tmp_path / "out.hevc")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", LIB_TAGS)
def test_lowpass_dct_through_the_library(tag):
    """x265amd_encoder_open_tools with bLowPassDct in the record: the bytes of the case's command line"""
    g = json.load(open(GOLD_PATH))[tag]
    (w, h), n, depth, _, _ = CASES[tag]
    stream, coded = encoder_run_tools(T.load_hip(depth), case_frames(tag), w, h, _tools(bLowPassDct=1), **T.PRESET_BASE)
    assert coded == n
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream.tobytes()).hexdigest() == g["stream_md5"]


@pytest.mark.gpu
def test_plain_open_and_empty_records_give_the_plain_stream():
    """x265amd_encoder_open(p), open_ext(p, NULL), open_tools with NULL, a record of zeros and a record that only knows its size word: the stream of the line without
    the option -- header bytes included (the info SEI is on in no preset line, so it is looked at on its own below)"""
    tag = "medium/"
    g = json.load(open(GOLD_PATH))[tag]
    (w, h), n, depth, _, _ = CASES[tag]
    frames = case_frames(tag)
    L = T.load_hip(depth)
    plain, _ = T.encoder_run(L, frames, w, h, **T.PRESET_BASE)
    assert hashlib.md5(plain.tobytes()).hexdigest() == g["plain_stream_md5"]
    got, coded = S.encoder_run_ext(L, frames, w, h, None, **T.PRESET_BASE)
    assert coded == n and np.array_equal(got, plain)
    for tools in (None, _tools(), _tools(size=4, bLowPassDct=1)):
        got, coded = encoder_run_tools(L, frames, w, h, tools, **T.PRESET_BASE)
        assert coded == n and np.array_equal(got, plain), tools and tools.size


def _headers(tools, **fields):
    """the parameter sets and SEI units of an encoder on a 128x128 picture; (bytes or None, the error text)"""
    lib = T.load_hip(8).lib
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_encoder_close.argtypes = [C.c_void_p]
    lib.x265amd_encoder_headers.argtypes = [C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32)]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight = 128, 128
    for k, v in dict(T.PRESET_RC, **fields).items():
        setattr(prm, k, v)
    enc = open_tools(lib, prm, None, tools)
    err = lib.x265amd_last_error()
    if not enc:
        return None, err
    nal = C.POINTER(T.EncNal)(); nnal = C.c_uint32(0)
    assert lib.x265amd_encoder_headers(enc, C.byref(nal), C.byref(nnal)) > 0
    out = b"".join(bytes(nal[i].payload[:nal[i].sizeBytes]) for i in range(nnal.value))
    lib.x265amd_encoder_close(enc)
    return out, err


@pytest.mark.gpu
def test_header_bytes_with_the_option_off_and_on():
    """the info SEI's text ends in " lowpass-dct=1" only with the option on; off, every header byte is that of x265amd_encoder_open_ext"""
    off, _ = _headers(None, bEmitInfoSEI=1)
    zero, _ = _headers(_tools(), bEmitInfoSEI=1)
    on, _ = _headers(_tools(bLowPassDct=1), bEmitInfoSEI=1)
    assert off and off == zero
    assert b"lowpass-dct" not in off and on.rstrip(b"\x80").endswith(b" lowpass-dct=1")
    text = lambda b: b[b.index(b"x265amd ("):].rstrip(b"\x80")
    assert text(on) == text(off) + b" lowpass-dct=1"
    quiet_off, _ = _headers(None)
    quiet_on, _ = _headers(_tools(bLowPassDct=1))
    assert quiet_off == quiet_on           # nothing in VPS / SPS / PPS says it


@pytest.mark.gpu
def test_what_is_refused_round_the_option():
    for tools, word in ((_tools(reserved={0: 1}), b"reserved"), (_tools(reserved={13: -1}), b"reserved"), (_tools(size=0), b"size"), (_tools(size=2), b"size"),
                        (_tools(size=18), b"size"), (_tools(size=C.sizeof(ParamTools) + 4), b"size")):
        out, err = _headers(tools)
        assert out is None and word in err and b"x265amd_param_tools" in err, (tools.size, err)
    out, err = _headers(_tools(bLowPassDct=1), shardCount=2, shardRank=0, frameNumThreads=2)
    assert out is None and b"shardCount" in err and b"bLowPassDct" in err, err
    # a record cut short of the member reads it as zero: nothing to refuse
    out, err = _headers(_tools(size=4, bLowPassDct=1), shardCount=2, shardRank=0, frameNumThreads=2)
    assert out is not None, err


@pytest.mark.gpu
def test_lowpass_dct_through_the_api_table():
    """x265_api_get_209: param_default_preset + param_parse("lowpass-dct") + encoder_open + encoder_encode give the same bytes; and a caller who sets the member at its
    offset in x265_param, without the parser, gets them too"""
    import test_x265_api_abi as A
    tag = API_TAG
    g = json.load(open(GOLD_PATH))[tag]
    (w, h), n, depth, _, _ = CASES[tag]
    lib = A.table(depth)
    f = A._fns(lib, depth)
    api = f["api"]
    lib.x265amd_last_error.restype = C.c_char_p
    headers = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32))(api.fn[14])
    encode = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p)(api.fn[15])
    close = C.CFUNCTYPE(None, C.c_void_p)(api.fn[18])
    pic_alloc = C.CFUNCTYPE(C.c_void_p)(api.fn[7]); pic_init = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)(api.fn[9])
    frames = case_frames(tag)
    for by_parser in (True, False):
        p = f["alloc"]()
        assert f["preset"](p, b"medium", None) == 0
        for name, value in ((b"input-res", b"%dx%d" % (w, h)), (b"fps", b"30/1"), (b"sar", b"1"), (b"no-info", None)) + (((b"lowpass-dct", None),) if by_parser else ()):
            assert f["parse"](p, name, value) == 0, name
        if not by_parser:
            C.c_int32.from_address(p + A.LAYOUT["PARAM_bLowPassDct"]).value = 1
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
        Lay = A.LAYOUT
        pbuf = (C.c_ubyte * Lay["SIZEOF_PICTURE"]).from_address(pic)
        for t in range(n):
            keep = [np.ascontiguousarray(pl) for pl in frames[t]]
            for k in range(3):
                pbuf[Lay["PIC_planes"] + 8 * k:Lay["PIC_planes"] + 8 * k + 8] = list(int(keep[k].ctypes.data).to_bytes(8, "little"))
                pbuf[Lay["PIC_stride"] + 4 * k:Lay["PIC_stride"] + 4 * k + 4] = list(int(keep[k].strides[0]).to_bytes(4, "little"))
            pbuf[Lay["PIC_pts"]:Lay["PIC_pts"] + 8] = list(int(t).to_bytes(8, "little"))
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
        assert len(out) == g["stream_bytes"] and hashlib.md5(bytes(out)).hexdigest() == g["stream_md5"], by_parser
