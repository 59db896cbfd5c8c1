"""--sao-non-deblock, --limit-sao and --selective-sao through the encoder: the command line program, the library's own interface (x265amd_encoder_open_ext) and the
x265_api table give the reference program's bytes for the same arguments (tests/golden/encoder_sao_options_golden.json, cut by
tests/golden/make_sao_options_golden.py, in the record layout of encoder_rskip_edge_golden.json); what is refused round them is refused by name.

Every case's fixture also holds the md5 of the reference's stream for the same line WITHOUT the SAO option(s): the generator asserts that it differs from the case's, so
no case can pass with its option ignored.  It also asserts that --selective-sao 0 and 4 give the plain line's stream and that --selective-sao 2 --no-sao gives the
stream of --selective-sao 2 (the option switches SAO on)."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import hevc_testlib as T
import sao_options_lib as S

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "encoder_sao_options_golden.json")
CLI = os.path.join(T.PKG_DIR, "bin", "x265amd")

# tag -> (size, pictures, depth, survey_clip's configuration, the command line; T.PRESET_CLI follows it)
M = ["--preset", "medium"]
CASES = {
    "nd/": ((416, 240), 16, 8, 2, M + ["--sao-non-deblock"]),
    "limit/": ((416, 240), 16, 8, 2, M + ["--limit-sao"]),
    "nd_limit/": ((416, 240), 16, 8, 2, M + ["--sao-non-deblock", "--limit-sao"]),
    "nd_ft1/": ((416, 240), 16, 8, 2, M + ["--sao-non-deblock", "--frame-threads", "1"]),
    "limit_ft1/": ((416, 240), 16, 8, 2, M + ["--limit-sao", "--frame-threads", "1"]),
    "nd_nodeblock/": ((416, 240), 16, 8, 2, M + ["--sao-non-deblock", "--no-deblock"]),          # both statistics on the same samples
    "sel1/": ((416, 240), 16, 8, 2, M + ["--selective-sao", "1"]),
    "sel2/": ((416, 240), 16, 8, 2, M + ["--selective-sao", "2"]),
    "sel3/": ((416, 240), 16, 8, 2, M + ["--selective-sao", "3"]),
    "sel2_nosao/": ((416, 240), 16, 8, 2, M + ["--selective-sao", "2", "--no-sao"]),
    "b0_limit/": ((416, 240), 16, 8, 2, M + ["--bframes", "0", "--limit-sao"]),                  # P slices only: the skipped CTUs' rule
    "veryfast_limit/": ((416, 240), 16, 8, 2, ["--preset", "veryfast", "--limit-sao"]),
    "slow_nd_limit/": ((416, 240), 16, 8, 2, ["--preset", "slow", "--sao-non-deblock", "--limit-sao"]),
    "small_nd/": ((200, 152), 12, 8, 2, M + ["--sao-non-deblock"]),                              # a last CTU column of 8, a last row of 24
    "small_limit/": ((200, 152), 12, 8, 2, M + ["--limit-sao"]),
    "hbd_nd_limit/": ((416, 240), 12, 10, 2, M + ["--sao-non-deblock", "--limit-sao"]),
    "hbd_sel2/": ((416, 240), 12, 10, 2, M + ["--selective-sao", "2"]),
}
# through x265amd_encoder_open_ext: tag -> the members of x265amd_param_ext behind the case's options
LIB_CASES = {"nd/": dict(bSaoNonDeblocked=1), "limit/": dict(bLimitSAO=1), "sel2/": dict(selectiveSAO=2)}
API_TAG = "nd_limit/"


def plain_cli(cli):
    """the case's line without its SAO option(s)"""
    out, i = [], 0
    while i < len(cli):
        if cli[i] in ("--sao-non-deblock", "--limit-sao"):
            i += 1
        elif cli[i] == "--selective-sao":
            i += 2
        else:
            out.append(cli[i]); i += 1
    return out


def case_frames(tag):
    (w, h), n, depth, clip, _ = CASES[tag]
    return T.survey_clip(w, h, depth, clip, 0, n)


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
        assert len(g[tag]["plain_stream_md5"]) == 32 and g[tag]["plain_stream_md5"] != g[tag]["stream_md5"], tag
        assert g[tag]["plain_command_line"] == " ".join(plain_cli(cli) + T.PRESET_CLI), tag
    assert g["sel2_nosao/"]["stream_md5"] == g["sel2/"]["stream_md5"]
    assert len({g[t]["plain_stream_md5"] for t in ("nd/", "limit/", "nd_limit/", "sel1/", "sel2/", "sel3/")}) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(CASES))
def test_sao_option_command_lines(tag, tmp_path):
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
    print(tag, "stream", len(got), md5, "reference", g["stream_bytes"], g["stream_md5"], "without the option(s)", g["plain_stream_md5"])
    bad = [k for k in range(n) if hashlib.md5(rec[k * fsz:(k + 1) * fsz].tobytes()).hexdigest() != g["recon_md5"][k]]
    assert not bad, "reconstruction of pictures %s in display order" % bad
    assert len(got) == g["stream_bytes"] and md5 == g["stream_md5"]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(LIB_CASES))
def test_sao_options_through_the_library(tag):
    """x265amd_encoder_open_ext with the option in the extension record: the bytes of the case's command line"""
    g = json.load(open(GOLD_PATH))[tag]
    (w, h), n, depth, _, _ = CASES[tag]
    stream, coded = S.encoder_run_ext(T.load_hip(depth), case_frames(tag), w, h, LIB_CASES[tag], **T.PRESET_BASE)
    assert coded == n
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream.tobytes()).hexdigest() == g["stream_md5"]


@pytest.mark.gpu
def test_plain_open_and_empty_records_give_the_plain_stream():
    """x265amd_encoder_open(p), open_ext(p, NULL), a record of zeros, a record that only knows its size word, and selectiveSAO 4: the stream of the line without options"""
    g = json.load(open(GOLD_PATH))["limit/"]
    (w, h), n, depth, _, _ = CASES["limit/"]
    frames = case_frames("limit/")
    L = T.load_hip(depth)
    plain, _ = T.encoder_run(L, frames, w, h, **T.PRESET_BASE)
    assert hashlib.md5(plain.tobytes()).hexdigest() == g["plain_stream_md5"]
    for ext in (None, dict(), dict(selectiveSAO=4)):
        got, coded = S.encoder_run_ext(L, frames, w, h, ext, **T.PRESET_BASE)
        assert coded == n and np.array_equal(got, plain), ext


@pytest.mark.gpu
def test_sao_options_through_the_api_table():
    """x265_api_get_209: param_default_preset + param_parse of the options + encoder_open + encoder_encode give the same bytes"""
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
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0
    for name, value in ((b"input-res", b"%dx%d" % (w, h)), (b"fps", b"30/1"), (b"sar", b"1"), (b"sao-non-deblock", None), (b"limit-sao", b"1"), (b"no-info", None)):
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
    assert len(out) == g["stream_bytes"] and hashlib.md5(bytes(out)).hexdigest() == g["stream_md5"]


def _open(ext, **fields):
    """open an encoder on a 128x128 picture under the preset's rate control; returns (handle or None, the error text)"""
    lib = T.load_hip(8).lib
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_encoder_close.argtypes = [C.c_void_p]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight = 128, 128
    for k, v in dict(T.PRESET_RC, **fields).items():
        setattr(prm, k, v)
    enc = S.open_ext(lib, prm, ext)
    err = lib.x265amd_last_error()
    if enc:
        lib.x265amd_encoder_close(enc)
    return enc, err


def _ext(size=None, reserved=None, **fields):
    e = S.ParamExt(size=C.sizeof(S.ParamExt) if size is None else size, **fields)
    for k, v in (reserved or {}).items():
        e.reserved[k] = v
    return e


@pytest.mark.gpu
def test_what_is_refused_round_the_sao_options():
    for ext, word in ((_ext(selectiveSAO=5), b"selectiveSAO"), (_ext(selectiveSAO=-1), b"selectiveSAO"), (_ext(reserved={0: 1}), b"reserved"), (_ext(reserved={11: -1}), b"reserved"),
                      (_ext(size=0), b"size"), (_ext(size=2), b"size"), (_ext(size=18), b"size"), (_ext(size=C.sizeof(S.ParamExt) + 4), b"size")):
        enc, err = _open(ext)
        assert not enc and word in err, (ext.size, err)
    for fields in (dict(bSaoNonDeblocked=1), dict(bLimitSAO=1), dict(selectiveSAO=2)):
        enc, err = _open(_ext(**fields), shardCount=2, shardRank=0, frameNumThreads=2)
        assert not enc and b"shardCount" in err and b"SAO" in err, (fields, err)


@pytest.mark.gpu
def test_what_opens_round_the_sao_options():
    """the rules of Encoder::configure as x265amd_encoder_open_ext restates them: without SAO the two switches are cleared before the refusal under shardCount looks;
    selectiveSAO switches SAO on (and is then refused there); a record cut short of a member reads it as zero; selectiveSAO 4 is every picture -- the plain encoder"""
    for ext, fields in ((_ext(bSaoNonDeblocked=1, bLimitSAO=1), dict(bEnableSAO=0, shardCount=2, shardRank=0, frameNumThreads=2)),
                        (_ext(selectiveSAO=4), dict(shardCount=2, shardRank=0, frameNumThreads=2)),
                        (_ext(size=12, selectiveSAO=5), dict()),                    # the caller's record ends before selectiveSAO
                        (_ext(size=4, bSaoNonDeblocked=1), dict(shardCount=2, shardRank=0, frameNumThreads=2)),
                        (_ext(bSaoNonDeblocked=1, bLimitSAO=1, selectiveSAO=3), dict(bEnableSAO=0)),
                        (None, dict())):
        enc, err = _open(ext, **fields)
        assert enc, (fields, err)
    enc, err = _open(_ext(selectiveSAO=1), bEnableSAO=0, shardCount=2, shardRank=0, frameNumThreads=2)          # SAO is on by then
    assert not enc and b"shardCount" in err
