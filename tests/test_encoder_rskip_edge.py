"""--rskip 2 (the edge-based recursion skip) through the encoder: the command line program, the library's own interface and the x265_api table give the reference
program's bytes for the same arguments (tests/golden/encoder_rskip_edge_golden.json, cut by tests/golden/make_rskip_edge_golden.py); what stays refused round it is
refused by name.

Every case's fixture also holds the md5 of the reference's stream for the same clip under --rskip 1, under --rskip 2 with threshold 100 (every CU that asks ends the
recursion) and under --rskip 2 with threshold 0 (almost none does): the generator asserts that the case's stream differs from all three, so a case cannot pass with the
edge decision missing, always taken or never taken."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import hevc_testlib as T

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "encoder_rskip_edge_golden.json")
CLI = os.path.join(T.PKG_DIR, "bin", "x265amd")

# tag -> (size, pictures, depth, survey_clip's configuration, the command line behind the file names; T.PRESET_CLI follows it)
CASES = {
    "rskip2_medium/": ((416, 240), 8, 8, 2, ["--preset", "medium", "--rskip", "2"]),
    # the default threshold (5) decides 32x32 CUs both ways on this clip; 6 decides 64x64 CUs both ways
    "rskip2_threshold6/": ((416, 240), 8, 8, 2, ["--preset", "medium", "--rskip", "2", "--rskip-edge-threshold", "6"]),
    "rskip2_hbd/": ((416, 240), 6, 10, 2, ["--preset", "medium", "--rskip", "2"]),
    "rskip2_rd5/": ((416, 240), 6, 8, 2, ["--preset", "medium", "--rskip", "2", "--rd", "5"]),          # compressInterCU_rd5_6's place of the decision
    # constant QP, no B pictures: adaptive quantisation is off, nothing in the lookahead touches the source's edges -- the pass runs on the picture's own stream
    "rskip2_cqp_b0/": ((416, 240), 6, 8, 2, ["--preset", "medium", "--qp", "30", "--rskip", "2", "--bframes", "0", "--no-wpp"]),
    # coded size 424 x 240: the padding columns are part of the picture the filter sees, the right blocks are partial.  (At this size clip 2 with the default threshold
    # gives the reference's threshold-0 stream, and 6 its threshold-100 stream, with 6 and with 8 pictures: the generator's condition refused both.  Clip 1, 8 pictures
    # and threshold 6 meet it)
    "rskip2_odd_size/": ((420, 236), 8, 8, 1, ["--preset", "medium", "--rskip", "2", "--rskip-edge-threshold", "6"]),
    "rskip2_frame_threads/": ((416, 240), 8, 8, 2, ["--preset", "medium", "--rskip", "2", "--frame-threads", "3"]),
}
LIB_TAG = "rskip2_medium/"
# the three encodes of the generator's condition: name -> what replaces "--rskip 2 [--rskip-edge-threshold N]" in the case's command line
OTHERS = {"rskip1": ["--rskip", "1"], "threshold100": ["--rskip", "2", "--rskip-edge-threshold", "100"], "threshold0": ["--rskip", "2", "--rskip-edge-threshold", "0"]}


def other_cli(cli, name):
    out, i = [], 0
    while i < len(cli):
        if cli[i] in ("--rskip", "--rskip-edge-threshold"):
            i += 2
            continue
        out.append(cli[i]); i += 1
    return out + OTHERS[name]


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


def float_bits(v):
    """the float's bits as the int32 the ctypes mirror of x265amd_param still names its last slot by (reserved5: now edgeVarThreshold)"""
    return struct.unpack("<i", struct.pack("<f", v))[0]


def test_fixtures_present_and_complete():
    g = json.load(open(GOLD_PATH))
    assert sorted(g) == sorted(CASES)
    for tag, ((w, h), n, depth, _, cli) in CASES.items():
        assert len(g[tag]["recon_md5"]) == n and g[tag]["reference_command_line"] == " ".join(cli + T.PRESET_CLI), tag
        assert len(g[tag]["stream_md5"]) == 32 and g[tag]["stream_bytes"] > 0, tag
        assert sorted(g[tag]["other_stream_md5"]) == sorted(OTHERS), tag
        md5s = [g[tag]["stream_md5"]] + [g[tag]["other_stream_md5"][k] for k in sorted(OTHERS)]
        assert all(len(m) == 32 for m in md5s) and len(set(md5s)) == 4, (tag, md5s)


def test_param_slot_keeps_its_place():
    """x265amd_param's last four bytes: the ctypes mirror's reserved5 is where x265amd_param_default now writes 0.05f"""
    lib = T.load_hip(8).lib
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    assert prm.reserved5 == float_bits(0.05) and T.EncParam.reserved5.offset + 4 == C.sizeof(T.EncParam)
    assert prm.recursionSkipMode == 1


@pytest.mark.needs_ref
def test_layout_of_the_new_member_matches_reference_header():
    ref_src = os.path.join(T.REF_DIR, "include")
    if not os.path.isdir(ref_src):
        pytest.skip("oracle/_ref/include (the reference's headers) is not built")
    cmd = ["g++", "-std=gnu++11", "-fsyntax-only", "-I" + os.path.join(T.REF_DIR, "cfg"), "-I" + ref_src, "-I" + os.path.join(T.PKG_DIR, "host"),
           os.path.join(T.ROOT, "tests", "native", "abi_layout_rskip_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _api(depth):
    import test_x265_api_abi as A
    lib = A.table(depth)
    return A, lib, A._fns(lib, depth)


def _threshold_offset():
    for line in open(os.path.join(T.PKG_DIR, "host", "x265_abi_layout_rskip.h")):
        if line.startswith("#define X265ABI_PARAM_edgeVarThreshold"):
            return int(line.split()[2])
    raise AssertionError("x265_abi_layout_rskip.h: no offset")


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref (the reference build) is not present")
def test_param_parse_of_the_threshold_matches_the_references():
    """x265_param_parse("rskip-edge-threshold", V) through our table against the reference library's own: the same return code, the same float (bit for bit: V / 100.0f),
    the same other members; "rskip" 2 likewise"""
    import test_x265_api_abi as A
    R, f = A._reference_api(), A._fns(A.table(8))
    off = _threshold_offset()
    bits = lambda p: bytes((C.c_ubyte * 4).from_address(p + off))
    a, b = R.x265_param_alloc(), f["alloc"]()
    R.x265_param_default_preset(a, b"medium", None); f["preset"](b, b"medium", None)
    assert bits(a) == bits(b) == struct.pack("<f", 0.05)
    for value in ("0", "5", "37", "100", "x"):
        ra, rb = R.x265_param_parse(a, b"rskip-edge-threshold", value.encode()), f["parse"](b, b"rskip-edge-threshold", value.encode())
        assert ra == rb, (value, ra, rb)
        assert bits(a) == bits(b), (value, bits(a), bits(b))
        assert A._members(a) == A._members(b), value
    assert R.x265_param_parse(a, b"rskip", b"2") == f["parse"](b, b"rskip", b"2") == 0 and A._members(a) == A._members(b)
    R.x265_param_free(a); f["free"](b)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(CASES))
def test_rskip_edge_command_lines(tag, tmp_path):
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
    print(tag, "stream", len(got), md5, "reference", g["stream_bytes"], g["stream_md5"], "others", g["other_stream_md5"])
    for k in range(n):
        assert hashlib.md5(rec[k * fsz:(k + 1) * fsz].tobytes()).hexdigest() == g["recon_md5"][k], "reconstruction of picture %d in display order" % k
    assert len(got) == g["stream_bytes"] and md5 == g["stream_md5"]


@pytest.mark.gpu
def test_rskip_edge_through_the_library():
    """x265amd_encoder_open with recursionSkipMode 2 (the threshold as x265amd_param_default left it): the bytes of `--preset medium --rskip 2`"""
    g = json.load(open(GOLD_PATH))[LIB_TAG]
    (w, h), n, depth, _, _ = CASES[LIB_TAG]
    stream, coded = T.encoder_run(T.load_hip(depth), case_frames(LIB_TAG), w, h, **dict(T.PRESET_BASE, recursionSkipMode=2))
    assert len(coded) == n
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream.tobytes()).hexdigest() == g["stream_md5"]


@pytest.mark.gpu
def test_rskip_edge_through_the_api_table():
    """x265_api_get_209: param_default_preset + param_parse("rskip", "2") + param_parse("rskip-edge-threshold", "5") + encoder_open + encoder_encode give the same bytes"""
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
    for name, value in ((b"input-res", b"%dx%d" % (w, h)), (b"fps", b"30/1"), (b"sar", b"1"), (b"rskip", b"2"), (b"rskip-edge-threshold", b"5"), (b"no-info", None)):
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


def _open_refused(word, base=None, **fields):
    lib = T.load_hip(8).lib
    lib.x265amd_encoder_open.restype = C.c_void_p
    lib.x265amd_encoder_open.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight = 128, 128
    for k, v in dict(T.PRESET_RC if base is None else base, **fields).items():
        setattr(prm, k, v)
    enc = lib.x265amd_encoder_open(C.byref(prm))
    if enc:
        lib.x265amd_encoder_close.argtypes = [C.c_void_p]
        lib.x265amd_encoder_close(enc)
    assert not enc and word in lib.x265amd_last_error(), lib.x265amd_last_error()


@pytest.mark.gpu
def test_what_is_refused_round_the_edge_based_recursion_skip():
    _open_refused(b"recursionSkipMode", recursionSkipMode=3)
    _open_refused(b"edgeVarThreshold", recursionSkipMode=2, reserved5=float_bits(1.5))
    _open_refused(b"edgeVarThreshold", recursionSkipMode=2, reserved5=float_bits(-0.01))
    _open_refused(b"recursionSkipMode", recursionSkipMode=2, aqMode=4)          # under the preset's rate control: the reference reads the filtered edge picture there
    _open_refused(b"recursionSkipMode", recursionSkipMode=2, shardCount=2, shardRank=0, frameNumThreads=2)


@pytest.mark.gpu
def test_what_opens_round_the_edge_based_recursion_skip():
    """constant QP switches adaptive quantisation off before the refusal looks (Encoder::configure's rule): aqMode 4 with rskip 2 then opens; a threshold outside 0 .. 1
    is not looked at under rskip 1"""
    lib = T.load_hip(8).lib
    lib.x265amd_encoder_open.restype = C.c_void_p
    lib.x265amd_encoder_open.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_encoder_close.argtypes = [C.c_void_p]
    lib.x265amd_last_error.restype = C.c_char_p
    for fields in (dict(rateControlMode=1, qp=30, aqMode=4, recursionSkipMode=2), dict(T.PRESET_RC, recursionSkipMode=1, reserved5=float_bits(1.5)),
                   dict(T.PRESET_RC, recursionSkipMode=2, reserved5=float_bits(1.0)), dict(T.PRESET_RC, recursionSkipMode=2, reserved5=float_bits(0.0))):
        prm = T.EncParam()
        lib.x265amd_param_default(C.byref(prm))
        prm.sourceWidth, prm.sourceHeight = 128, 128
        for k, v in fields.items():
            setattr(prm, k, v)
        enc = lib.x265amd_encoder_open(C.byref(prm))
        assert enc, (fields, lib.x265amd_last_error())
        lib.x265amd_encoder_close(enc)
