"""--hist-scenecut through the encoder: the command line program, the library's own interface and the x265_api table give the reference program's bytes for the same
arguments (tests/golden/encoder_hist_scenecut_golden.json, cut by tests/golden/make_hist_scenecut_golden.py, which ASSERTS the relations between the reference's own
streams that make each case worth having); what stays refused under the option is refused by name."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import hevc_testlib as T

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "encoder_hist_scenecut_golden.json")
CLI = os.path.join(T.PKG_DIR, "bin", "x265amd")

# clip -> (size, pictures, the pictures at which the reference's histogram detector reports a scene change: `Scene Change in Pic Number#` of its debug log)
CLIPS = {
    "two_cuts": ((416, 240), 18, [6, 8]),          # the content changes at 6 and at 8: the cost-based detector places one I picture, this one two
    "step": ((420, 236), 14, [6]),                 # luma steps up by 25 at picture 6 (coded size 424 x 240): only the histogram detector cuts
    "flash": ((416, 240), 16, []),                 # one other picture at 6: a flash, no cut (the cost-based detector cuts)
    "fade": ((416, 240), 16, []),                  # luma fades from picture 5 on: no change logged, yet the stream differs from both others (scenecut()'s side effects are absent)
    "small": ((320, 192), 16, [6]),                # NUM64x64INPIC is 0: zero thresholds; the content changes at 7, the reference reports 6
}


def clip_frames(clip):
    (w, h), n, _ = CLIPS[clip]
    if clip == "two_cuts":
        return T.scene_clip(w, h, n, [6, 8])
    if clip == "flash":
        return T.scene_clip(w, h, n, [6, 7])
    if clip == "small":
        return T.scene_clip(w, h, n, [7])
    frames = T.scene_clip(w, h, n, [])
    for t, fr in enumerate(frames):
        y = fr[0].astype(np.int64)
        if clip == "step":
            y = y + (25 if t >= 6 else 0)
        else:
            y = np.floor(y * (1 - 0.06 * max(0, t - 4))).astype(np.int64)
        fr[0] = np.clip(y, 0, 255).astype(np.uint8)
    return frames


HS = ["--preset", "medium", "--hist-scenecut"]
# tag -> (clip, the command line; T.PRESET_CLI follows it)
CASES = {
    "two_cuts/": ("two_cuts", HS),
    "two_cuts_scenecut0/": ("two_cuts", HS + ["--scenecut", "0"]),               # a detected change places no I picture: the --scenecut 0 stream
    "step/": ("step", HS),
    "flash/": ("flash", HS),
    "fade/": ("fade", HS),
    "small/": ("small", HS),
    "two_cuts_no_b/": ("two_cuts", HS + ["--bframes", "0", "--lookahead-slices", "0"]),          # histBasedScenecut analyses nothing without B pictures
    "two_cuts_frame_threads/": ("two_cuts", HS + ["--frame-threads", "3", "--pools", "4"]),
    "two_cuts_keyint_open/": ("two_cuts", HS + ["--keyint", "-1"]),               # Encoder::configure clears the option: the stream of --keyint -1 alone
    "two_cuts_zerolatency/": ("two_cuts", ["--preset", "medium", "--hist-scenecut", "--tune", "zerolatency"]),          # the tune clears it
}
# the reference's streams each case is held against by the generator: name -> (command line, "differs" / "equals")
RELATIONS = {
    "two_cuts/": {"plain": (["--preset", "medium"], "differs"), "scenecut0": (["--preset", "medium", "--scenecut", "0"], "differs")},
    "two_cuts_scenecut0/": {"scenecut0": (["--preset", "medium", "--scenecut", "0"], "equals")},
    "step/": {"plain": (["--preset", "medium"], "differs")},
    "flash/": {"plain": (["--preset", "medium"], "differs"), "scenecut0": (["--preset", "medium", "--scenecut", "0"], "equals")},
    "fade/": {"plain": (["--preset", "medium"], "differs"), "scenecut0": (["--preset", "medium", "--scenecut", "0"], "differs")},
    "small/": {"plain": (["--preset", "medium"], "differs")},
    "two_cuts_no_b/": {},
    "two_cuts_frame_threads/": {"default": (HS, "equals")},
    "two_cuts_keyint_open/": {"plain": (["--preset", "medium", "--keyint", "-1"], "equals")},
    "two_cuts_zerolatency/": {"plain": (["--preset", "medium", "--tune", "zerolatency"], "equals")},
}
LIB_TAG = "two_cuts/"


def write_y4m(path, frames, w, h):
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420\n" % (w, h))
        for fr in frames:
            f.write(b"FRAME\n")
            for pl in fr:
                f.write(np.ascontiguousarray(pl).tobytes())


def test_fixtures_present_and_complete():
    g = json.load(open(GOLD_PATH))
    assert sorted(g) == sorted(CASES) == sorted(RELATIONS)
    for tag, (clip, cli) in CASES.items():
        n = CLIPS[clip][1]
        assert len(g[tag]["recon_md5"]) == n and g[tag]["reference_command_line"] == " ".join(cli + T.PRESET_CLI), tag
        assert len(g[tag]["stream_md5"]) == 32 and g[tag]["stream_bytes"] > 0, tag
        for name, (_, how) in RELATIONS[tag].items():
            assert (g[tag]["other_stream_md5"][name] == g[tag]["stream_md5"]) == (how == "equals"), (tag, name)
    # the I pictures of the two-cut clip: where the histogram detector reports, and only one of them without it
    assert g["two_cuts/"]["i_pictures"] == [0, 6, 8] and g["step/"]["i_pictures"] == [0, 6] and g["flash/"]["i_pictures"] == [0] and g["fade/"]["i_pictures"] == [0]
    assert g["two_cuts_no_b/"]["i_pictures"] == [0]


def test_param_slot_keeps_its_place():
    """x265amd_param.bHistBasedSceneCut is the four bytes the ctypes mirror still calls reserved2, 0 by default"""
    lib = T.load_hip(8).lib
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    assert prm.reserved2 == 0 and T.EncParam.reserved2.offset == T.EncParam.bRepeatHeaders.offset + 4 == T.EncParam.vuiSarWidth.offset - 4


def test_layout_of_the_member_in_both_headers():
    """tests/native/abi_layout_hist_check.cpp: the slot's place in x265amd_param, and -- where the reference's headers are built -- the offset x265_api_abi.cpp reads
    x265_param.bHistBasedSceneCut at"""
    ref_src = os.path.join(T.REF_DIR, "include")
    cmd = ["g++", "-std=gnu++11", "-fsyntax-only", "-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.PKG_DIR, "host")]
    if os.path.isdir(ref_src):
        cmd += ["-DWITH_REFERENCE_HEADER", "-I" + os.path.join(T.REF_DIR, "cfg"), "-I" + ref_src]
    r = subprocess.run(cmd + [os.path.join(T.ROOT, "tests", "native", "abi_layout_hist_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_host_half_under_the_sanitizers(tmp_path):
    """tests/native/hist_scenecut_check.cpp: a stand-alone program (host code only) that runs the model, finish and change on planes of its own under
    -fsanitize=address,undefined"""
    exe = str(tmp_path / "hist_scenecut_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DX265AMD_DEPTH=8", "-I" + os.path.join(T.ROOT, "include"),
           os.path.join(T.ROOT, "tests", "native", "hist_scenecut_check.cpp"), os.path.join(T.PKG_DIR, "host", "hist_scenecut.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def _api(depth):
    import test_x265_api_abi as A
    lib = A.table(depth)
    return A, lib, A._fns(lib, depth)


def test_the_table_no_longer_refuses_the_member_by_name():
    """x265_param_parse knows the word, and with the member set x265_encoder_open's first complaint is no longer about it (the next refusal is about something else:
    lossless coding, asked for here so that nothing touches a device)"""
    A, lib, f = _api(8)
    lib.x265amd_last_error.restype = C.c_char_p
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0
    assert f["parse"](p, b"hist-scenecut", None) == 0 and A._members(p)["bHistBasedSceneCut"] == 1
    assert f["parse"](p, b"no-hist-scenecut", None) == 0 and A._members(p)["bHistBasedSceneCut"] == 0
    assert f["parse"](p, b"hist-scenecut", b"1") == 0 and f["parse"](p, b"lossless", None) == 0
    assert f["parse"](p, b"input-res", b"128x128") == 0
    enc = f["open"](p)
    assert not enc and b"lossless" in lib.x265amd_last_error() and b"bHistBasedSceneCut" not in lib.x265amd_last_error(), lib.x265amd_last_error()
    f["free"](p)


@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref (the reference build) is not present")
def test_param_parse_of_the_switch_matches_the_references():
    """x265_param_parse("hist-scenecut") / ("no-hist-scenecut") through our table against the reference library's own: return code and every member; --tune zerolatency
    clears the member in both"""
    import test_x265_api_abi as A
    R, f = A._reference_api(), A._fns(A.table(8))
    a, b = R.x265_param_alloc(), f["alloc"]()
    R.x265_param_default_preset(a, b"medium", None); f["preset"](b, b"medium", None)
    for name, value, want in ((b"hist-scenecut", None, 1), (b"no-hist-scenecut", None, 0), (b"hist-scenecut", b"1", 1), (b"hist-scenecut", b"0", 0), (b"hist_scenecut", b"true", 1),
                              (b"no-hist-scenecut", b"1", 0)):
        ra, rb = R.x265_param_parse(a, name, value), f["parse"](b, name, value)
        assert ra == rb == 0, (name, value, ra, rb)
        assert A._members(a) == A._members(b) and A._members(b)["bHistBasedSceneCut"] == want, (name, value)
    R.x265_param_parse(a, b"hist-scenecut", None); f["parse"](b, b"hist-scenecut", None)
    R.x265_param_default_preset(a, b"medium", b"zerolatency"); f["preset"](b, b"medium", b"zerolatency")
    assert A._members(a) == A._members(b) and A._members(b)["bHistBasedSceneCut"] == 0
    R.x265_param_free(a); f["free"](b)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(CASES))
def test_hist_scenecut_command_lines(tag, tmp_path):
    """the stream and every reconstructed picture equal the reference program's for the SAME arguments"""
    g = json.load(open(GOLD_PATH))[tag]
    clip, cli = CASES[tag]
    (w, h), n, _ = CLIPS[clip]
    write_y4m(tmp_path / "clip.y4m", clip_frames(clip), w, h)
    cmd = [CLI, "--input", str(tmp_path / "clip.y4m"), "-o", str(tmp_path / "out.hevc"), "--recon", str(tmp_path / "rec.yuv")] + cli + T.PRESET_CLI
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.fromfile(tmp_path / "out.hevc", np.uint8)
    rec = np.fromfile(tmp_path / "rec.yuv", np.uint8)
    fsz = w * h * 3 // 2
    assert len(rec) == n * fsz
    md5 = hashlib.md5(got.tobytes()).hexdigest()
    print(tag, "stream", len(got), md5, "reference", g["stream_bytes"], g["stream_md5"], "others", g["other_stream_md5"])
    for k in range(n):
        assert hashlib.md5(rec[k * fsz:(k + 1) * fsz].tobytes()).hexdigest() == g["recon_md5"][k], "reconstruction of picture %d in display order" % k
    assert len(got) == g["stream_bytes"] and md5 == g["stream_md5"]


@pytest.mark.gpu
def test_hist_scenecut_through_the_library():
    """x265amd_encoder_open with bHistBasedSceneCut 1 (the ctypes mirror's reserved2): the bytes of `--preset medium --hist-scenecut`"""
    g = json.load(open(GOLD_PATH))[LIB_TAG]
    (w, h), n, _ = CLIPS[CASES[LIB_TAG][0]]
    stream, coded = T.encoder_run(T.load_hip(8), clip_frames(CASES[LIB_TAG][0]), w, h, **dict(T.PRESET_BASE, reserved2=1))
    assert len(coded) == n
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream.tobytes()).hexdigest() == g["stream_md5"]


@pytest.mark.gpu
def test_hist_scenecut_through_the_api_table():
    """x265_api_get_209: param_default_preset + param_parse("hist-scenecut") + encoder_open + encoder_encode give the same bytes"""
    g = json.load(open(GOLD_PATH))[LIB_TAG]
    (w, h), n, _ = CLIPS[CASES[LIB_TAG][0]]
    A, lib, f = _api(8)
    api = f["api"]
    lib.x265amd_last_error.restype = C.c_char_p
    headers = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32))(api.fn[14])
    encode = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p)(api.fn[15])
    close = C.CFUNCTYPE(None, C.c_void_p)(api.fn[18])
    pic_alloc = C.CFUNCTYPE(C.c_void_p)(api.fn[7]); pic_init = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)(api.fn[9])
    frames = clip_frames(CASES[LIB_TAG][0])
    p = f["alloc"]()
    assert f["preset"](p, b"medium", None) == 0
    for name, value in ((b"input-res", b"%dx%d" % (w, h)), (b"fps", b"30/1"), (b"sar", b"1"), (b"hist-scenecut", None), (b"no-info", None)):
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


def _open(depth, **fields):
    lib = T.load_hip(depth).lib
    lib.x265amd_encoder_open.restype = C.c_void_p
    lib.x265amd_encoder_open.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_encoder_close.argtypes = [C.c_void_p]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight = 128, 128
    for k, v in dict(T.PRESET_RC, **fields).items():
        setattr(prm, k, v)
    enc = lib.x265amd_encoder_open(C.byref(prm))
    if enc:
        lib.x265amd_encoder_close(enc)
    return bool(enc), lib.x265amd_last_error()


@pytest.mark.gpu
def test_what_is_refused_under_the_option():
    for depth, fields in ((10, dict(reserved2=1)), (8, dict(reserved2=1, shardCount=2, shardRank=0, frameNumThreads=2))):
        opened, why = _open(depth, **fields)
        assert not opened and b"bHistBasedSceneCut" in why, (depth, fields, why)


@pytest.mark.gpu
def test_what_opens_round_the_option():
    """the 8-bit library opens with it; the 10-bit library opens where Encoder::configure's rules clear it first (keyframeMax -1, all-intra)"""
    for depth, fields in ((8, dict(reserved2=1)), (8, dict(reserved2=1, scenecutThreshold=0)), (10, dict(reserved2=1, keyframeMax=-1)), (10, dict(reserved2=1, keyframeMax=1))):
        opened, why = _open(depth, **fields)
        assert opened, (depth, fields, why)
