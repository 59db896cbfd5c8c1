"""--me full through the encoder: the command line program and the library's own interface give the reference program's bytes for the same arguments
(tests/golden/encoder_me_full_golden.json, cut by tests/golden/make_me_full_golden.py); umh and sea stay refused by name."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import hevc_testlib as T
import test_hip_me_full as MF

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "encoder_me_full_golden.json")
CLI = os.path.join(os.path.dirname(T.GOLDEN_DIR), "..", "x265-amod_amd", "bin", "x265amd")

# tag -> (size, pictures, depth, survey_clip's configuration, the command line behind the file names; T.PRESET_CLI follows it)
CASES = {
    # P and B pictures, frame threads, CTUs cut right and below
    "me_full_medium_wqvga/": ((416, 240), 8, 8, 2, ["--preset", "medium", "--me", "full", "--merange", "16"]),
    # rect partitions, four references, chroma SATD, RDOQ
    "me_full_slow_hbd/": ((192, 128), 6, 10, 4, ["--preset", "slow", "--me", "full", "--merange", "12", "--subme", "4"]),
    # areas larger than the staged window; mvmin / mvmax clipped at all four picture edges
    "me_full_merange57/": ((128, 128), 3, 8, 2, ["--preset", "medium", "--me", "full", "--merange", "57", "--frame-threads", "1", "--no-wpp", "--bframes", "0", "--qp", "30"]),
}
ABI_TAG = "me_full_medium_wqvga/"


def _write_y4m(path, frames, w, h, depth):
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
    gold = np.load(MF.GOLD_PATH)
    for depth in (8, 10):
        sets = MF.golden_sets(depth)
        for key, (_, jobs, _) in sets.items():
            assert key in gold.files and gold[key].shape == (len(jobs), 3) and gold[key].dtype == np.int32, key
    assert sorted(gold.files) == sorted(list(MF.golden_sets(8)) + list(MF.golden_sets(10)))


@pytest.mark.parametrize("depth", [8, 10])
def test_me_full_golden_is_the_reference(depth):
    """cut again through the reference's MotionEstimate (oracle/_ref), the committed results come out"""
    ref, gold = T.load_ref(depth), np.load(MF.GOLD_PATH)
    for key, (planes, jobs, chroma) in MF.golden_sets(depth).items():
        assert np.array_equal(MF.cut(ref, planes, jobs, chroma), gold[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(CASES))
def test_me_full_command_lines(tag, tmp_path):
    """the stream and every reconstructed picture equal the reference program's for the SAME arguments"""
    g = json.load(open(GOLD_PATH))[tag]
    (w, h), n, depth, cfg_id, cli = CASES[tag]
    _write_y4m(tmp_path / "clip.y4m", T.survey_clip(w, h, depth, cfg_id, 0, n), w, h, depth)
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
def test_me_full_through_the_library():
    """x265amd_encoder_open with searchMethod 5: the bytes of `--preset medium --me full --merange 16`"""
    g = json.load(open(GOLD_PATH))[ABI_TAG]
    (w, h), n, depth, cfg_id, _ = CASES[ABI_TAG]
    stream, coded = T.encoder_run(T.load_hip(depth), T.survey_clip(w, h, depth, cfg_id, 0, n), w, h, **dict(T.PRESET_BASE, searchMethod=5, searchRange=16))         # (aspectRatioIdc 1, as the clip file's header says: A1:1)
    assert len(coded) == n
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream.tobytes()).hexdigest() == g["stream_md5"]


@pytest.mark.gpu
@pytest.mark.parametrize("method", [2, 4])
def test_umh_and_sea_are_still_refused(method):
    lib = T.load_hip(8).lib
    lib.x265amd_encoder_open.restype = C.c_void_p
    lib.x265amd_encoder_open.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight, prm.searchMethod = 128, 128, method
    enc = lib.x265amd_encoder_open(C.byref(prm))
    if enc:
        lib.x265amd_encoder_close.argtypes = [C.c_void_p]
        lib.x265amd_encoder_close(enc)
    assert not enc and b"searchMethod" in lib.x265amd_last_error()
