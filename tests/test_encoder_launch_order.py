"""The start rule (x265-amod_amd/host/launch_plan.cpp) inside the encoder object: pictures of the reference chain that start ahead of their turn behind a running I
picture change nothing in the stream, and they do start.

The clip is the 416x240 `--preset medium` case of tests/golden/encoder_preset_golden.json (30 pictures, a scene change at 24), coded with frameNumThreads = 5, the B
pyramid and three references as the bench codes its clip.  416x240 is enough: the lookahead hands the first pictures over when 20-odd have come in, the I picture at the
head then runs for tens of milliseconds, and the remaining pictures arrive and are typed within that time -- more of them than start in turn (at this size the encoder's
own count of pictures in turn is 17, the clip has 30), with the I picture still at the head, which is the rule's case: five referenced pictures started ahead of their
turn when this was written.  The counters of x265amd_encoder_stats (out[31], out[32]) say that it acted; the test fails with the
rule idle."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import hevc_testlib as T

PRESET_GOLD = os.path.join(T.GOLDEN_DIR, "encoder_preset_golden.json")
TAG = "crf_wqvga_medium_30/"


def encode_with_stats(L, frames, w, h, **cfg):
    """open -> encode every frame -> flush -> x265amd_encoder_stats -> close; returns (stream, the 33 words)"""
    lib = L.lib
    lib.x265amd_encoder_open.restype = C.c_void_p
    lib.x265amd_encoder_open.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_encoder_headers.argtypes = [C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32)]
    lib.x265amd_encoder_encode.argtypes = [C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32), C.POINTER(T.EncPicture), C.POINTER(T.EncPicture)]
    lib.x265amd_encoder_close.argtypes = [C.c_void_p]
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_encoder_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight = w, h
    for k, v in cfg.items():
        assert hasattr(prm, k), k
        setattr(prm, k, v)
    enc = lib.x265amd_encoder_open(C.byref(prm))
    assert enc, lib.x265amd_last_error()
    stream = bytearray()
    nal = C.POINTER(T.EncNal)(); nnal = C.c_uint32(0)
    try:
        assert lib.x265amd_encoder_headers(enc, C.byref(nal), C.byref(nnal)) > 0
        for i in range(nnal.value):
            stream += bytes(nal[i].payload[:nal[i].sizeBytes])
        coded = 0
        for planes in list(frames) + [None] * (len(frames) + 1):
            pic = None
            if planes is not None:
                keep = [np.ascontiguousarray(pl) for pl in planes]
                pic = T.EncPicture()
                for k in range(3):
                    pic.planes[k] = keep[k].ctypes.data; pic.stride[k] = keep[k].strides[0]
            ret = lib.x265amd_encoder_encode(enc, C.byref(nal), C.byref(nnal), C.byref(pic) if pic is not None else None, None)
            assert ret >= 0, lib.x265amd_last_error()
            if ret:
                coded += 1
                for i in range(nnal.value):
                    stream.extend(bytes(nal[i].payload[:nal[i].sizeBytes]))
            elif planes is None:
                break
        assert coded == len(frames)
        words = np.full(34, 0x5a5a, np.uint64)
        assert lib.x265amd_encoder_stats(enc, words.ctypes.data, 33) == 0 and words[33] == 0x5a5a
        short = np.full(34, 0x5a5a, np.uint64)
        assert lib.x265amd_encoder_stats(enc, short.ctypes.data, 31) == 0 and (short[31:] == 0x5a5a).all() and np.array_equal(short[:31], words[:31])
    finally:
        lib.x265amd_encoder_close(enc)
    return np.frombuffer(bytes(stream), np.uint8), words


@pytest.mark.gpu
def test_chain_pictures_start_ahead_of_their_turn_and_the_stream_stays():
    g = json.load(open(PRESET_GOLD))[TAG]
    (w, h), n, depth, cfg_id, cfg, _ = T.PRESET_CASES[TAG]
    cfg = dict(cfg, frameNumThreads=5, bBPyramid=1, maxNumReferences=3)
    stream, words = encode_with_stats(T.load_hip(depth), T.full_case_frames(TAG), w, h, **cfg)
    print("pictures I / P / B: %d / %d / %d; started ahead of their turn: %d referenced, %d leaf b" % (words[0], words[1], words[2], words[31], words[32]))
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream.tobytes()).hexdigest() == g["stream_md5"], "the stream is the reference's, byte for byte"
    assert int(words[0] + words[1] + words[2]) == n
    assert words[31] > 0, "no referenced picture started ahead of its turn: the rule under test did not act"
    assert words[32] == 0, "leaf b pictures start ahead of their turn only in pictures of more than 24 CTU rows"
