"""Device job queues (x265-amod_amd/csrc/xa_queue.h, device_queue.hip): the CTU rows of the encoder object run their block operations as commands to
resident workgroups instead of kernel launches.  The transport must not change a byte: the end-to-end streams of tests/test_encoder_api.py run through
the queues by default; here the transport itself is exercised, and one configuration is repeated with the queues switched off (X265AMD_QUEUES=0, in a
child process because the switch is read once) so that both paths stay pinned to the reference encoder's bytes."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import hevc_testlib as T


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_queue_selftest(depth):
    L = T.load_hip(depth)
    # copies through the BAR ring, rectangle copies, fills, deferred copies to pageable memory: 24 queues hammered by 24 host threads
    L.lib.x265amd_last_error.restype = C.c_char_p
    assert L.lib.x265amd_queue_selftest(400, 24) == 0, L.lib.x265amd_last_error().decode()
    # again: the server generation ended with the last release and starts anew
    assert L.lib.x265amd_queue_selftest(50, 3) == 0, L.lib.x265amd_last_error().decode()


@pytest.mark.gpu
def test_a_wait_that_gives_up_poisons_its_owner_only():
    """XA_OP_WAIT bounds its wait (two seconds); a queue whose wait gave up runs nothing more and fails every host wait -- for the owner it happened to: released and handed out
    again (the resident kernel still running) the queue starts clean (XA_CMD_RESET, csrc/device_queue.hip: xa_queue_clear_fault)"""
    L = T.load_hip(8)
    L.lib.x265amd_last_error.restype = C.c_char_p
    assert L.lib.x265amd_queue_selftest_wait_fault() == 0, L.lib.x265amd_last_error().decode()
    assert L.lib.x265amd_queue_selftest(20, 4) == 0, L.lib.x265amd_last_error().decode()


@pytest.mark.gpu
def test_stream_path_still_reproduces_reference_stream():
    env = dict(os.environ, X265AMD_QUEUES="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(T.ROOT, "tests", "test_encoder_api.py"),
                        "-k", "sao_bframes or wpp/ or hbd_wpp"], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# The path selectors of csrc/xa_env.h, each on the side the defaults do not take (X265AMD_QUEUES=0 and X265AMD_CHAIN_64=1 have tests of their own: above, and
# tests/test_encoder_full_size.py).  name -> (value, clips, what X265AMD_TIMING=1 must then report).  Clips: wvga/ (EDGE_CONFIGS: 832x480, 5 pictures, I + P + B, SAO and
# wavefronts, the last CTU row cut) for the chains, the fused search and the searches ahead; opt_p/ beside it for the quantiser's switch (the smallest case of the same golden
# file with rdoq-level 2 and wavefronts: wvga/ has no RDOQ); ft_b/ (FT_CASES: 256x448, 8 pictures, three frame threads) for the filters' switch, which only pictures coded in
# parallel read (x265amd_encoder::runFrameParallel).  "defaults": the same clips with nothing set, where every counter the other cases expect at zero must count.
SELECTORS_OFF = {
    "defaults": (None, ["wvga/", "ft_b/"], dict(chains=True, ahead=True, filter_units=True)),
    "X265AMD_INTRA_CHAIN": ("0", ["wvga/"], {}),
    "X265AMD_INTER_CHAIN": ("0", ["wvga/"], dict(chains=False)),
    "X265AMD_FUSED_SEARCH": ("0", ["wvga/"], dict(chains=True, ahead=False)),
    "X265AMD_DEVICE_RDOQ": ("0", ["wvga/", "opt_p/"], {}),
    "X265AMD_SEARCH_AHEAD": ("0", ["wvga/"], dict(chains=True, ahead=False)),
    "X265AMD_FILTER_COLS": ("0", ["wvga/", "ft_b/"], dict(filter_units=False)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SELECTORS_OFF))
def test_path_selectors_other_side_reproduces_reference_stream(name):
    """A selector that localises a stream mismatch must itself give the reference's stream on both sides, and must be read: the child runs with X265AMD_TIMING=1 and the
    counters it prints ("skip chains so far", "searches started ahead so far", the column filters' "filter units of poc") show that the path was taken or left.  The
    switches are read once per process: a child process per setting."""
    import re
    value, tags, expect = SELECTORS_OFF[name]
    code = ("import sys; sys.path.insert(0, %r); import numpy as np, hevc_testlib as T, test_encoder_api as E\n"
            "for tag in %r:\n"
            "    if tag in T.FT_CASES:\n"
            "        g = np.load(E.FT_GOLD); (w, h), n, depth, _, cfg, _ = T.FT_CASES[tag]; frames = T.encoder_ft_frames(tag)\n"
            "    else:\n"
            "        g = np.load(E.EDGE_GOLD); (w, h), n, cfg = E.EDGE_CONFIGS[tag]; frames = T.encoder_api_clip(tag, w, h, n, 8)\n"
            "    stream, coded = T.encoder_run(T.load_hip(8), frames, w, h, **cfg)\n"
            "    assert len(coded) == n and not T.stream_diff(stream, g[tag + 'stream']), (tag, T.stream_diff(stream, g[tag + 'stream']))\n"
            "    print('same stream', tag)\n") % (os.path.dirname(os.path.abspath(__file__)), tags)
    env = dict(os.environ, X265AMD_TIMING="1")
    if value is not None:
        env[name] = value
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and all("same stream " + t in r.stdout for t in tags), r.stdout[-1500:] + r.stderr[-3000:]
    chains = [int(m.group(1)) for m in re.finditer(r"skip chains so far: (\d+) commands", r.stderr)]
    ahead = [int(m.group(1)) + int(m.group(2)) for m in re.finditer(r"searches started ahead so far: (\d+) beside a leaf's merge check, (\d+) behind", r.stderr)]
    print(name, "chains", max(chains, default=None), "ahead", max(ahead, default=None), "filter units lines", r.stderr.count("filter units of poc"))
    if "chains" in expect:
        assert chains and (max(chains) > 0) == expect["chains"], chains[-3:]
    if "ahead" in expect:
        assert ahead and (max(ahead) > 0) == expect["ahead"], ahead[-3:]
    if "filter_units" in expect:
        assert ("filter units of poc" in r.stderr) == expect["filter_units"]


def test_selftest_symbol_is_exported():
    assert hasattr(C.CDLL(T.hip_path(8)), "x265amd_queue_selftest")


@pytest.mark.gpu
def test_repeated_encodes_are_identical():
    """the same clip eight times in one process (warm buffer pools, the job server restarted between pictures): every stream must be the reference
    encoder's.  A transport fault shows here as an occasional different stream -- a command slot accepted half written did exactly that once."""
    import hashlib
    import numpy as np
    import test_encoder_api as E
    g = np.load(E.EDGE_GOLD)
    tag = "wvga/"
    (w, h), n, cfg = E.EDGE_CONFIGS[tag]
    want = hashlib.md5(g[tag + "stream"].tobytes()).hexdigest()
    clip = T.encoder_api_clip(tag, w, h, n, 8)
    L = T.load_hip(8)
    for r in range(8):
        stream, _ = T.encoder_run(L, clip, w, h, **cfg)
        assert hashlib.md5(stream.tobytes()).hexdigest() == want, "run %d" % r
