"""The edge-based adaptive quantisation modes (--aq-mode 4 / 5) below the encoder: x265amd_aq_edge (device), x265amd_aq_offsets_edge (host) and the angle function both
sides share (csrc/aq_edge_dev.h), against tests/golden/aq_edge_golden.npz -- cut by tests/golden/make_aq_edge_golden.py from the reference's own computeEdge
(libx265_ref{8,10}.so) and from whole reference encodes with their rate-control record (x265_rc_dump{8,10}).

Without a GPU: every gradient pair of both bit depths through the angle function against the reference's arithmetic (tests/native/aq_theta_check.cpp); the numpy model
of the picture pass (with the library's HOST angle function) against computeEdge's planes; the host half on the stored block arrays against the reference encoder's doubles.
On the GPU: the kernel's planes, block arrays and sums against the same fixture; the device's angle function against the host's; device + host against the encoder's doubles."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hevc_testlib as T

GOLD_PATH = os.path.join(T.GOLDEN_DIR, "aq_edge_golden.npz")
NATIVE = os.path.join(T.ROOT, "tests", "native", "aq_theta_check.cpp")

# ---- cases ----
# planes handed to computeEdge as they are (its refPic): name -> how plane_direct builds it.  Small noise amplitudes put the gradients' magnitudes around the threshold;
# the ramps give gradients on the axes and the diagonals (theta 0, 45, 90, 135, 180 exactly)
DIRECT = ["noise4", "noise16", "noise40", "noisefull", "ramp_x", "ramp_y", "ramp_diag", "ramp_anti", "steps"]
DIRECT_W, DIRECT_H = 48, 40
# whole pictures through Gaussian + Sobel + block sums.  The kernel's workgroup tile is 64 x 16 samples (4 x 1 blocks):
#   16x16   everything is border or next to it: no sample further than 2 from the edge but the middle 12x12, one block, three idle wavefronts
#   72x40   the right blocks (8 of 16 columns) and the bottom blocks (8 of 16 rows) hang over the edge; two tiles across, three down
#   200x72  four tiles across, five down: more than one workgroup tile in both directions, the last of each cut
PICTURES = [(16, 16), (72, 40), (200, 72)]
# the rate-control clip: T.survey_clip(w, h, depth, 2, 0, n); 120 and 200 are no multiples of 16
RC_CLIPS = {8: (208, 120, 4), 10: (200, 128, 4)}
RC_OPTS = {4: ["aq-mode=4", "cutree=0"], 5: ["aq-mode=5", "cutree=0"]}
RC_PRESET = "medium"
PAD = 32          # the margin the test puts round a source picture (blocks at the right and bottom edge read into it, as x265amd_aq_energy's header says)


def plane_direct(name, depth):
    rng = np.random.default_rng([depth, DIRECT.index(name)])
    pmax = (1 << depth) - 1
    sc = 1 << (depth - 8)
    yy, xx = np.mgrid[0:DIRECT_H, 0:DIRECT_W]
    if name.startswith("noise"):
        amp = pmax if name == "noisefull" else int(name[5:]) * sc
        p = rng.integers(0, amp + 1, (DIRECT_H, DIRECT_W)) + (0 if name == "noisefull" else 100 * sc)
    elif name == "ramp_x":
        p = xx * 5 * sc
    elif name == "ramp_y":
        p = (DIRECT_H - 1 - yy) * 6 * sc
    elif name == "ramp_diag":
        p = (xx + yy) * 2 * sc
    elif name == "ramp_anti":
        p = (xx - yy + DIRECT_H) * 2 * sc
    else:
        p = ((xx // 7 + yy // 5) % 2) * rng.integers(1, 60 * sc, (DIRECT_H, DIRECT_W)) + 20 * sc
    return np.clip(p, 0, pmax).astype(np.uint8 if depth == 8 else np.uint16)


def picture(w, h, depth):
    """noise on a gradient with a bright disc, a dark bar and a diagonal band: edges in every direction, flat areas, and texture right up to the border"""
    rng = np.random.default_rng([depth, w, h])
    sc = 1 << (depth - 8)
    yy, xx = np.mgrid[0:h, 0:w]
    p = 60 + xx // 2 + yy + rng.integers(-6, 7, (h, w))
    p = np.where((xx - w * 0.6) ** 2 + (yy - h * 0.5) ** 2 < (min(w, h) * 0.3) ** 2, 215 + rng.integers(-3, 4, (h, w)), p)
    p = np.where((xx > w // 5) & (xx < w // 5 + 5), 12, p)
    p = np.where(np.abs(xx - 2 * yy - w // 3) < 3, 180, p)
    return (np.clip(p, 0, 255) * sc + rng.integers(0, sc, (h, w))).astype(np.uint8 if depth == 8 else np.uint16)


# ---- the model: edgeFilter + computeEdge + edgeDensityCu in numpy, the angle from the library's host function ----
GAUSS = np.array([[2, 4, 5, 4, 2], [4, 9, 12, 9, 4], [5, 12, 15, 12, 5], [4, 9, 12, 9, 4], [2, 4, 5, 4, 2]], np.int64)


def host_angles(depth, gv, gh):
    lib = T.load_hip(depth).lib
    gv = np.ascontiguousarray(gv, np.int32).ravel(); gh = np.ascontiguousarray(gh, np.int32).ravel()
    theta = np.zeros(len(gv), np.int32); edge = np.zeros(len(gv), np.int32)
    if len(gv):
        assert lib.x265amd_aq_edge_angles(T._ptr(gv), T._ptr(gh), len(gv), T._ptr(theta), T._ptr(edge)) == 0
    return theta, edge


def gaussian(src):
    h, w = src.shape
    g = src.astype(np.int64).copy()
    if h > 4 and w > 4:
        acc = np.zeros((h - 4, w - 4), np.int64)
        for dy in range(5):
            for dx in range(5):
                acc += GAUSS[dy, dx] * src[dy:h - 4 + dy, dx:w - 4 + dx].astype(np.int64)
        g[2:h - 2, 2:w - 2] = acc // 159
    return g


def sobel(ref):
    """(gV, gH) of the samples one inside the plane's border"""
    r = ref.astype(np.int64)
    tl, tc, tr = r[:-2, :-2], r[:-2, 1:-1], r[:-2, 2:]
    ml, mr = r[1:-1, :-2], r[1:-1, 2:]
    bl, bc, br = r[2:, :-2], r[2:, 1:-1], r[2:, 2:]
    return -3 * tl - 10 * tc - 3 * tr + 3 * bl + 10 * bc + 3 * br, -3 * tl + 3 * tr - 10 * ml + 10 * mr - 3 * bl + 3 * br


def edge_planes(depth, ref, border):
    """computeEdge on `ref`: the edge picture (holding `border` where computeEdge does not write) and the angles"""
    h, w = ref.shape
    edge = border.astype(np.int64).copy(); theta = np.zeros((h, w), np.int64)
    if h > 2 and w > 2:
        gv, gh = sobel(ref)
        t, e = host_angles(depth, gv, gh)
        edge[1:-1, 1:-1] = e.reshape(h - 2, w - 2); theta[1:-1, 1:-1] = t.reshape(h - 2, w - 2)
    return edge, theta


def block_sums(edge, theta):
    """edgeDensityCu per 16x16 block (zeros beyond the picture): density, mean angle; and the edge picture's sum and sum of squares"""
    h, w = edge.shape
    bh, bw = (h + 15) // 16, (w + 15) // 16
    e = np.zeros((bh * 16, bw * 16), np.int64); t = np.zeros_like(e)
    e[:h, :w] = edge; t[:h, :w] = theta
    eb = e.reshape(bh, 16, bw, 16).transpose(0, 2, 1, 3).reshape(bh * bw, 256); tb = t.reshape(bh, 16, bw, 16).transpose(0, 2, 1, 3).reshape(bh * bw, 256)
    s, q = eb.sum(1), (eb * eb).sum(1)
    density = (q - ((s * s) >> 8)) & 0xffffffff
    return density.astype(np.uint32), (tb.sum(1) // 256).astype(np.uint32), np.array([s.sum(), q.sum()], np.uint64)


def model(depth, src):
    edge, theta = edge_planes(depth, gaussian(src), src)
    return (edge, theta) + block_sums(edge, theta)


def rc_frames(depth):
    w, h, n = RC_CLIPS[depth]
    return T.survey_clip(w, h, depth, 2, 0, n)


def padded(frame):
    """(flat Y|U|V with an edge-extended margin of PAD / PAD/2 samples, stride, cstride, the offsets of the three samples (0,0))"""
    parts, org, at = [], [], 0
    for k, pl in enumerate(frame):
        m = PAD if k == 0 else PAD // 2
        q = np.pad(pl, m, mode="edge")
        org.append(at + m * q.shape[1] + m); at += q.size
        parts.append(q.ravel())
    return np.concatenate(parts), frame[0].shape[1] + 2 * PAD, frame[1].shape[1] + PAD, org


def offsets_edge(depth, energy, density, angle, avg, mode, strength=1.0, bias=1.0, qg=16):
    lib = T.load_hip(depth).lib
    n = len(energy)
    a = np.zeros(n, np.float64); t = np.zeros(n, np.float64); f = np.zeros(n, np.int32)
    rc = lib.x265amd_aq_offsets_edge(T._ptr(np.ascontiguousarray(energy, np.uint32)), T._ptr(np.ascontiguousarray(density, np.uint32)), T._ptr(np.ascontiguousarray(angle, np.uint32)), n, avg, mode,
                                     C.c_double(strength), C.c_double(bias), qg, T._ptr(a), T._ptr(t), T._ptr(f))
    return rc, a, t, f


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD_PATH)


# ---- without a GPU ----
@pytest.mark.parametrize("depth", [8, 10])
def test_angle_function_equals_the_references_arithmetic_on_every_gradient_pair(depth, tmp_path):
    """zero differences allowed, in the angle and in the edge decision, over all 8161^2 (8 bits) / 32737^2 (10 bits) pairs; the program uses at most 16 threads"""
    exe = str(tmp_path / "aq_theta_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off", "-I", os.path.join(T.PKG_DIR, "csrc"), "-o", exe, NATIVE])
    r = subprocess.run([exe, str(depth)], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    n = 16 * ((1 << depth) - 1) * 2 + 1
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "pairs %d theta_diff 0 edge_diff 0" % (n * n), r.stdout[-3000:] + r.stderr[-1000:]


@pytest.mark.parametrize("depth", [8, 10])
def test_model_with_host_angles_equals_compute_edge(depth, gold):
    """the reference's own computeEdge (called when the fixture was cut) against Sobel in numpy + the library's host angle function: this ties the arithmetic the native
    check restates to the real binary.  Both every directly built plane and the whole pictures (where the Gaussian is the model's as well)"""
    for name in DIRECT:
        ref = plane_direct(name, depth)
        edge, theta = edge_planes(depth, ref, ref)
        assert np.array_equal(edge, gold["ce%d/%s/edge" % (depth, name)]), name
        assert np.array_equal(theta, gold["ce%d/%s/theta" % (depth, name)]), name
    seen = set()
    for name in DIRECT:
        seen |= set(np.unique(gold["ce%d/%s/theta" % (depth, name)]).tolist())
    assert {0, 45, 90, 135, 180} <= seen and len(seen) > 150          # the axes and diagonals are hit, and most degrees in between
    for w, h in PICTURES:
        edge, theta, density, angle, sums = model(depth, picture(w, h, depth))
        k = "pic%d/%dx%d/" % (depth, w, h)
        assert np.array_equal(edge, gold[k + "edge"]) and np.array_equal(theta, gold[k + "theta"]), k
        assert np.array_equal(density, gold[k + "density"]) and np.array_equal(angle, gold[k + "angle"]) and np.array_equal(sums, gold[k + "sums"]), k
        assert np.count_nonzero(density) * 2 >= len(density), k           # the pictures do have edges


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("mode", [4, 5])
def test_offsets_edge_equal_the_reference_encoders_doubles(depth, mode, gold):
    """x265amd_aq_offsets_edge on the stored energies, densities and angles: Lowres::qpAqOffset and invQscaleFactor of every picture of the reference's encode, identical as
    64-bit patterns"""
    w, h, n = RC_CLIPS[depth]
    avg = (((w // 2) + 7) >> 3) * (((h // 2) + 7) >> 3)
    inclined = 0
    for poc in range(n):
        k = "rc%d/m%d/p%d/" % (depth, mode, poc)
        rc, a, t, f = offsets_edge(depth, gold["rc%d/p%d/energy" % (depth, poc)], gold["rc%d/p%d/density" % (depth, poc)], gold["rc%d/p%d/angle" % (depth, poc)], avg, mode)
        assert rc == 0
        assert np.array_equal(a.view(np.uint64), gold[k + "qp_aq_offset"].view(np.uint64)), k
        assert np.array_equal(t.view(np.uint64), a.view(np.uint64)) and np.array_equal(f, gold[k + "inv_qscale"]), k
        ang = gold["rc%d/p%d/angle" % (depth, poc)]
        inclined += int(np.count_nonzero((gold["rc%d/p%d/density" % (depth, poc)] != 0) & (((ang >= 30) & (ang <= 60)) | ((ang >= 120) & (ang <= 150)))))
    assert inclined > 0           # the clip does have inclined blocks: the stronger branch is taken


def test_offsets_entries_keep_to_their_modes():
    e = np.full(4, 1000, np.uint32)
    a = np.zeros(4, np.float64); f = np.zeros(4, np.int32)
    lib = T.load_hip(8).lib
    assert lib.x265amd_aq_offsets(T._ptr(e), 4, 4, 4, C.c_double(1.0), C.c_double(1.0), 16, T._ptr(a), T._ptr(a), T._ptr(f)) == -1          # X265AMD_EINVAL: the edge modes have their own entry
    for mode in (3, 6):
        assert offsets_edge(8, e, e, e, 4, mode)[0] == -1
    assert offsets_edge(8, e, e, e, 4, 4, qg=8)[0] == -1


# ---- on the GPU ----
def run_edge(depth, src, planes=True, stride_extra=5):
    """x265amd_aq_edge on a picture (held with a stride wider than the picture and a guard of 0xa5 bytes round it that no sample may come from)"""
    import torch
    lib = T.load_hip(depth).lib
    h, w = src.shape
    stride = w + stride_extra
    host = np.full((h + 2, stride), 0xa5a5 if depth > 8 else 0xa5, src.dtype)
    host[1:h + 1, :w] = src
    d = torch.from_numpy(host.view(np.uint8)).cuda()
    nb = ((w + 15) // 16) * ((h + 15) // 16)
    d_den = torch.full((nb,), -1, dtype=torch.int32, device="cuda"); d_ang = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    start = np.array([5, 1 << 40], np.int64)
    d_wp = torch.from_numpy(start.copy()).cuda()
    tdt = torch.uint8 if depth == 8 else torch.int16
    d_e = torch.full((h * w,), 77, dtype=tdt, device="cuda"); d_t = torch.full((h * w,), 77, dtype=tdt, device="cuda")
    lib.x265amd_last_error.restype = C.c_char_p
    rc = lib.x265amd_aq_edge(None, C.c_uint64(d.data_ptr() + stride * src.itemsize), C.c_int64(stride), w, h, 16, C.c_void_p(d_den.data_ptr()), C.c_void_p(d_ang.data_ptr()),
                             C.c_void_p(d_wp.data_ptr()), C.c_uint64(d_e.data_ptr() if planes else 0), C.c_uint64(d_t.data_ptr() if planes else 0))
    assert rc == 0, lib.x265amd_last_error()
    torch.cuda.synchronize()
    view = lambda x: x.cpu().numpy().view(src.dtype).reshape(h, w)
    return view(d_e), view(d_t), d_den.cpu().numpy().view(np.uint32), d_ang.cpu().numpy().view(np.uint32), (d_wp.cpu().numpy() - start).astype(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", PICTURES)
def test_hip_aq_edge_matches_compute_edge(depth, size, gold):
    """the kernel's two planes against the reference's computeEdge (on the Gaussian picture), its block arrays and its additions to the two sums against the stored ones;
    and the same block arrays with no planes asked for.  (Tile: 64 x 16 samples -- 200x72 is 4 x 5 tiles, 72x40 cuts blocks right and below, 16x16 is one block.)"""
    w, h = size
    k = "pic%d/%dx%d/" % (depth, w, h)
    src = picture(w, h, depth)
    edge, theta, density, angle, sums = run_edge(depth, src)
    assert np.array_equal(edge, gold[k + "edge"]), np.argwhere(edge != gold[k + "edge"])[:8]
    assert np.array_equal(theta, gold[k + "theta"]), np.argwhere(theta != gold[k + "theta"])[:8]
    assert np.array_equal(density, gold[k + "density"]) and np.array_equal(angle, gold[k + "angle"])
    assert np.array_equal(sums, gold[k + "sums"]), (sums, gold[k + "sums"])
    e2, t2, density2, angle2, sums2 = run_edge(depth, src, planes=False, stride_extra=0)
    assert np.all(e2 == 77) and np.all(t2 == 77)
    assert np.array_equal(density2, density) and np.array_equal(angle2, angle) and np.array_equal(sums2, sums)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_device_angles_equal_the_hosts(depth, gold):
    """what the CPU tests cannot see: the device's arithmetic (double division, the conversions, no contraction) gives the host's bits.  A grid over the whole range of
    gradients, the axes and diagonals, and every coprime pair whose angle lies within one float ulp of a whole degree (found by the native check when the fixture was cut)"""
    import torch
    lib = T.load_hip(depth).lib
    gmax = 16 * ((1 << depth) - 1)
    near = gold["near_pairs"].astype(np.int64)
    near = near[(np.abs(near[:, 0]) <= gmax) & (np.abs(near[:, 1]) <= gmax)]
    assert len(near) > 500
    ax = np.unique(np.concatenate([np.arange(-gmax, gmax + 1, 37), np.arange(-40, 41), [-gmax, gmax]]))
    gv, gh = (a.ravel() for a in np.meshgrid(ax, ax, indexing="ij"))
    gv = np.concatenate([gv, near[:, 0], near[:, 0] * (gmax // np.maximum(1, np.abs(near).max(1)))]).astype(np.int32)
    gh = np.concatenate([gh, near[:, 1], near[:, 1] * (gmax // np.maximum(1, np.abs(near).max(1)))]).astype(np.int32)
    want_t, want_e = host_angles(depth, gv, gh)
    d_gv, d_gh = torch.from_numpy(gv).cuda(), torch.from_numpy(gh).cuda()
    d_t = torch.full((len(gv),), -1, dtype=torch.int32, device="cuda"); d_e = torch.full((len(gv),), -1, dtype=torch.int32, device="cuda")
    assert lib.x265amd_aq_edge_angles_device(None, C.c_void_p(d_gv.data_ptr()), C.c_void_p(d_gh.data_ptr()), len(gv), C.c_void_p(d_t.data_ptr()), C.c_void_p(d_e.data_ptr())) == 0
    torch.cuda.synchronize()
    got_t, got_e = d_t.cpu().numpy(), d_e.cpu().numpy()
    bad = np.flatnonzero((got_t != want_t) | (got_e != want_e))
    assert len(bad) == 0, [(int(gv[i]), int(gh[i]), int(got_t[i]), int(want_t[i])) for i in bad[:10]]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_device_and_host_equal_the_reference_encoders_doubles(depth, gold):
    """x265amd_aq_energy + x265amd_aq_edge + x265amd_aq_offsets_edge on the first pictures of the clip the reference encoded: its qpAqOffset bit for bit, modes 4 and 5"""
    import torch
    L = T.load_hip(depth)
    w, h, n = RC_CLIPS[depth]
    avg = (((w // 2) + 7) >> 3) * (((h // 2) + 7) >> 3)
    frames = rc_frames(depth)
    for poc in range(2):
        flat, stride, cstride, org = padded(frames[poc])
        energy, wp = T.aq_run_hip(L, dict(pic=flat, stride=stride, cstride=cstride, org=org), w, h, 16)
        assert np.array_equal(energy, gold["rc%d/p%d/energy" % (depth, poc)])
        _, _, density, angle, sums = run_edge(depth, frames[poc][0], planes=False)
        assert np.array_equal(density, gold["rc%d/p%d/density" % (depth, poc)]) and np.array_equal(angle, gold["rc%d/p%d/angle" % (depth, poc)])
        assert np.array_equal(sums, gold["rc%d/p%d/sums" % (depth, poc)])
        for mode in (4, 5):
            rc, a, t, f = offsets_edge(depth, energy, density, angle, avg, mode)
            k = "rc%d/m%d/p%d/" % (depth, mode, poc)
            assert rc == 0 and np.array_equal(a.view(np.uint64), gold[k + "qp_aq_offset"].view(np.uint64)) and np.array_equal(f, gold[k + "inv_qscale"]), k
