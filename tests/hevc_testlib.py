"""Shared parity-test machinery (test infrastructure).

One table of *cases* drives every comparison in the suite, in the style of the reference's TestBench
(/root/reference/source/test/testbench.cpp:102-261, pixelharness.cpp:30-81: random / all-min / all-max buffers,
exact equality):

  * oracle  vs reference build (oracle/_ref/librefprims*.so)       -> tests/test_oracle_vs_ref.py   (CPU, here only)
  * oracle  vs golden vectors generated from the reference          -> tests/test_oracle_golden.py   (CPU)
  * HIP C-ABI vs oracle (and vs golden)                             -> tests/test_hip_parity.py      (GPU)

A case is a function `case(L, rng) -> list[np.ndarray]` that performs calls through a `PrimLib` `L`
(`L.call("sad", part, a, sa, b, sb)` resolves to `ref_sad` / `orc_sad` / the HIP per-slot shim
`x265amd_sad`) and returns every output.  The same seeded rng gives the same inputs to every implementation.
"""
import ctypes as C
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
REF_DIR = os.path.join(ORACLE_DIR, "_ref")
PKG_DIR = os.path.join(ROOT, "x265-amod_amd")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")

# enum LumaPU order (reference: source/common/primitives.h:41-55)
PU_SIZES = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (8, 4), (4, 8), (16, 8), (8, 16), (32, 16), (16, 32),
            (64, 32), (32, 64), (16, 12), (12, 16), (16, 4), (4, 16), (32, 24), (24, 32), (32, 8), (8, 32),
            (64, 48), (48, 64), (64, 16), (16, 64)]
CSP_I420 = 1
FENC_STRIDE = 64

_U64_FUNCS = {"sse_pp", "sse_ss", "ssd_s", "var"}


def _ptr(a):
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return a


class PrimLib:
    """ctypes view of one implementation of the primitive set."""

    def __init__(self, path, prefix, depth):
        self.path, self.prefix, self.depth = path, prefix, depth
        self.lib = C.CDLL(path)
        self.pixel = np.uint8 if depth == 8 else np.uint16
        self.pmax = (1 << depth) - 1
        got = getattr(self.lib, prefix + "bit_depth")()
        assert got == depth, (path, got, depth)

    def has(self, name):
        return hasattr(self.lib, self.prefix + name)

    def call(self, name, *args):
        fn = getattr(self.lib, self.prefix + name)
        fn.restype = C.c_uint64 if name in _U64_FUNCS else C.c_int
        conv = []
        for a in args:
            if isinstance(a, np.ndarray):
                conv.append(_ptr(a))
            elif isinstance(a, (int, np.integer)):
                conv.append(C.c_int64(int(a)))
            else:
                conv.append(a)
        return fn(*conv)


# ----------------------------------------------------------------------------------------------------------
# stream argument of the orchestrating entry points: NULL stream, or (X265AMD_TEST_QUEUE=1) a device job queue
# (csrc/xa_queue.h) held for the duration of the call -- the same calls then run as commands to a resident workgroup
# ----------------------------------------------------------------------------------------------------------
class call_stream:
    def __init__(self, L):
        self.lib = L.lib if hasattr(L, "lib") else L
        self.h = None

    def __enter__(self):
        if os.environ.get("X265AMD_TEST_QUEUE"):
            self.lib.x265amd_queue_acquire.restype = C.c_void_p
            self.h = self.lib.x265amd_queue_acquire()
            assert self.h, "no device job queue (X265AMD_QUEUES=0?)"
            return C.c_void_p(self.h)
        return None

    def __exit__(self, *exc):
        if self.h:
            self.lib.x265amd_queue_release(C.c_void_p(self.h))
        return False


class held_queue:
    """a device job queue held for a `with` block, whatever X265AMD_TEST_QUEUE says: yields the handle (the `stream` argument of the entry points), gives the
    queue back on exit.  No queue because the environment carries X265AMD_QUEUES=0: the test is skipped with that reason; no queue otherwise: a failure.

    While a queue is held the resident job server is running, and a device-wide wait behind it hangs ("Round 6, at the very end": a
    hipDeviceSynchronize behind the resident job server).  So:
      * every upload, every torch.zeros and ONE torch.cuda.synchronize() happen BEFORE the block is entered;
      * inside the block there are only calls into the library;
      * x265amd_queue_release fences and drains the queue (xa_queue_release: a releasing fence, then xa_stream_sync), so for the entry points that only enqueue
        (tu_chain, intra_tu_chain, intra_scan, motion_compensation, inter_cost, me_search) the release IS the wait: results are read back only AFTER the block;
      * one queue per case, and no device buffer is used by two cases under one held queue: the server looks at memory afresh only for the commands that ask
        for it (k_job_server: XA_CMD_ACQUIRE and the copy / table-reading commands).
    The runners below take `stream=None` or a held_queue that has NOT been entered yet: they upload, synchronise once, enter it around their library call
    and leave it before they read anything back (stream_scope)."""

    def __init__(self, L):
        self.lib = L.lib if hasattr(L, "lib") else L
        self.h = None

    def __enter__(self):
        self.lib.x265amd_queue_acquire.restype = C.c_void_p
        self.h = self.lib.x265amd_queue_acquire()
        if not self.h:
            if os.environ.get("X265AMD_QUEUES") == "0":
                import pytest
                pytest.skip("X265AMD_QUEUES=0: no device job queues")
            raise AssertionError("x265amd_queue_acquire returned NULL although X265AMD_QUEUES is not 0")
        return C.c_void_p(self.h)

    def __exit__(self, *exc):
        if self.h:
            self.lib.x265amd_queue_release(C.c_void_p(self.h))
            self.h = None
        return False


class stream_scope:
    """the `stream` parameter of a runner: None -> the NULL stream; a held_queue (not entered) -> everything the runner has uploaded so far is waited for, then
    the queue is held for the block.  After the block the results may be read (NULL stream: after a torch.cuda.synchronize(), which this does on exit)."""

    def __init__(self, stream):
        assert stream is None or isinstance(stream, held_queue), "stream: None or a held_queue that has not been entered"
        self.q = stream

    def __enter__(self):
        import torch
        torch.cuda.synchronize()
        return self.q.__enter__() if self.q is not None else None

    def __exit__(self, *exc):
        if self.q is not None:
            self.q.__exit__(*exc)
        if exc[0] is None:
            import torch
            torch.cuda.synchronize()
        return False


# enum XaOp (csrc/xa_queue.h:17-21), in its order: x265amd_queue_stats reports command kind k at out[10 + 3 * k]
XA_OPS = ("NOP", "EXIT", "COPY", "COPY2D", "FILL", "COPY_RECTS", "MC", "MC_COST", "CU_MEASURE", "TU_CHAIN", "TU_CHAIN_RDOQ", "INTRA_TU_CHAIN", "INTRA_TU_CHAIN_RDOQ",
          "INTRA_SCAN", "ME_SEARCH", "ME_SEARCH_STAR", "ME_DEFERRED", "EST_BIT", "INTRA_PU", "INTRA_NXN", "INTER_CHAIN", "INTER_SEARCH", "WAIT")
XA_OP = {name: k for k, name in enumerate(XA_OPS)}
XA_SERVER_WAVES = 8


def queue_stats(L, reset=0, algorithmic_bytes=False):
    """x265amd_queue_stats (valid only while no queue is held): {command kind: commands the job server ran since the last reset}; algorithmic_bytes=True: the bytes
    its jobs had to read and write instead (every job body adds its own figure once, so a job run twice shows there and nowhere else)"""
    out = np.zeros(106, np.uint64)
    lib = L.lib if hasattr(L, "lib") else L
    assert lib.x265amd_queue_stats(_ptr(out), 106, reset) == 0
    return {name: int(out[(12 if algorithmic_bytes else 10) + 3 * k]) for k, name in enumerate(XA_OPS)}


def oracle_path(depth):
    return os.path.join(ORACLE_DIR, "liboracle%d.so" % depth)


def ref_path(depth):
    return os.path.join(REF_DIR, "librefprims%d.so" % depth)


def have_ref():
    return os.path.exists(ref_path(8)) and os.path.exists(ref_path(10))


def load_oracle(depth):
    p = oracle_path(depth)
    if not os.path.exists(p):
        import subprocess
        subprocess.check_call(["make", "-C", ORACLE_DIR, "-s"])
    return PrimLib(p, "orc_", depth)


def load_ref(depth):
    return PrimLib(ref_path(depth), "ref_", depth)


_REF_DRIVER_DIR = None


def load_ref_with(depth, name):
    """load_ref whose driver has the entry ref_<name>.  oracle/_ref/librefprims*.so is OUR file (oracle/refprims.cpp) linked to the reference's objects; a copy of oracle/_ref
    made before the entry was added lacks it, and then the driver alone is built again from the objects and headers oracle/_ref keeps (oracle/build_ref.sh), into a
    directory of this process"""
    global _REF_DRIVER_DIR
    R = load_ref(depth)
    if R.has(name):
        return R
    if _REF_DRIVER_DIR is None:
        import subprocess
        import tempfile
        import atexit
        import shutil
        d = tempfile.mkdtemp(prefix="refprims_")
        atexit.register(shutil.rmtree, d, True)
        subprocess.check_call(["bash", os.path.join(ORACLE_DIR, "build_ref.sh")], env=dict(os.environ, X265_REF_DRIVER_ONLY="1", X265_REF_DRIVER_OUT=d))
        _REF_DRIVER_DIR = d
    R = PrimLib(os.path.join(_REF_DRIVER_DIR, "librefprims%d.so" % depth), "ref_", depth)
    assert R.has(name), "oracle/_ref has no ref_%s and the driver could not be built again on its objects" % name
    return R


def hip_path(depth):
    return os.path.join(PKG_DIR, "lib", "libx265amd_main.so" if depth == 8 else "libx265amd_main10.so")


def load_hip(depth):
    """the product library; never falls back to anything else.  torch (which bundles its own HIP runtime) is imported
    first: the other order leaves torch unable to see the GPU once libx265amd has initialised the system runtime."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    return PrimLib(hip_path(depth), "x265amd_", depth)


# ----------------------------------------------------------------------------------------------------------
# buffers
# ----------------------------------------------------------------------------------------------------------
MODES = ("random", "min", "max")


def pix_buf(L, rng, n, mode):
    if mode == "min":
        return np.zeros(n, L.pixel)
    if mode == "max":
        return np.full(n, L.pmax, L.pixel)
    return rng.integers(0, L.pmax + 1, n, dtype=np.int64).astype(L.pixel)


def s16_buf(rng, n, lo, hi, mode):
    if mode == "min":
        return np.full(n, lo, np.int16)
    if mode == "max":
        return np.full(n, hi, np.int16)
    return rng.integers(lo, hi + 1, n, dtype=np.int64).astype(np.int16)


def off(a, elems):
    """pointer `elems` elements into array a"""
    return C.c_void_p(a.ctypes.data + elems * a.itemsize)


# ----------------------------------------------------------------------------------------------------------
# cases.  Every case takes (L, rng, mode) and returns a list of arrays.
# ----------------------------------------------------------------------------------------------------------
def case_sad(L, rng, mode):
    out = []
    for part, (w, h) in enumerate(PU_SIZES):
        sb = 64 + 2 * int(rng.integers(0, 40))
        a = pix_buf(L, rng, 64 * 64, mode)
        b = pix_buf(L, rng, sb * 80 + 80, "random" if mode == "random" else ("max" if mode == "min" else "min"))
        o = int(rng.integers(0, 16))
        out.append(np.array([L.call("sad", part, a, FENC_STRIDE, off(b, o), sb)], np.int64))
        res = np.zeros(4, np.int32)
        L.call("sad_x3", part, a, off(b, o), off(b, o + 1), off(b, o + sb), sb, res)
        out.append(res[:3].copy())
        res = np.zeros(4, np.int32)
        L.call("sad_x4", part, a, off(b, o), off(b, o + 2), off(b, o + sb), off(b, o + 3 * sb + 1), sb, res)
        out.append(res.copy())
    return out


def case_satd(L, rng, mode):
    out = []
    for part, (w, h) in enumerate(PU_SIZES):
        sa, sb = 64, 64 + 2 * int(rng.integers(0, 40))
        a = pix_buf(L, rng, sa * 64, mode)
        b = pix_buf(L, rng, sb * 64 + 64, "random" if mode == "random" else ("max" if mode == "min" else "min"))
        out.append(np.array([L.call("satd", part, a, sa, b, sb)], np.int64))
        if w >= 8 and h >= 8 and w <= 64 and h <= 64 and (w // 2, h // 2) in PU_SIZES:
            out.append(np.array([L.call("chroma_satd", CSP_I420, part, a, sa, b, sb)], np.int64))
    return out


def case_sa8d(L, rng, mode):
    out = []
    for cu in range(5):
        sa, sb = 64 + 8 * int(rng.integers(0, 4)), 64 + 2 * int(rng.integers(0, 40))
        a = pix_buf(L, rng, sa * 64, mode)
        b = pix_buf(L, rng, sb * 64, "random" if mode == "random" else ("max" if mode == "min" else "min"))
        out.append(np.array([L.call("sa8d", cu, a, sa, b, sb)], np.int64))
        if cu >= 1:
            out.append(np.array([L.call("chroma_sa8d", CSP_I420, cu, a, sa, b, sb)], np.int64))
    return out


def case_sse(L, rng, mode):
    out = []
    lim = L.pmax
    for cu in range(5):
        sa, sb = 64 + 8 * int(rng.integers(0, 4)), 64 + 2 * int(rng.integers(0, 40))
        a = pix_buf(L, rng, sa * 64, mode)
        b = pix_buf(L, rng, sb * 64, "random" if mode == "random" else ("max" if mode == "min" else "min"))
        out.append(np.array([L.call("sse_pp", cu, a, sa, b, sb)], np.uint64))
        sa_ = s16_buf(rng, sa * 64, -lim, lim, mode)
        sb_ = s16_buf(rng, sb * 64, -lim, lim, "random" if mode == "random" else ("max" if mode == "min" else "min"))
        out.append(np.array([L.call("sse_ss", cu, sa_, sa, sb_, sb)], np.uint64))
        out.append(np.array([L.call("ssd_s", cu, sa_, sa)], np.uint64))
    return out


def case_psy(L, rng, mode):
    out = []
    for cu in range(5):
        sa, sb = 64 + 8 * int(rng.integers(0, 4)), 64 + 2 * int(rng.integers(0, 40))
        a = pix_buf(L, rng, sa * 64, mode)
        b = pix_buf(L, rng, sb * 64, "random" if mode == "random" else ("max" if mode == "min" else "min"))
        out.append(np.array([L.call("psy_cost_pp", cu, a, sa, b, sb)], np.int64))
    return out


def case_residual(L, rng, mode):
    out = []
    lim = L.pmax
    for cu in range(5):
        n = 4 << cu
        s0, s1, ds = 64 + 8 * int(rng.integers(0, 3)), 64 + 2 * int(rng.integers(0, 9)), 64
        a = pix_buf(L, rng, s0 * 64, mode)
        b = pix_buf(L, rng, s1 * 64, "random" if mode == "random" else ("max" if mode == "min" else "min"))
        r = np.zeros(ds * 64, np.int16)
        L.call("sub_ps", cu, r, ds, a, b, s0, s1)
        out.append(r.reshape(64, ds)[:n, :n].copy())
        resi = s16_buf(rng, s1 * 64, -lim, lim, mode)
        rec = np.zeros(ds * 64, L.pixel)
        L.call("add_ps", cu, rec, ds, a, resi, s0, s1)
        out.append(rec.reshape(64, ds)[:n, :n].copy())
    return out


def case_avg(L, rng, mode):
    out = []
    for part, (w, h) in enumerate(PU_SIZES):
        s0, s1, ds = 64 + 2 * int(rng.integers(0, 9)), 64 + 2 * int(rng.integers(0, 9)), 64
        a = pix_buf(L, rng, s0 * 64, mode)
        b = pix_buf(L, rng, s1 * 64, mode)
        d = np.zeros(ds * 64, L.pixel)
        L.call("pixelavg_pp", part, d, ds, a, s0, b, s1)
        out.append(d.reshape(64, ds)[:h, :w].copy())
        lo, hi = -8192, 8191
        x = s16_buf(rng, s0 * 64, lo, hi, mode)
        y = s16_buf(rng, s1 * 64, lo, hi, mode)
        d = np.zeros(ds * 64, L.pixel)
        L.call("addAvg", part, x, y, d, s0, s1, ds)
        out.append(d.reshape(64, ds)[:h, :w].copy())
        if w >= 4 and h >= 4:
            d = np.zeros(ds * 64, L.pixel)
            L.call("chroma_addAvg", CSP_I420, part, x, y, d, s0, s1, ds)
            out.append(d.reshape(64, ds)[:h // 2, :w // 2].copy())
    return out


def case_weight(L, rng, mode):
    out = []
    corr = 14 - L.depth
    for _ in range(4):
        w, h, stride = 16 * int(rng.integers(1, 5)), int(rng.integers(1, 17)), 64 + 16 * int(rng.integers(0, 3))
        w0 = int(rng.integers(1, 128))
        shift = int(rng.integers(0, 7)) + corr
        rnd = (1 << (shift - 1)) if shift else 0
        rnd &= ~((1 << corr) - 1)
        offset = int(rng.integers(-20, 21))
        src = pix_buf(L, rng, stride * 16, mode)
        dst = np.zeros(stride * 16, L.pixel)
        L.call("weight_pp", src, dst, stride, w, h, w0, rnd, shift, offset)
        out.append(dst.reshape(16, stride)[:h, :w].copy())
        s = s16_buf(rng, stride * 16, -8192, 8191, mode)
        dst = np.zeros(stride * 16, L.pixel)
        L.call("weight_sp", s, dst, stride, stride, w - 1, h, w0, rnd, shift, offset)
        out.append(dst.reshape(16, stride)[:h, :w - 1].copy())
    return out


def case_misc(L, rng, mode):
    out = []
    stride = 64 + 2 * int(rng.integers(0, 9))
    src = pix_buf(L, rng, stride * 64, mode)
    d = np.zeros(32 * 32, L.pixel)
    L.call("scale2D_64to32", d, src, stride)
    out.append(d.copy())
    s1 = pix_buf(L, rng, 256, mode)
    d = np.zeros(128, L.pixel)
    L.call("scale1D_128to64", d, s1)
    out.append(d.copy())
    for cu in range(5):
        n = 4 << cu
        d = np.zeros(n * n, L.pixel)
        L.call("transpose", cu, d, src, stride)
        out.append(d.copy())
    for cu in range(4):
        n = 4 << cu
        st = n + 8 * int(rng.integers(0, 3))
        s = s16_buf(rng, st * n, -4096, 4095, mode)
        for name, twod in (("cpy2Dto1D_shl", 0), ("cpy2Dto1D_shr", 0), ("cpy1Dto2D_shl", 1), ("cpy1Dto2D_shr", 1)):
            shift = int(rng.integers(1, 3))
            d = np.zeros(st * n, np.int16)
            L.call(name, cu, d, s, st, shift)
            out.append(d.reshape(n, st)[:, :n].copy() if twod else d[:n * n].copy())
        q = s16_buf(rng, n * n, -3, 3, mode)
        out.append(np.array([L.call("count_nonzero", cu, q)], np.int64))
        c = np.zeros(n * n, np.int16)
        out.append(np.array([L.call("copy_cnt", cu, c, s, st)], np.int64))
        out.append(c.copy())
    for cu in range(5):
        out.append(np.array([L.call("var", cu, src, stride)], np.uint64))
    return out


def case_dct(L, rng, mode):
    out = []
    lim = L.pmax
    for cu in range(4):
        n = 4 << cu
        st = n + 8 * int(rng.integers(0, 3))
        src = s16_buf(rng, st * n, -lim, lim, mode)
        d = np.zeros(n * n, np.int16)
        L.call("dct", cu, src, d, st)
        out.append(d.copy())
        # inverse on plausible coefficient data (the forward result) and on full-range data
        r = np.zeros(st * n, np.int16)
        L.call("idct", cu, d, r, st)
        out.append(r.reshape(n, st)[:, :n].copy())
        c = s16_buf(rng, n * n, -32768, 32767, mode)
        r = np.zeros(st * n, np.int16)
        L.call("idct", cu, c, r, st)
        out.append(r.reshape(n, st)[:, :n].copy())
        if cu == 0:
            d2 = np.zeros(16, np.int16)
            L.call("dst4x4", src, d2, st)
            out.append(d2.copy())
            r = np.zeros(st * 4, np.int16)
            L.call("idst4x4", d2, r, st)
            out.append(r.reshape(4, st)[:, :4].copy())
            r = np.zeros(st * 4, np.int16)
            L.call("idst4x4", c, r, st)
            out.append(r.reshape(4, st)[:, :4].copy())
    return out


QUANT_SCALES = [26214, 23302, 20560, 18396, 16384, 14564]   # HEVC quantisation scale per qp%6 (reference: scalinglist.cpp)
INV_QUANT_SCALES = [40, 45, 51, 57, 64, 72]


def case_quant(L, rng, mode):
    out = []
    for cu in range(4):
        n = (4 << cu) ** 2
        log2n = cu + 2
        for _ in range(3):
            qp = int(rng.integers(0, 52))
            per, rem = qp // 6, qp % 6
            tshift = 15 - L.depth - log2n                   # MAX_TR_DYNAMIC_RANGE - depth - log2TrSize
            qbits = 14 + per + tshift
            add = (171 if rng.integers(0, 2) else 85) << (qbits - 9)
            coef = s16_buf(rng, n, -32768, 32767, mode)
            qc = np.full(n, QUANT_SCALES[rem], np.int32)
            if mode == "random":
                qc = (qc.astype(np.int64) * 16 // rng.integers(8, 40, n)).astype(np.int32)   # scaling-list style tables
            du = np.zeros(n, np.int32)
            q = np.zeros(n, np.int16)
            ns = L.call("quant", coef, qc, du, q, qbits, add, n)
            out += [np.array([ns], np.int64), du.copy(), q.copy()]
            q2 = np.zeros(n, np.int16)
            ns = L.call("nquant", coef, qc, q2, qbits, add, n)
            out += [np.array([ns], np.int64), q2.copy()]
            # dequant (quant.cpp:559-569): shift = QUANT_IQUANT_SHIFT(20) - QUANT_SHIFT(14) - transformShift
            shift = 20 - 14 - tshift
            d = np.zeros(n, np.int16)
            L.call("dequant_normal", q, d, n, INV_QUANT_SCALES[rem] << per, shift)
            out.append(d.copy())
            dq = (np.full(n, INV_QUANT_SCALES[rem] * 16, np.int64) if mode != "random"
                  else INV_QUANT_SCALES[rem] * rng.integers(8, 40, n)).astype(np.int32)
            d = np.zeros(n, np.int16)
            L.call("dequant_scaling", q, dq, d, n, per, shift)
            out.append(d.copy())
    return out


def case_intra(L, rng, mode):
    out = []
    for cu in range(4):
        n = 4 << cu
        nb = pix_buf(L, rng, 4 * n + 1 + 16, mode)
        if mode == "random" and rng.integers(0, 2):     # smooth neighbours exercise the rounding paths differently
            nb = np.clip(np.cumsum(rng.integers(-3, 4, nb.size)) + L.pmax // 2, 0, L.pmax).astype(L.pixel)
        filt = np.zeros_like(nb)
        L.call("intra_filter", cu, nb, filt)
        out.append(filt[:4 * n + 1].copy())
        ds = n + 8 * int(rng.integers(0, 3))
        for m in range(35):
            for bf in (0, 1):
                d = np.zeros(ds * n, L.pixel)
                L.call("intra_pred", cu, m, d, ds, nb, bf)
                out.append(d.reshape(n, ds)[:, :n].copy())
        for bl in (0, 1):
            d = np.zeros(33 * n * n, L.pixel)
            L.call("intra_allangs", cu, d, nb, filt, bl)
            out.append(d.copy())
    return out


def case_ipfilter_luma(L, rng, mode):
    out = []
    for part, (w, h) in enumerate(PU_SIZES):
        ss = 80 + 2 * int(rng.integers(0, 9))
        src = pix_buf(L, rng, ss * 80, mode)
        sp = off(src, 4 * ss + 4)
        s16 = s16_buf(rng, ss * 80, -8192, 8191 if L.depth == 8 else 8191, mode)
        s16p = off(s16, 4 * ss + 4)
        ds = 64 + 2 * int(rng.integers(0, 5))
        idx = int(rng.integers(0, 4))
        for name in ("luma_hpp", "luma_vpp"):
            d = np.zeros(ds * 72, L.pixel)
            L.call(name, part, sp, ss, d, ds, idx)
            out.append(d.reshape(72, ds)[:h, :w].copy())
        for ext in (0, 1):
            d = np.zeros(ds * 72, np.int16)
            L.call("luma_hps", part, sp, ss, d, ds, idx, ext)
            out.append(d.reshape(72, ds)[:h + 7 * ext, :w].copy())
        d = np.zeros(ds * 72, np.int16)
        L.call("luma_vps", part, sp, ss, d, ds, idx)
        out.append(d.reshape(72, ds)[:h, :w].copy())
        d = np.zeros(ds * 72, L.pixel)
        L.call("luma_vsp", part, s16p, ss, d, ds, idx)
        out.append(d.reshape(72, ds)[:h, :w].copy())
        d = np.zeros(ds * 72, np.int16)
        L.call("luma_vss", part, s16p, ss, d, ds, idx)
        out.append(d.reshape(72, ds)[:h, :w].copy())
        d = np.zeros(ds * 72, L.pixel)
        L.call("luma_hvpp", part, sp, ss, d, ds, int(rng.integers(1, 4)), int(rng.integers(1, 4)))
        out.append(d.reshape(72, ds)[:h, :w].copy())
        d = np.zeros(ds * 72, np.int16)
        L.call("luma_p2s", part, sp, ss, d, ds)
        out.append(d.reshape(72, ds)[:h, :w].copy())
    return out


def case_ipfilter_chroma(L, rng, mode):
    out = []
    for part, (w, h) in enumerate(PU_SIZES):
        if (w, h) == (4, 4):      # no 2x2 chroma filter entries (reference: ipfilter.cpp:418-466)
            continue
        cw, ch = w // 2, h // 2
        ss = 48 + 2 * int(rng.integers(0, 9))
        src = pix_buf(L, rng, ss * 48, mode)
        sp = off(src, 4 * ss + 4)
        s16 = s16_buf(rng, ss * 48, -8192, 8191, mode)
        s16p = off(s16, 4 * ss + 4)
        ds = 32 + 2 * int(rng.integers(0, 5))
        idx = int(rng.integers(0, 8))
        for name in ("chroma_hpp", "chroma_vpp"):
            d = np.zeros(ds * 40, L.pixel)
            L.call(name, CSP_I420, part, sp, ss, d, ds, idx)
            out.append(d.reshape(40, ds)[:ch, :cw].copy())
        for ext in (0, 1):
            d = np.zeros(ds * 40, np.int16)
            L.call("chroma_hps", CSP_I420, part, sp, ss, d, ds, idx, ext)
            out.append(d.reshape(40, ds)[:ch + 3 * ext, :cw].copy())
        d = np.zeros(ds * 40, np.int16)
        L.call("chroma_vps", CSP_I420, part, sp, ss, d, ds, idx)
        out.append(d.reshape(40, ds)[:ch, :cw].copy())
        d = np.zeros(ds * 40, L.pixel)
        L.call("chroma_vsp", CSP_I420, part, s16p, ss, d, ds, idx)
        out.append(d.reshape(40, ds)[:ch, :cw].copy())
        d = np.zeros(ds * 40, np.int16)
        L.call("chroma_vss", CSP_I420, part, s16p, ss, d, ds, idx)
        out.append(d.reshape(40, ds)[:ch, :cw].copy())
        d = np.zeros(ds * 40, np.int16)
        L.call("chroma_p2s", CSP_I420, part, sp, ss, d, ds)
        out.append(d.reshape(40, ds)[:ch, :cw].copy())
    return out


CASES = {
    "sad": case_sad,
    "satd": case_satd,
    "sa8d": case_sa8d,
    "sse": case_sse,
    "psy": case_psy,
    "residual": case_residual,
    "avg": case_avg,
    "weight": case_weight,
    "misc": case_misc,
    "dct": case_dct,
    "quant": case_quant,
    "intra": case_intra,
    "ipfilter_luma": case_ipfilter_luma,
    "ipfilter_chroma": case_ipfilter_chroma,
}


def case_seed(name, depth, mode, rep):
    h = hashlib.sha256(("%s/%d/%s/%d" % (name, depth, mode, rep)).encode()).digest()
    return int.from_bytes(h[:8], "little")


def run_case(L, name, mode, rep=0):
    rng = np.random.default_rng(case_seed(name, L.depth, mode, rep))
    return CASES[name](L, rng, mode)


def digest(arrs):
    h = hashlib.sha256()
    for a in arrs:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def assert_same(got, want, what):
    assert len(got) == len(want), "%s: %d vs %d outputs" % (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, "%s[%d]: shape/dtype %s %s vs %s %s" % (what, i, g.shape, g.dtype, w.shape, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s: output %d differs at %d positions, first %s: got %s want %s"
                                 % (what, i, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])]))


# ----------------------------------------------------------------------------------------------------------
# motion-estimation cases: the arguments of MotionEstimate::motionEstimate()
# ----------------------------------------------------------------------------------------------------------
ME_DIA, ME_HEX, ME_UMH, ME_STAR = 0, 1, 2, 3
ME_MARGIN = 96      # padded planes, like PicYuv (reference: common/picyuv.cpp: marginX = maxCU + 32)


def me_make_planes(depth, seed, width=256, height=192, motion=(5, -3), noise=3, margin=None):
    """Deterministic integer-only synthetic pair: a textured reference plane (with margins) and a current plane that
    is the reference displaced by `motion` full-pel samples plus small noise.  Returns (cur, ref, stride, origin)
    where origin is the element offset of sample (0,0)."""
    rng = np.random.default_rng(seed)
    pmax = (1 << depth) - 1
    margin = ME_MARGIN if margin is None else margin
    stride = width + 2 * margin
    rows = height + 2 * margin
    base = rng.integers(0, pmax + 1, (rows // 8 + 2, stride // 8 + 2)).astype(np.int64)
    up = np.kron(base, np.ones((8, 8), np.int64))[:rows, :stride]
    # cheap integer smoothing so that sub-pel interpolation and the search have structure to follow
    sm = (up + np.roll(up, 1, 0) + np.roll(up, 1, 1) + np.roll(up, (1, 1), (0, 1)) + 2) >> 2
    sm = (sm * 3 + np.roll(sm, 3, 1) + 2) >> 2
    ref = np.clip(sm + rng.integers(-noise, noise + 1, sm.shape), 0, pmax)
    def shifted(mx, my):
        return np.roll(ref, (-my, -mx), (0, 1))
    # four quadrants move differently (one of them by a half-sample) so that results differ from job to job
    cur = shifted(*motion).copy()
    hy, hx = rows // 2, stride // 2
    cur[:hy, hx:] = shifted(motion[0] + 2, motion[1] - 1)[:hy, hx:]
    cur[hy:, :hx] = ((shifted(motion[0], motion[1]) + shifted(motion[0] + 1, motion[1]) + 1) >> 1)[hy:, :hx]
    cur[hy:, hx:] = shifted(-motion[0], motion[1] + 4)[hy:, hx:]
    cur = np.clip(cur + rng.integers(-noise, noise + 1, cur.shape), 0, pmax)
    dt = np.uint8 if depth == 8 else np.uint16
    return np.ascontiguousarray(cur.astype(dt)).ravel(), np.ascontiguousarray(ref.astype(dt)).ravel(), stride, margin * stride + margin


def me_jobs(seed, n, width=256, height=192, motion=(5, -3), methods=(ME_HEX,), submes=(2,), merange=57):
    """n random search jobs: dict of arrays, one row per job"""
    rng = np.random.default_rng(seed ^ 0x5EED)
    sizes = [(64, 64), (32, 32), (16, 16), (8, 8), (32, 16), (16, 32), (16, 8), (8, 16), (64, 32), (32, 64), (8, 4), (4, 8),
             (16, 12), (12, 16), (16, 4), (4, 16), (32, 24), (24, 32), (32, 8), (8, 32), (64, 48), (48, 64), (64, 16), (16, 64)]
    jobs = []
    for i in range(n):
        w, h = sizes[int(rng.integers(0, 4 if i % 3 else len(sizes)))]
        # a PU never straddles a CTU: pick a 64x64 tile, then an offset (multiple of 4) that keeps the PU inside it
        x = int(rng.integers(0, width // 64)) * 64 + int(rng.integers(0, (64 - w) // 4 + 1)) * 4
        y = int(rng.integers(0, height // 64)) * 64 + int(rng.integers(0, (64 - h) // 4 + 1)) * 4
        qp = int(rng.integers(12, 46))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            mvp = (0, 0)
        elif kind == 1:
            mvp = (motion[0] * 4 + int(rng.integers(-6, 7)), motion[1] * 4 + int(rng.integers(-6, 7)))
        else:
            mvp = (int(rng.integers(-80, 81)), int(rng.integers(-80, 81)))
        # setSearchRange (reference: search.cpp:2724-2768): window = mvp +- merange, clipped so the block stays
        # inside the padded picture; values in full-pel
        mr = merange if rng.integers(0, 3) else int(rng.integers(4, 32))
        lim = 64 + 8     # how far outside the picture a block may reach (inside the 96-sample margin with taps)
        mnx = max((mvp[0] >> 2) - mr, -x - lim + 8); mxx = min((mvp[0] >> 2) + mr, width - x - w + lim - 8)
        mny = max((mvp[1] >> 2) - mr, -y - lim + 8); mxy = min((mvp[1] >> 2) + mr, height - y - h + lim - 8)
        ncand = int(rng.integers(0, 5))
        mvc = [(int(rng.integers(-60, 61)), int(rng.integers(-60, 61))) for _ in range(ncand)]
        if ncand and rng.integers(0, 2):
            mvc[0] = (motion[0] * 4, motion[1] * 4)
        jobs.append(dict(x=x, y=y, w=w, h=h, qp=qp, mvp=mvp, mvmin=(mnx, mny), mvmax=(mxx, mxy), mvc=mvc, merange=mr,
                         method=int(methods[i % len(methods)]), subme=int(submes[(i // len(methods)) % len(submes)])))
    return jobs


def me_run_host(L, cur, ref, stride, origin, jobs):
    """runs jobs one by one through `<prefix>motion_estimate` (reference driver or oracle); returns int array [n,3]"""
    out = np.zeros((len(jobs), 3), np.int32)
    fn = getattr(L.lib, L.prefix + "motion_estimate")
    fn.restype = C.c_int
    for i, j in enumerate(jobs):
        mv = np.zeros(2, np.int32)
        mvc = np.array(j["mvc"], np.int32).reshape(-1) if j["mvc"] else np.zeros(2, np.int32)
        cost = fn(off(cur, origin), off(ref, origin), C.c_int64(stride), j["x"], j["y"], j["w"], j["h"], j["method"], j["subme"], j["qp"],
                  _ptr(np.array(j["mvmin"], np.int32)), _ptr(np.array(j["mvmax"], np.int32)), _ptr(np.array(j["mvp"], np.int32)),
                  len(j["mvc"]), _ptr(mvc), j["merange"], _ptr(mv))
        out[i] = (mv[0], mv[1], cost)
    return out


def me_run_host_batch(L, cur, ref, stride, origin, packed):
    """all jobs of a packed array (ME_JOB_DT) in ONE C call; returns int32 [n,3]"""
    out = np.zeros((len(packed), 3), np.int32)
    fn = getattr(L.lib, L.prefix + "motion_estimate_batch")
    fn.restype = C.c_int
    fn(off(cur, origin), off(ref, origin), C.c_int64(stride), _ptr(np.ascontiguousarray(packed)), len(packed), _ptr(out))
    return out


ME_JOB_DT = np.dtype([("x", "<i2"), ("y", "<i2"), ("w", "u1"), ("h", "u1"), ("method", "u1"), ("subme", "u1"), ("qp", "u1"),
                      ("num_cand", "u1"), ("merange", "<i2"), ("mvmin", "<i2", 2), ("mvmax", "<i2", 2), ("mvp", "<i2", 2),
                      ("mvc", "<i2", (12, 2))])
ME_GROUP_DT = np.dtype([("first_job", "<i4"), ("num_jobs", "<i4"), ("ref", "<i4"), ("win_x", "<i2"), ("win_y", "<i2"),
                        ("win_w", "<i2"), ("win_h", "<i2"), ("fenc_x", "<i2"), ("fenc_y", "<i2")])
ME_RESULT_DT = np.dtype([("mv", "<i2", 2), ("cost", "<i4")])
assert ME_JOB_DT.itemsize == 72 and ME_GROUP_DT.itemsize == 24 and ME_RESULT_DT.itemsize == 8


def me_pack_jobs(jobs):
    a = np.zeros(len(jobs), ME_JOB_DT)
    for i, j in enumerate(jobs):
        a[i]["x"], a[i]["y"], a[i]["w"], a[i]["h"] = j["x"], j["y"], j["w"], j["h"]
        a[i]["method"], a[i]["subme"], a[i]["qp"], a[i]["num_cand"], a[i]["merange"] = j["method"], j["subme"], j["qp"], len(j["mvc"]), j["merange"]
        a[i]["mvmin"], a[i]["mvmax"], a[i]["mvp"] = j["mvmin"], j["mvmax"], j["mvp"]
        for k, c in enumerate(j["mvc"]):
            a[i]["mvc"][k] = c
    return a


class HipME:
    """drives x265amd_me_* (include/x265amd.h layer 3) with torch tensors as device memory"""

    def __init__(self, depth):
        import torch
        self.torch = torch
        self.L = load_hip(depth)
        self.lib = self.L.lib
        self.lib.x265amd_me_open.restype = C.c_void_p
        self.ctx = C.c_void_p(self.lib.x265amd_me_open())
        assert self.ctx.value, self.lib.x265amd_last_error()

    def close(self):
        self.lib.x265amd_me_close(self.ctx)

    def host_mvcost(self, qp):
        self.lib.x265amd_me_host_mvcost.restype = C.POINTER(C.c_uint16)
        return np.ctypeslib.as_array(self.lib.x265amd_me_host_mvcost(self.ctx, qp), (2 * 65536 + 1,))

    def plan(self, packed, ref=0, max_win=(192, 192)):
        n = len(packed)
        groups = np.zeros(max(n, 1), ME_GROUP_DT)
        order = np.zeros(max(n, 1), np.int32)
        ng = self.lib.x265amd_me_plan(_ptr(packed), n, ref, max_win[0], max_win[1], _ptr(groups), _ptr(order))
        assert ng >= 0, self.lib.x265amd_last_error()
        return groups[:ng].copy(), order[:n].copy()

    def upload(self, arr):
        t = self.torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()
        return t

    def search(self, d_cur, d_refs, stride, origin_elems, itemsize, groups, packed_ordered, max_win=(192, 192), stream=None, flags=None,
               d_chroma=None, cstride=0):
        """d_cur / d_refs: uploaded planes (uint8 tensors); returns result tensor (device, bytes)"""
        torch = self.torch
        d_groups = self.upload(groups)
        d_jobs = self.upload(packed_ordered)
        d_out = torch.zeros(len(packed_ordered) * 8, dtype=torch.uint8, device="cuda")
        refs = np.array([r.data_ptr() + origin_elems * itemsize for r in d_refs], np.uint64)
        d_reftab = self.upload(refs)
        if flags is None:
            flags = (1 if ((packed_ordered["method"] & 0x7f) == ME_STAR).any() else 0) | (2 if (packed_ordered["method"] & 0x80).any() else 0)
        def call(st):
            return self.lib.x265amd_me_search(self.ctx, st, C.c_void_p(d_cur.data_ptr() + origin_elems * itemsize),
                                              C.c_void_p(d_reftab.data_ptr()), C.c_int64(stride), C.c_void_p(d_groups.data_ptr()), len(groups),
                                              C.c_void_p(d_jobs.data_ptr()), C.c_void_p(d_out.data_ptr()), max_win[0], max_win[1], flags,
                                              C.c_void_p(d_chroma.data_ptr() if d_chroma is not None else 0), C.c_int64(cstride))
        if isinstance(stream, held_queue):      # not entered yet: held around the call alone, after the uploads above (see held_queue)
            with stream_scope(stream) as st:
                rc = call(st)
        else:
            rc = call(C.c_void_p(stream or 0))
        assert rc == 0, self.lib.x265amd_last_error()
        self._keep = (d_groups, d_jobs, d_reftab)
        return d_out

    def run_c(self, cur, ref, stride, cstride, origin, corg, jobs, max_win=(192, 192)):
        """encoder form with chroma SATD: cur / ref are [Y, U, V] host planes"""
        packed = me_pack_jobs(jobs)
        packed["method"] |= 0x80
        groups, order = self.plan(packed, 0, max_win)
        d = [self.upload(p) for p in cur + ref]
        isz = cur[0].itemsize
        chroma = self.upload(np.array([d[1].data_ptr() + corg * isz, d[2].data_ptr() + corg * isz, d[4].data_ptr() + corg * isz, d[5].data_ptr() + corg * isz], np.uint64))
        d_out = self.search(d[0], [d[3]], stride, origin, isz, groups, packed[order], max_win, d_chroma=chroma, cstride=cstride)
        self.torch.cuda.synchronize()
        res = d_out.cpu().numpy().view(ME_RESULT_DT)
        out = np.zeros((len(jobs), 3), np.int32)
        out[order, 0] = res["mv"][:, 0]; out[order, 1] = res["mv"][:, 1]; out[order, 2] = res["cost"]
        return out

    def run(self, cur, ref, stride, origin, jobs, max_win=(192, 192), flags=None):
        """host arrays in, int array [n,3] (mvx, mvy, cost) out, in the order of `jobs`"""
        packed = me_pack_jobs(jobs)
        groups, order = self.plan(packed, 0, max_win)
        d_cur, d_ref = self.upload(cur), self.upload(ref)
        d_out = self.search(d_cur, [d_ref], stride, origin, cur.itemsize, groups, packed[order], max_win, flags=flags)
        self.torch.cuda.synchronize()
        res = d_out.cpu().numpy().view(ME_RESULT_DT)
        out = np.zeros((len(jobs), 3), np.int32)
        out[order, 0] = res["mv"][:, 0]
        out[order, 1] = res["mv"][:, 1]
        out[order, 2] = res["cost"]
        return out


# ----------------------------------------------------------------------------------------------------------
# residual (transform unit) cases: Quant::transformNxN / invtransformNxN / the per-TU measurement
# ----------------------------------------------------------------------------------------------------------
def tu_cases(depth, seed, n):
    """n random TUs: dict(fenc, pred (N x N arrays), log2, ttype, intra, dir, slice, qpScaled, signhide)"""
    rng = np.random.default_rng(seed)
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    cases = []
    for i in range(n):
        log2 = int(rng.integers(2, 6))
        N = 1 << log2
        ttype = int(rng.integers(0, 3))
        intra = int(rng.integers(0, 2))
        base = rng.integers(0, pmax + 1, (N // 4 + 1, N // 4 + 1)).astype(np.int64)
        tex = np.kron(base, np.ones((4, 4), np.int64))[:N, :N]
        amp = int(rng.choice([1, 3, 8, 24, 80])) << (depth - 8)
        fenc = np.clip(tex + rng.integers(-amp, amp + 1, (N, N)), 0, pmax)
        kind = int(rng.integers(0, 4))
        if kind == 0:
            pred = np.clip(fenc + rng.integers(-2, 3, (N, N)), 0, pmax)           # tiny residual -> mostly zero levels
        elif kind == 1:
            pred = np.clip(tex + rng.integers(-amp, amp + 1, (N, N)), 0, pmax)
        elif kind == 2:
            pred = np.full((N, N), int(fenc.mean()))                                # DC-ish prediction
        else:
            pred = np.clip(fenc + int(rng.integers(-3, 4)), 0, pmax)                # DC-only residual
        qp = int(rng.integers(4, 52))
        cases.append(dict(fenc=np.ascontiguousarray(fenc.astype(dt)), pred=np.ascontiguousarray(pred.astype(dt)), log2=log2, ttype=ttype,
                          intra=intra, dir=int(rng.integers(0, 35)), slice=int(rng.integers(0, 3)), qp=qp + 6 * (depth - 8),
                          signhide=int(rng.integers(0, 4) != 0)))
    return cases


def tu_run_host(L, cases):
    """through <prefix>transform_tu / invtransform_tu; returns list of (numSig, coeff, resi)"""
    out = []
    ft = getattr(L.lib, L.prefix + "transform_tu"); ft.restype = C.c_uint32
    fi = getattr(L.lib, L.prefix + "invtransform_tu")
    for c in cases:
        N = 1 << c["log2"]
        resi = (c["fenc"].astype(np.int32) - c["pred"].astype(np.int32)).astype(np.int16)
        coeff = np.zeros(N * N, np.int16)
        ns = ft(_ptr(c["fenc"]), C.c_int64(N), _ptr(resi), C.c_int64(N), _ptr(coeff), c["log2"], c["ttype"], c["intra"], c["dir"], c["slice"], c["qp"], c["signhide"])
        r2 = np.zeros((N, N), np.int16)
        if ns:
            fi(_ptr(r2), C.c_int64(N), _ptr(coeff), c["log2"], c["ttype"], c["intra"], c["qp"], C.c_uint32(ns))
        out.append((int(ns), coeff.copy(), r2.copy()))
    return out


def tu_run_chain_oracle(L, cases):
    """orc_tu_chain: returns list of (stats[5], coeff, resi, recon)"""
    out = []
    for c in cases:
        N = 1 << c["log2"]
        coeff = np.zeros(N * N, np.int16); resi = np.zeros((N, N), np.int16); recon = np.zeros((N, N), c["fenc"].dtype)
        st = np.zeros(5, np.uint64)
        L.lib.orc_tu_chain(_ptr(c["fenc"]), C.c_int64(N), _ptr(c["pred"]), C.c_int64(N), c["log2"], c["ttype"], c["intra"], c["dir"], c["slice"],
                           c["qp"], c["signhide"], _ptr(coeff), _ptr(resi), C.c_int64(N), _ptr(recon), C.c_int64(N), _ptr(st))
        out.append((st.copy(), coeff, resi, recon))
    return out


TU_JOB_DT = np.dtype([("fenc", "<u8"), ("pred", "<u8"), ("coeff", "<u8"), ("resi", "<u8"), ("recon", "<u8"),
                      ("fenc_stride", "<i4"), ("pred_stride", "<i4"), ("resi_stride", "<i4"), ("recon_stride", "<i4"),
                      ("log2", "u1"), ("ttype", "u1"), ("intra", "u1"), ("dir", "u1"), ("slice", "u1"), ("qp", "u1"), ("signhide", "u1"), ("reserved", "u1")])
TU_RESULT_DT = np.dtype([("num_sig", "<u4"), ("zero_energy", "<u4"), ("nz_energy", "<u4"), ("reserved", "<u4"), ("zero_dist", "<u8"), ("nz_dist", "<u8")])
assert TU_JOB_DT.itemsize == 64 and TU_RESULT_DT.itemsize == 32


def tu_chain_run_hip(L, cases, depth, stream=None):
    """x265amd_tu_chain on a batch in one arena (per case fenc | pred | recon | coeff | resi at stride 32); same return shape as tu_run_chain_oracle:
    list of (stats[5], coeff, resi, recon)"""
    import torch
    dt = np.uint8 if depth == 8 else np.uint16
    isz = np.dtype(dt).itemsize
    per = 32 * 32 * (isz * 3 + 2 * 2)
    arena = np.zeros(len(cases) * per, np.uint8)
    jobs = np.zeros(len(cases), TU_JOB_DT)
    for i, c in enumerate(cases):
        N = 1 << c["log2"]
        base = i * per
        f = arena[base:base + 1024 * isz].view(dt).reshape(32, 32); f[:N, :N] = c["fenc"]
        p = arena[base + 1024 * isz:base + 2048 * isz].view(dt).reshape(32, 32); p[:N, :N] = c["pred"]
        jobs[i] = (0, 0, 0, 0, 0, 32, 32, 32, 32, c["log2"], c["ttype"], c["intra"], c["dir"], c["slice"], c["qp"], c["signhide"], 0)
    d_arena = torch.from_numpy(arena).cuda()
    a0 = d_arena.data_ptr()
    for i in range(len(cases)):
        base = a0 + i * per
        jobs[i]["fenc"] = base; jobs[i]["pred"] = base + 1024 * isz
        jobs[i]["recon"] = base + 2048 * isz; jobs[i]["coeff"] = base + 3072 * isz; jobs[i]["resi"] = base + 3072 * isz + 2048
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(len(cases) * TU_RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    with stream_scope(stream) as st:
        rc = L.lib.x265amd_tu_chain(st, C.c_void_p(d_jobs.data_ptr()), len(cases), C.c_void_p(d_out.data_ptr()))
    assert rc == 0
    return tu_chain_unpack(cases, d_out.cpu().numpy().view(TU_RESULT_DT), d_arena.cpu().numpy(), per, dt)


def tu_chain_unpack(cases, res, back, per, dt):
    isz = np.dtype(dt).itemsize
    out = []
    for i, c in enumerate(cases):
        N = 1 << c["log2"]
        base = i * per
        st = np.array([res[i]["num_sig"], res[i]["zero_dist"], res[i]["zero_energy"], res[i]["nz_dist"], res[i]["nz_energy"]], np.uint64)
        out.append((st, back[base + 3072 * isz:base + 3072 * isz + N * N * 2].view(np.int16).copy(),
                    back[base + 3072 * isz + 2048:base + 3072 * isz + 4096].view(np.int16).reshape(32, 32)[:N, :N].copy(),
                    back[base + 2048 * isz:base + 3072 * isz].view(dt).reshape(32, 32)[:N, :N].copy()))
    return out


def tu_chain_assert(got, want, cases, what):
    """(stats, coeff, resi, recon) per unit, product against oracle; the message names the operation, the unit and its size"""
    assert len(got) == len(want) == len(cases)
    for i, (c, g, w) in enumerate(zip(cases, got, want)):
        tag = "%s: unit %d of %d (%dx%d)" % (what, i, len(cases), 1 << c["log2"], 1 << c["log2"])
        assert tuple(int(v) for v in g[0]) == tuple(int(v) for v in w[0]), "%s: (numSig, dist0, energy0, dist, energy) %s, want %s" % (tag, g[0], w[0])
        assert np.array_equal(g[3], w[3]), tag + ": reconstruction"
        assert np.array_equal(g[1], w[1]), tag + ": levels"
        assert np.array_equal(g[2], w[2]), tag + ": residual"


# ----------------------------------------------------------------------------------------------------------
# intra cases: neighbour set (initAdiPattern) + 35-mode sa8d scan
# ----------------------------------------------------------------------------------------------------------
def intra_cases(depth, seed, n):
    """n random intra blocks inside a small reconstructed plane; dict(plane, stride, off (block top-left), log2, flags, strong, fenc)"""
    rng = np.random.default_rng(seed)
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    cases = []
    for i in range(n):
        log2 = int(rng.integers(2, 6))
        N = 1 << log2
        stride = 3 * N + 16
        kind = int(rng.integers(0, 3))
        if kind == 0:
            plane = rng.integers(0, pmax + 1, (3 * N + 8, stride))
        elif kind == 1:     # smooth plane: triggers the strong (bilinear) smoothing at 32x32
            yy, xx = np.mgrid[0:3 * N + 8, 0:stride]
            plane = np.clip((pmax // 3) + (xx * int(rng.integers(0, 3)) + yy * int(rng.integers(0, 3))) // 4 + rng.integers(0, 2, xx.shape), 0, pmax)
        else:
            base = rng.integers(0, pmax + 1, ((3 * N + 8) // 8 + 1, stride // 8 + 1))
            plane = np.kron(base, np.ones((8, 8), np.int64))[:3 * N + 8, :stride]
        plane = np.ascontiguousarray(plane.astype(dt))
        units = N // 4
        total = 4 * units + 1
        mode = int(rng.integers(0, 5))
        if mode == 0:
            flags = np.ones(total, np.uint8)
        elif mode == 1:
            flags = np.zeros(total, np.uint8)
        elif mode == 2:     # typical: left + above available, below-left / above-right not
            flags = np.ones(total, np.uint8); flags[:units] = 0; flags[3 * units + 1:] = 0
        elif mode == 3:     # picture top edge
            flags = np.zeros(total, np.uint8); flags[units:2 * units] = 1
        else:
            flags = rng.integers(0, 2, total).astype(np.uint8)
        fenc = np.ascontiguousarray(np.clip(plane[N + 4:2 * N + 4, N + 4:2 * N + 4].astype(np.int64) + rng.integers(-6, 7, (N, N)), 0, pmax).astype(dt))
        cases.append(dict(plane=plane.ravel(), stride=stride, off=(N + 4) * stride + N + 4, log2=log2, flags=flags,
                          strong=int(rng.integers(0, 2)), fenc=fenc))
    return cases


def intra_run_host(L, cases):
    """returns list of (ref[4N+1], flt[4N+1] or None, sa8d[35])"""
    out = []
    fa = getattr(L.lib, L.prefix + "init_adi_pattern")
    fs = getattr(L.lib, L.prefix + "intra_scan")
    for c in cases:
        N = 1 << c["log2"]
        ref = np.zeros(258, c["plane"].dtype); flt = np.zeros(258, c["plane"].dtype)
        fa(off(c["plane"], c["off"]), C.c_int64(c["stride"]), c["log2"], _ptr(c["flags"]), c["strong"], -1, _ptr(ref), _ptr(flt))
        filtered = N >= 8
        if not filtered:
            flt[:] = 0
        sa = np.zeros(35, np.int32)
        fs(_ptr(c["fenc"]), C.c_int64(N), c["log2"], _ptr(ref), _ptr(flt if filtered else ref), _ptr(sa))
        out.append((ref[:4 * N + 1].copy(), flt[:4 * N + 1].copy() if filtered else None, sa))
    return out


INTRA_JOB_DT = np.dtype([("recon", "<u8"), ("fenc", "<u8"), ("avail", "<u8"), ("recon_stride", "<i4"), ("fenc_stride", "<i4"),
                         ("log2", "u1"), ("strong", "u1"), ("reserved", "u1", 6)])
assert INTRA_JOB_DT.itemsize == 40


def intra_run_hip(L, cases, stream=None):
    """x265amd_intra_scan on a batch; same return shape as intra_run_host"""
    import torch
    isz = cases[0]["plane"].itemsize
    planes = np.concatenate([c["plane"].view(np.uint8) for c in cases])
    fencs = np.concatenate([c["fenc"].ravel().view(np.uint8) for c in cases])
    d_planes, d_fencs = torch.from_numpy(planes).cuda(), torch.from_numpy(fencs).cuda()
    jobs = np.zeros(len(cases), INTRA_JOB_DT)
    po = fo = 0
    for i, c in enumerate(cases):
        N = 1 << c["log2"]
        mask = 0
        for u, f in enumerate(c["flags"]):
            mask |= int(f) << u
        jobs[i] = (d_planes.data_ptr() + po + c["off"] * isz, d_fencs.data_ptr() + fo, mask, c["stride"], N, c["log2"], c["strong"], 0)
        po += c["plane"].nbytes; fo += c["fenc"].nbytes
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_sa = torch.zeros(len(cases) * 35, dtype=torch.int32, device="cuda")
    d_nb = torch.zeros(len(cases) * 2 * 129 * isz, dtype=torch.uint8, device="cuda")
    with stream_scope(stream) as st:
        rc = L.lib.x265amd_intra_scan(st, C.c_void_p(d_jobs.data_ptr()), len(cases), C.c_void_p(d_sa.data_ptr()), C.c_void_p(d_nb.data_ptr()))
    assert rc == 0
    sa = d_sa.cpu().numpy().reshape(-1, 35)
    nb = d_nb.cpu().numpy().view(cases[0]["plane"].dtype).reshape(-1, 2, 129)
    out = []
    for i, c in enumerate(cases):
        N = 1 << c["log2"]
        out.append((nb[i, 0, :4 * N + 1].copy(), nb[i, 1, :4 * N + 1].copy() if N >= 8 else None, sa[i].copy()))
    return out


# ----------------------------------------------------------------------------------------------------------
# inter prediction cases: Predict::motionCompensation
# ----------------------------------------------------------------------------------------------------------
MC_WP_DT = np.dtype([("w", "<i2"), ("o", "<i2"), ("denom", "u1"), ("present", "u1")])
MC_JOB_DT = np.dtype([("dstY", "<u8"), ("dstU", "<u8"), ("dstV", "<u8"), ("dstStride", "<i4"), ("dstCStride", "<i4"),
                      ("x", "<i2"), ("y", "<i2"), ("cuX", "<i2"), ("cuY", "<i2"), ("w", "u1"), ("h", "u1"), ("ref0", "i1"), ("ref1", "i1"),
                      ("mv0", "<i2", 2), ("mv1", "<i2", 2), ("sliceType", "u1"), ("flags", "u1"), ("wp", MC_WP_DT, (2, 3)), ("metric", "u1"), ("chroma_cost", "u1"), ("reserved", "u1", 4)])
assert MC_JOB_DT.itemsize == 96
MC_W, MC_H, MC_MX, MC_MY = 256, 192, 96, 80


def mc_make_refs(depth, seed, nref=3):
    """nref padded 4:2:0 pictures (Y, U, V planes concatenated per picture); returns (list of arrays, stride, cstride, offsets)"""
    rng = np.random.default_rng(seed)
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    stride, cstride = MC_W + 2 * MC_MX, MC_W // 2 + MC_MX
    rows, crows = MC_H + 2 * MC_MY, MC_H // 2 + MC_MY
    pics = []
    for r in range(nref):
        planes = []
        for (rw, st) in ((rows, stride), (crows, cstride), (crows, cstride)):
            base = rng.integers(0, pmax + 1, (rw // 4 + 1, st // 4 + 1)).astype(np.int64)
            p = np.kron(base, np.ones((4, 4), np.int64))[:rw, :st]
            p = np.clip((p + np.roll(p, 1, 0) + np.roll(p, 2, 1) + rng.integers(-3, 4, p.shape) * 3) // 2, 0, pmax)
            planes.append(p.astype(dt).ravel())
        pics.append(np.concatenate(planes))
    ysz, csz = rows * stride, crows * cstride
    org = (MC_MY * stride + MC_MX, ysz + (MC_MY // 2) * cstride + MC_MX // 2, ysz + csz + (MC_MY // 2) * cstride + MC_MX // 2)
    return pics, stride, cstride, org


def mc_jobs(seed, n):
    rng = np.random.default_rng(seed ^ 0xC0FFEE)
    j = np.zeros(n, MC_JOB_DT)
    for i in range(n):
        w, h = PU_SIZES[int(rng.integers(1, 25))] if i % 2 else [(8, 8), (16, 16), (32, 32), (64, 64)][int(rng.integers(0, 4))]
        cu = max(w, h)
        cux = int(rng.integers(0, MC_W // cu)) * cu; cuy = int(rng.integers(0, MC_H // cu)) * cu
        x = cux + (cu - w if rng.integers(0, 2) else 0); y = cuy + (cu - h if rng.integers(0, 2) else 0)
        j[i]["x"], j[i]["y"], j[i]["cuX"], j[i]["cuY"], j[i]["w"], j[i]["h"] = x, y, cux, cuy, w, h
        p = int(rng.integers(0, 2))
        j[i]["sliceType"] = p
        if p:
            j[i]["ref0"], j[i]["ref1"] = int(rng.integers(0, 3)), -1
        else:
            k = int(rng.integers(0, 3))
            j[i]["ref0"], j[i]["ref1"] = [(int(rng.integers(0, 3)), int(rng.integers(0, 3))), (int(rng.integers(0, 3)), -1), (-1, int(rng.integers(0, 3)))][k]
        far = rng.integers(0, 8) == 0       # occasionally far outside: exercises clipMv
        for key in ("mv0", "mv1"):
            j[i][key] = (int(rng.integers(-2000, 2001)) if far else int(rng.integers(-70, 71)), int(rng.integers(-1500, 1501)) if far else int(rng.integers(-70, 71)))
        if rng.integers(0, 4) == 0:
            j[i][("mv0", "mv1")[int(rng.integers(0, 2))]] = (int(rng.integers(-8, 9)) * 4, int(rng.integers(-8, 9)) * 4)     # full-pel
        flags = 3 if rng.integers(0, 4) else int(rng.integers(1, 3))
        wmode = int(rng.integers(0, 3))
        if wmode:
            flags |= 4 | 8
            for l in range(2):
                pres = int(rng.integers(0, 2)) if wmode == 1 else 1
                for c in range(3):
                    den = int(rng.integers(0, 8)) if c == 0 else int(rng.integers(0, 8))
                    j[i]["wp"][l][c] = (int(rng.integers(-20, 128)), int(rng.integers(-30, 31)), den, pres)
        j[i]["flags"] = flags
    return j


def mc_run_host(L, pics, stride, cstride, org, jobs):
    """through <prefix>motion_compensation_batch with host addresses; returns list of (Y, U, V) arrays (None when a plane is off)"""
    n = len(jobs)
    dt = pics[0].dtype
    isz = dt.itemsize
    planes = np.array([p.ctypes.data + org[c] * isz for p in pics for c in range(3)], np.uint64)
    outY = np.zeros((n, 64, 64), dt); outU = np.zeros((n, 32, 32), dt); outV = np.zeros((n, 32, 32), dt)
    jb = jobs.copy()
    jb["dstY"] = outY.ctypes.data + np.arange(n) * 64 * 64 * isz
    jb["dstU"] = outU.ctypes.data + np.arange(n) * 32 * 32 * isz
    jb["dstV"] = outV.ctypes.data + np.arange(n) * 32 * 32 * isz
    jb["dstStride"], jb["dstCStride"] = 64, 32
    fn = getattr(L.lib, L.prefix + "motion_compensation_batch")
    fn(_ptr(planes), C.c_int64(stride), C.c_int64(cstride), MC_W, MC_H, _ptr(jb), n)
    res = []
    for i in range(n):
        w, h, f = int(jobs[i]["w"]), int(jobs[i]["h"]), int(jobs[i]["flags"])
        res.append((outY[i, :h, :w].copy() if f & 1 else None, outU[i, :h // 2, :w // 2].copy() if f & 2 else None, outV[i, :h // 2, :w // 2].copy() if f & 2 else None))
    return res


def mc_digest(res):
    h = hashlib.sha256()
    for y, u, v in res:
        for a in (y, u, v):
            h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    return h.digest()


def mc_run_hip(L, pics, stride, cstride, org, jobs, stream=None):
    """x265amd_motion_compensation on device memory; same return shape as mc_run_host"""
    import torch
    n = len(jobs)
    dt = pics[0].dtype
    isz = dt.itemsize
    d_pics = [torch.from_numpy(p.view(np.uint8)).cuda() for p in pics]
    planes = np.array([d.data_ptr() + org[c] * isz for d in d_pics for c in range(3)], np.uint64)
    d_planes = torch.from_numpy(planes.view(np.uint8).copy()).cuda()
    d_y = torch.zeros(n * 64 * 64 * isz, dtype=torch.uint8, device="cuda")
    d_u = torch.zeros(n * 32 * 32 * isz, dtype=torch.uint8, device="cuda")
    d_v = torch.zeros(n * 32 * 32 * isz, dtype=torch.uint8, device="cuda")
    jb = jobs.copy()
    jb["dstY"] = d_y.data_ptr() + np.arange(n) * 64 * 64 * isz
    jb["dstU"] = d_u.data_ptr() + np.arange(n) * 32 * 32 * isz
    jb["dstV"] = d_v.data_ptr() + np.arange(n) * 32 * 32 * isz
    jb["dstStride"], jb["dstCStride"] = 64, 32
    d_jobs = torch.from_numpy(jb.view(np.uint8).copy()).cuda()
    with stream_scope(stream) as st:
        rc = L.lib.x265amd_motion_compensation(st, C.c_void_p(d_planes.data_ptr()), C.c_int64(stride), C.c_int64(cstride), MC_W, MC_H,
                                               C.c_void_p(d_jobs.data_ptr()), n)
    assert rc == 0
    outY = d_y.cpu().numpy().view(dt).reshape(n, 64, 64); outU = d_u.cpu().numpy().view(dt).reshape(n, 32, 32); outV = d_v.cpu().numpy().view(dt).reshape(n, 32, 32)
    res = []
    for i in range(n):
        w, h, f = int(jobs[i]["w"]), int(jobs[i]["h"]), int(jobs[i]["flags"])
        res.append((outY[i, :h, :w].copy() if f & 1 else None, outU[i, :h // 2, :w // 2].copy() if f & 2 else None, outV[i, :h // 2, :w // 2].copy() if f & 2 else None))
    return res


# ---- motion estimation with chroma SATD (subme > 2): the encoder form of setSourcePU ----
def me_make_yuv(depth, seed, motion=(5, -3)):
    """(cur, ref) each a list [Y, U, V] of flat padded planes; plus (stride, cstride, originY, originC)"""
    cy, ry, stride, origin = me_make_planes(depth, seed, motion=motion)
    cmarg = ME_MARGIN // 2
    cu, ru, cstride, corg = me_make_planes(depth, seed + 1000, width=128, height=96, motion=(motion[0] // 2, motion[1] // 2), noise=2, margin=cmarg)
    cv, rv, _, _ = me_make_planes(depth, seed + 2000, width=128, height=96, motion=(motion[0] // 2, motion[1] // 2), noise=2, margin=cmarg)
    return [cy, cu, cv], [ry, ru, rv], stride, cstride, origin, corg


def me_run_host_c(L, cur, ref, stride, cstride, origin, corg, jobs, bChroma=1):
    out = np.zeros((len(jobs), 3), np.int32)
    fn = getattr(L.lib, L.prefix + "motion_estimate_c")
    fn.restype = C.c_int
    isz = cur[0].itemsize
    fpl = (C.c_void_p * 3)(cur[0].ctypes.data + origin * isz, cur[1].ctypes.data + corg * isz, cur[2].ctypes.data + corg * isz)
    rpl = (C.c_void_p * 3)(ref[0].ctypes.data + origin * isz, ref[1].ctypes.data + corg * isz, ref[2].ctypes.data + corg * isz)
    for i, j in enumerate(jobs):
        mv = np.zeros(2, np.int32)
        mvc = np.array(j["mvc"], np.int32).reshape(-1) if j["mvc"] else np.zeros(2, np.int32)
        cost = fn(fpl, rpl, C.c_int64(stride), C.c_int64(cstride), j["x"], j["y"], j["w"], j["h"], j["method"], j["subme"], j["qp"],
                  _ptr(np.array(j["mvmin"], np.int32)), _ptr(np.array(j["mvmax"], np.int32)), _ptr(np.array(j["mvp"], np.int32)),
                  len(j["mvc"]), _ptr(mvc), j["merange"], bChroma, _ptr(mv))
        out[i] = (mv[0], mv[1], cost)
    return out


# ----------------------------------------------------------------------------------------------------------
# entropy side of the residual path: contexts, estBit tables, RDOQ, bits-only coefficient coding
# ----------------------------------------------------------------------------------------------------------
CTX_COUNT = 157          # MAX_OFF_CTX_MOD (contexts.h:106)
EST_INTS = 184           # sizeof(EstBitsSbac) / sizeof(int) (entropy.h:88-97)


def entropy_reset(L, sliceType, qp):
    ctx = np.zeros(160, np.uint8)
    getattr(L.lib, L.prefix + "entropy_reset")(sliceType, qp, _ptr(ctx))
    return ctx[:CTX_COUNT].copy()


def est_bit(L, ctx, log2, isLuma):
    est = np.zeros(EST_INTS, np.int32)
    c = np.zeros(160, np.uint8); c[:CTX_COUNT] = ctx[:CTX_COUNT]
    # the product's x265amd_est_bit is the batched device entry; its host-pointer form carries the _host suffix
    getattr(L.lib, L.prefix + ("est_bit_host" if L.prefix == "x265amd_" else "est_bit"))(_ptr(c), log2, isLuma, _ptr(est))
    return est


def rdoq_cases(depth, seed, n, ctxlib=None):
    """tu_cases + RDOQ parameters: tuDepth, rdoq level, psy-rdoq scale (Quant::m_psyRdoqScale = psyRdoq * 256) and a context
    set: slice-start states of a random QP, part of the cases with states perturbed as after some coding"""
    rng = np.random.default_rng(seed + 1000)
    cases = tu_cases(depth, seed, n)
    from_oracle = ctxlib or load_oracle(depth)
    for c in cases:
        if c["ttype"] and c["log2"] == 5:
            c["log2"] = 4
            c["fenc"] = np.ascontiguousarray(c["fenc"][:16, :16]); c["pred"] = np.ascontiguousarray(c["pred"][:16, :16])
        c["tudepth"] = int(rng.integers(0, 3))
        c["rdoq"] = int(rng.integers(1, 3))
        c["psyrdoq"] = int(rng.choice([0, 0, 256, 1024, 2560]))
        ctx = entropy_reset(from_oracle, c["slice"], int(rng.integers(10, 50)))
        if rng.integers(0, 2):
            k = rng.integers(0, CTX_COUNT, 40)
            ctx[k] = rng.integers(0, 124, 40).astype(np.uint8)
        c["ctx"] = ctx
    return cases


def rdoq_run(L, cases):
    """<prefix>transform_tu_rdoq with the estBit tables of the case's contexts; returns list of (numSig, coeff)"""
    out = []
    f = getattr(L.lib, L.prefix + "transform_tu_rdoq"); f.restype = C.c_uint32
    for c in cases:
        N = 1 << c["log2"]
        est = est_bit(L, c["ctx"], c["log2"], int(c["ttype"] == 0))
        resi = (c["fenc"].astype(np.int32) - c["pred"].astype(np.int32)).astype(np.int16)
        coeff = np.zeros(N * N, np.int16)
        ns = f(_ptr(c["fenc"]), C.c_int64(N), _ptr(resi), C.c_int64(N), _ptr(coeff), c["log2"], c["ttype"], c["intra"], c["dir"], c["slice"], c["qp"],
               c["signhide"], c["tudepth"], c["rdoq"], c["psyrdoq"], _ptr(est))
        out.append((int(ns), coeff.copy()))
    return out


def coeff_bits_run(L, cases, levels):
    """<prefix>code_coeff_bits on given level arrays; returns list of (bits FIX15, updated contexts)"""
    out = []
    f = getattr(L.lib, L.prefix + "code_coeff_bits"); f.restype = C.c_uint64
    for c, (ns, coeff) in zip(cases, levels):
        ctx = np.zeros(160, np.uint8); ctx[:CTX_COUNT] = c["ctx"]
        if ns == 0:
            out.append((0, ctx[:CTX_COUNT].copy()))
            continue
        bits = f(_ptr(coeff), c["log2"], c["ttype"], c["intra"], c["dir"], c["signhide"], _ptr(ctx))
        out.append((int(bits), ctx[:CTX_COUNT].copy()))
    return out


TU_RDOQ_DT = np.dtype([("est_bits", "<u8"), ("lambda2", "<i8"), ("lambda_", "<i4"), ("psy_rdoq_scale", "<i4"), ("rdoq_level", "u1"), ("tu_depth", "u1"),
                       ("reserved", "u1", 6)])
EST_JOB_DT = np.dtype([("ctx", "<u8"), ("est", "<u8"), ("log2", "u1"), ("is_luma", "u1"), ("reserved", "u1", 6)])
COEFF_BITS_JOB_DT = np.dtype([("coeff", "<u8"), ("ctx_in", "<u8"), ("ctx_out", "<u8"), ("log2", "u1"), ("ttype", "u1"), ("intra", "u1"), ("dir", "u1"),
                              ("signhide", "u1"), ("reserved", "u1", 3)])
assert TU_RDOQ_DT.itemsize == 32 and EST_JOB_DT.itemsize == 24 and COEFF_BITS_JOB_DT.itemsize == 32


def rdoq_chain_oracle(L, cases):
    """orc_tu_chain_rdoq: list of (stats[5], coeff, resi, recon)"""
    out = []
    for c in cases:
        N = 1 << c["log2"]
        est = est_bit(L, c["ctx"], c["log2"], int(c["ttype"] == 0))
        coeff = np.zeros(N * N, np.int16); resi = np.zeros((N, N), np.int16); recon = np.zeros((N, N), c["fenc"].dtype)
        st = np.zeros(5, np.uint64)
        L.lib.orc_tu_chain_rdoq(_ptr(c["fenc"]), C.c_int64(N), _ptr(c["pred"]), C.c_int64(N), c["log2"], c["ttype"], c["intra"], c["dir"], c["slice"],
                                c["qp"], c["signhide"], c["tudepth"], c["rdoq"], c["psyrdoq"], _ptr(est),
                                _ptr(coeff), _ptr(resi), C.c_int64(N), _ptr(recon), C.c_int64(N), _ptr(st))
        out.append((st.copy(), coeff, resi, recon))
    return out


def est_bit_run_hip(L, ctxs, shapes, stream=None):
    """x265amd_est_bit on a batch: ctxs [n, 160] context states, shapes[i] = (log2, is_luma); returns int32 [n, EST_INTS]"""
    import torch
    n = len(ctxs)
    jobs = np.zeros(n, EST_JOB_DT)
    d_ctx = torch.from_numpy(np.ascontiguousarray(ctxs)).cuda()
    d_est = torch.zeros(n * EST_INTS, dtype=torch.int32, device="cuda")
    for i, (l, lu) in enumerate(shapes):
        jobs[i] = (d_ctx.data_ptr() + i * 160, d_est.data_ptr() + i * EST_INTS * 4, l, lu, 0)
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    with stream_scope(stream) as st:
        rc = L.lib.x265amd_est_bit(st, C.c_void_p(d_jobs.data_ptr()), n)
    assert rc == 0
    return d_est.cpu().numpy().reshape(n, EST_INTS)


def tu_chain_rdoq_run_hip(L, cases, stream=None, coeff_bits=False):
    """x265amd_tu_chain_rdoq on a batch (jobs with rdoq == 0 quantise plainly), estBit tables from the oracle; list of (stats[5], coeff, resi, recon) as
    rdoq_chain_oracle.  coeff_bits=True (NULL stream only): x265amd_coeff_bits on the levels just written, and (chain results, bits [n], contexts out [n, 160])"""
    import torch
    assert not (coeff_bits and stream is not None)
    orc = load_oracle(L.depth)
    dt = L.pixel
    isz = np.dtype(dt).itemsize
    n = len(cases)
    per = 32 * 32 * (isz * 3 + 2 * 2)
    arena = np.zeros(n * per, np.uint8)
    ests = np.stack([est_bit(orc, c["ctx"], c["log2"], int(c["ttype"] == 0)) for c in cases])
    ctxs = np.zeros((n, 160), np.uint8)
    for i, c in enumerate(cases):
        N = 1 << c["log2"]
        base = i * per
        arena[base:base + 1024 * isz].view(dt).reshape(32, 32)[:N, :N] = c["fenc"]
        arena[base + 1024 * isz:base + 2048 * isz].view(dt).reshape(32, 32)[:N, :N] = c["pred"]
        ctxs[i, :CTX_COUNT] = c["ctx"]
    d_arena = torch.from_numpy(arena).cuda()
    d_est = torch.from_numpy(ests).cuda()
    d_ctx = torch.from_numpy(ctxs).cuda()
    d_ctx_out = torch.zeros_like(d_ctx)
    a0 = d_arena.data_ptr()
    jobs = np.zeros(n, TU_JOB_DT); rq = np.zeros(n, TU_RDOQ_DT); cb = np.zeros(n, COEFF_BITS_JOB_DT)
    for i, c in enumerate(cases):
        base = a0 + i * per
        jobs[i] = (base, base + 1024 * isz, base + 3072 * isz, base + 3072 * isz + 2048, base + 2048 * isz, 32, 32, 32, 32,
                   c["log2"], c["ttype"], c["intra"], c["dir"], c["slice"], c["qp"], c["signhide"], 0)
        l2, l1 = C.c_int64(0), C.c_int32(0)
        L.lib.x265amd_rdoq_lambda(c["qp"], C.byref(l2), C.byref(l1))
        rq[i] = (d_est.data_ptr() + i * EST_INTS * 4, l2.value, l1.value, c["psyrdoq"], c["rdoq"], c["tudepth"], 0)
        cb[i] = (base + 3072 * isz, d_ctx.data_ptr() + i * 160, d_ctx_out.data_ptr() + i * 160, c["log2"], c["ttype"], c["intra"], c["dir"], c["signhide"], 0)
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_rq = torch.from_numpy(rq.view(np.uint8).copy()).cuda()
    d_cb = torch.from_numpy(cb.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(n * TU_RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    d_bits = torch.zeros(n, dtype=torch.int64, device="cuda")
    with stream_scope(stream) as st:
        rc = L.lib.x265amd_tu_chain_rdoq(st, C.c_void_p(d_jobs.data_ptr()), C.c_void_p(d_rq.data_ptr()), n, C.c_void_p(d_out.data_ptr()))
        assert rc == 0
        if coeff_bits:
            assert L.lib.x265amd_coeff_bits(None, C.c_void_p(d_cb.data_ptr()), n, C.c_void_p(d_bits.data_ptr())) == 0
    chain = tu_chain_unpack(cases, d_out.cpu().numpy().view(TU_RESULT_DT), d_arena.cpu().numpy(), per, dt)
    if coeff_bits:
        return chain, d_bits.cpu().numpy().astype(np.uint64), d_ctx_out.cpu().numpy()
    return chain


# ---- distortion of inter prediction candidates (x265amd_inter_cost): MC jobs + a metric ----
def inter_cost_jobs(seed, n):
    """mc_jobs with the decision metrics of the reference: SAD (selectMVP), SATD (+chroma: mergeEstimation / bi-prediction
    tries), SA8D on square PUs (+chroma: merge scan), and the pixel-average form of the bi-prediction try"""
    rng = np.random.default_rng(seed ^ 0xBEEF)
    j = mc_jobs(seed, n)
    for i in range(n):
        w, h = int(j[i]["w"]), int(j[i]["h"])
        kind = int(rng.integers(0, 4))
        if kind == 0:                       # selectMVP: luma pixel path of one list, SAD
            j[i]["metric"], j[i]["chroma_cost"] = 1, 0
            j[i]["flags"] = 1
            j[i]["sliceType"] = 1
            if j[i]["ref0"] < 0:
                j[i]["ref0"], j[i]["ref1"] = 0, -1
        elif kind == 1:                     # merge estimation / bidir with chroma SATD
            j[i]["metric"] = 2
            ok = (w // 2) % 4 == 0 and (h // 2) % 4 == 0
            j[i]["chroma_cost"] = 1 if ok and rng.integers(0, 2) else 0
            j[i]["flags"] = (int(j[i]["flags"]) & ~3) | (3 if j[i]["chroma_cost"] else 1)
        elif kind == 2:                     # merge scan: square PU = CU, SA8D (+ chroma for CU >= 16)
            s = int(rng.choice([8, 16, 32, 64]))
            cux = int(rng.integers(0, MC_W // s)) * s; cuy = int(rng.integers(0, MC_H // s)) * s
            j[i]["x"], j[i]["y"], j[i]["cuX"], j[i]["cuY"], j[i]["w"], j[i]["h"] = cux, cuy, cux, cuy, s, s
            j[i]["metric"] = 3
            j[i]["chroma_cost"] = 1 if s >= 16 and rng.integers(0, 2) else 0
            j[i]["flags"] = (int(j[i]["flags"]) & ~3) | (3 if j[i]["chroma_cost"] else 1)
        else:                               # bi-prediction try without chroma SATD: pixel average, SATD
            j[i]["metric"], j[i]["chroma_cost"] = 2, 0
            j[i]["sliceType"] = 0
            j[i]["ref0"], j[i]["ref1"] = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            j[i]["flags"] = 1 | 16
            if rng.integers(0, 3) == 0:
                j[i]["mv0"] = (0, 0); j[i]["mv1"] = (0, 0)
    return j


def inter_cost_run_host(L, pics, fenc, stride, cstride, org, jobs):
    """<prefix>inter_cost_batch with host addresses: (n x 2 costs, predictions as mc_run_host)"""
    n = len(jobs)
    dt = pics[0].dtype
    isz = dt.itemsize
    planes = np.array([p.ctypes.data + org[c] * isz for p in pics for c in range(3)], np.uint64)
    fplanes = np.array([fenc.ctypes.data + org[c] * isz for c in range(3)], np.uint64)
    outY = np.zeros((n, 64, 64), dt); outU = np.zeros((n, 32, 32), dt); outV = np.zeros((n, 32, 32), dt)
    jb = jobs.copy()
    jb["dstY"] = outY.ctypes.data + np.arange(n) * 64 * 64 * isz
    jb["dstU"] = outU.ctypes.data + np.arange(n) * 32 * 32 * isz
    jb["dstV"] = outV.ctypes.data + np.arange(n) * 32 * 32 * isz
    jb["dstStride"], jb["dstCStride"] = 64, 32
    cost = np.zeros((n, 2), np.uint32)
    getattr(L.lib, L.prefix + "inter_cost_batch")(_ptr(planes), C.c_int64(stride), C.c_int64(cstride), MC_W, MC_H, _ptr(jb), n,
                                                  _ptr(fplanes), C.c_int64(stride), C.c_int64(cstride), _ptr(cost))
    return cost, [outY[i, :int(jobs[i]["h"]), :int(jobs[i]["w"])].copy() for i in range(n)]


def inter_cost_run_hip(L, pics, fenc, stride, cstride, org, jobs, stream=None):
    import torch
    n = len(jobs)
    dt = pics[0].dtype
    isz = dt.itemsize
    d_pics = [torch.from_numpy(p.view(np.uint8)).cuda() for p in pics]
    d_fenc = torch.from_numpy(fenc.view(np.uint8)).cuda()
    planes = np.array([d.data_ptr() + org[c] * isz for d in d_pics for c in range(3)], np.uint64)
    fplanes = np.array([d_fenc.data_ptr() + org[c] * isz for c in range(3)], np.uint64)
    d_planes = torch.from_numpy(planes.view(np.uint8).copy()).cuda()
    d_fplanes = torch.from_numpy(fplanes.view(np.uint8).copy()).cuda()
    d_y = torch.zeros(n * 64 * 64 * isz, dtype=torch.uint8, device="cuda")
    d_u = torch.zeros(n * 32 * 32 * isz, dtype=torch.uint8, device="cuda")
    d_v = torch.zeros(n * 32 * 32 * isz, dtype=torch.uint8, device="cuda")
    jb = jobs.copy()
    jb["dstY"] = d_y.data_ptr() + np.arange(n) * 64 * 64 * isz
    jb["dstU"] = d_u.data_ptr() + np.arange(n) * 32 * 32 * isz
    jb["dstV"] = d_v.data_ptr() + np.arange(n) * 32 * 32 * isz
    jb["dstStride"], jb["dstCStride"] = 64, 32
    d_jobs = torch.from_numpy(jb.view(np.uint8).copy()).cuda()
    d_cost = torch.zeros(n * 2, dtype=torch.int32, device="cuda")
    with stream_scope(stream) as st:
        rc = L.lib.x265amd_inter_cost(st, C.c_void_p(d_planes.data_ptr()), C.c_int64(stride), C.c_int64(cstride), MC_W, MC_H,
                                      C.c_void_p(d_jobs.data_ptr()), n, C.c_void_p(d_fplanes.data_ptr()), C.c_int64(stride), C.c_int64(cstride),
                                      C.c_void_p(d_cost.data_ptr()))
    assert rc == 0
    outY = d_y.cpu().numpy().view(dt).reshape(n, 64, 64)
    return d_cost.cpu().numpy().view(np.uint32).reshape(n, 2), [outY[i, :int(jobs[i]["h"]), :int(jobs[i]["w"])].copy() for i in range(n)]


# ---- fused intra TU jobs: prediction from the reconstructed plane + per-TU measurement (x265amd_intra_tu_chain) ----
INTRA_TU_JOB_DT = np.dtype([("tu", TU_JOB_DT), ("nb", "<u8"), ("avail", "<u8"), ("nb_stride", "<i4"), ("strong", "u1"), ("reserved", "u1", 11)])
assert INTRA_TU_JOB_DT.itemsize == 96


def intra_tu_cases(depth, seed, n, rdoq=False):
    """intra_cases + a prediction mode, plane type and the TU parameters; with rdoq=True also the RDOQ parameters and contexts"""
    rng = np.random.default_rng(seed + 4242)
    cases = intra_cases(depth, seed, n)
    orc = load_oracle(depth)
    for c in cases:
        c["ttype"] = int(rng.integers(0, 3))
        c["mode"] = int(rng.integers(0, 35)) if c["ttype"] == 0 else int(rng.choice([0, 1, 10, 26, 34, int(rng.integers(2, 35))]))
        c["slice"] = int(rng.integers(0, 3))
        c["qp"] = int(rng.integers(4, 52)) + 6 * (depth - 8)
        c["signhide"] = int(rng.integers(0, 4) != 0)
        c["rdoq"] = int(rng.integers(0, 3)) if rdoq else 0
        c["tudepth"] = int(rng.integers(0, 3))
        c["psyrdoq"] = int(rng.choice([0, 256, 1024]))
        c["ctx"] = entropy_reset(orc, c["slice"], int(rng.integers(10, 50)))
    return cases


def intra_predict_host(L, cases):
    out = []
    f = getattr(L.lib, L.prefix + "intra_predict")
    for c in cases:
        N = 1 << c["log2"]
        pred = np.zeros((N, N), c["plane"].dtype)
        f(off(c["plane"], c["off"]), C.c_int64(c["stride"]), c["log2"], _ptr(c["flags"]), c["strong"], int(c["ttype"] != 0), c["mode"], _ptr(pred), C.c_int64(N))
        out.append(pred)
    return out


def intra_tu_pack(cases, addr_plane, addr_fenc, addr_out, est_addr=None, L=None):
    """job / rdoq records; addr_*(i) -> base address of case i's plane, fenc and output area (pred | recon | coeff | resi at stride 32)"""
    n = len(cases)
    jobs = np.zeros(n, INTRA_TU_JOB_DT); rq = np.zeros(n, TU_RDOQ_DT)
    isz = cases[0]["plane"].itemsize
    for i, c in enumerate(cases):
        N = 1 << c["log2"]
        o = addr_out(i)
        mask = 0
        for u, f in enumerate(c["flags"]):
            mask |= int(f) << u
        jobs[i]["tu"] = (addr_fenc(i), o, o + 2048 * isz, o + 2048 * isz + 2048, o + 1024 * isz, N, 32, 32, 32,
                         c["log2"], c["ttype"], 1, c["mode"], c["slice"], c["qp"], c["signhide"], 0)
        jobs[i]["nb"] = addr_plane(i) + c["off"] * isz
        jobs[i]["avail"], jobs[i]["nb_stride"], jobs[i]["strong"] = mask, c["stride"], c["strong"]
        if c["rdoq"]:
            l2, l1 = C.c_int64(0), C.c_int32(0)
            L.lib.x265amd_rdoq_lambda(c["qp"], C.byref(l2), C.byref(l1)) if L is not None and L.prefix == "x265amd_" else None
            rq[i] = (est_addr(i), l2.value, l1.value, c["psyrdoq"], c["rdoq"], c["tudepth"], 0)
    return jobs, rq


INTRA_TU_OUT_BYTES = lambda isz: 1024 * isz * 2 + 4096


def intra_tu_run_host(L, cases):
    """<prefix>intra_tu_chain_batch on host memory: list of (stats tuple, pred, recon, coeff, resi)"""
    n = len(cases)
    dt = cases[0]["plane"].dtype
    isz = dt.itemsize
    per = INTRA_TU_OUT_BYTES(isz)
    arena = np.zeros(n * per, np.uint8)
    ests = np.stack([est_bit(L, c["ctx"], c["log2"], int(c["ttype"] == 0)) for c in cases])
    jobs, rq = intra_tu_pack(cases, lambda i: cases[i]["plane"].ctypes.data, lambda i: cases[i]["fenc"].ctypes.data, lambda i: arena.ctypes.data + i * per,
                             lambda i: ests.ctypes.data + i * EST_INTS * 4)
    res = np.zeros(n, TU_RESULT_DT)
    getattr(L.lib, L.prefix + "intra_tu_chain_batch")(_ptr(jobs), _ptr(rq), n, _ptr(res))
    return intra_tu_unpack(cases, res, arena, per)


def intra_tu_unpack(cases, res, arena, per):
    dt = cases[0]["plane"].dtype
    isz = dt.itemsize
    out = []
    for i, c in enumerate(cases):
        N = 1 << c["log2"]
        b = i * per
        pred = arena[b:b + 1024 * isz].view(dt).reshape(32, 32)[:N, :N].copy()
        recon = arena[b + 1024 * isz:b + 2048 * isz].view(dt).reshape(32, 32)[:N, :N].copy()
        coeff = arena[b + 2048 * isz:b + 2048 * isz + N * N * 2].view(np.int16).copy()
        resi = arena[b + 2048 * isz + 2048:b + 2048 * isz + 4096].view(np.int16).reshape(32, 32)[:N, :N].copy()
        st = (int(res[i]["num_sig"]), int(res[i]["zero_dist"]), int(res[i]["zero_energy"]), int(res[i]["nz_dist"]), int(res[i]["nz_energy"]))
        out.append((st, pred, recon, coeff, resi))
    return out


def intra_tu_run_hip(L, cases, stream=None):
    import torch
    n = len(cases)
    dt = cases[0]["plane"].dtype
    isz = dt.itemsize
    per = INTRA_TU_OUT_BYTES(isz)
    orc = load_oracle(L.depth)
    ests = np.stack([est_bit(orc, c["ctx"], c["log2"], int(c["ttype"] == 0)) for c in cases])
    planes = np.concatenate([c["plane"].view(np.uint8) for c in cases])
    fencs = np.concatenate([c["fenc"].ravel().view(np.uint8) for c in cases])
    po = np.cumsum([0] + [c["plane"].nbytes for c in cases]); fo = np.cumsum([0] + [c["fenc"].nbytes for c in cases])
    d_planes, d_fencs, d_est = torch.from_numpy(planes).cuda(), torch.from_numpy(fencs).cuda(), torch.from_numpy(ests).cuda()
    d_arena = torch.zeros(n * per, dtype=torch.uint8, device="cuda")
    jobs, rq = intra_tu_pack(cases, lambda i: d_planes.data_ptr() + int(po[i]), lambda i: d_fencs.data_ptr() + int(fo[i]), lambda i: d_arena.data_ptr() + i * per,
                             lambda i: d_est.data_ptr() + i * EST_INTS * 4, L)
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    d_rq = torch.from_numpy(rq.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(n * TU_RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    with stream_scope(stream) as st:
        rc = L.lib.x265amd_intra_tu_chain(st, C.c_void_p(d_jobs.data_ptr()), C.c_void_p(d_rq.data_ptr()) if any(c["rdoq"] for c in cases) else None, n,
                                          C.c_void_p(d_out.data_ptr()))
    assert rc == 0
    return intra_tu_unpack(cases, d_out.cpu().numpy().view(TU_RESULT_DT), d_arena.cpu().numpy(), per)


# ---- reference-plane production: extendPicBorder / MotionReference::applyWeight ----
def plane_cases(depth, seed):
    """(plane array incl. margins with garbage in the margins, stride, w, h, mx, my, weight, offset, denom)"""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if depth == 8 else np.uint16
    pmax = (1 << depth) - 1
    out = []
    for (w, h, mx, my) in ((200, 120, 96, 80), (96, 72, 48, 40), (64, 136, 16, 8), (130, 70, 32, 24), (352, 288, 96, 80)):
        stride = w + 2 * mx
        buf = rng.integers(0, pmax + 1, (h + 2 * my) * stride).astype(dt)
        denom = int(rng.integers(0, 8))
        out.append(dict(buf=buf, stride=stride, w=w, h=h, mx=mx, my=my, org=my * stride + mx,
                        weight=int(rng.integers(1, 128)) if denom else 1, offset=int(rng.integers(-20, 21)), denom=denom))
    return out


def plane_run_host(L, cases):
    res = []
    fe = getattr(L.lib, L.prefix + "extend_pic_border"); fw = getattr(L.lib, L.prefix + "weight_plane")
    for c in cases:
        a = c["buf"].copy()
        fe(off(a, c["org"]), C.c_int64(c["stride"]), c["w"], c["h"], c["mx"], c["my"])
        b = np.zeros_like(c["buf"])
        fw(off(c["buf"], c["org"]), off(b, c["org"]), C.c_int64(c["stride"]), c["w"], c["h"], c["mx"], c["my"], c["weight"], c["offset"], c["denom"])
        res.append((a, b))
    return res


def plane_run_hip(L, cases):
    import torch
    res = []
    for c in cases:
        isz = c["buf"].itemsize
        d_a = torch.from_numpy(c["buf"].view(np.uint8).copy()).cuda()
        d_s = torch.from_numpy(c["buf"].view(np.uint8).copy()).cuda()
        d_b = torch.zeros_like(d_s)
        assert L.lib.x265amd_extend_pic_border(None, C.c_void_p(d_a.data_ptr() + c["org"] * isz), C.c_int64(c["stride"]), c["w"], c["h"], c["mx"], c["my"]) == 0
        assert L.lib.x265amd_weight_plane(None, C.c_void_p(d_s.data_ptr() + c["org"] * isz), C.c_void_p(d_b.data_ptr() + c["org"] * isz), C.c_int64(c["stride"]),
                                          c["w"], c["h"], c["mx"], c["my"], c["weight"], c["offset"], c["denom"]) == 0
        torch.cuda.synchronize()
        res.append((d_a.cpu().numpy().view(c["buf"].dtype), d_b.cpu().numpy().view(c["buf"].dtype)))
    return res


# ---- in-loop deblocking of a picture described per 4x4 unit ----
DB_UNIT_DT = np.dtype([("flags", "u1"), ("qp", "i1"), ("ref", "i1", 2), ("mv", "<i2", (2, 2))])
REF_DB_UNIT_DT = np.dtype([("log2CU", "u1"), ("partSize", "u1"), ("tuDepth", "u1"), ("intra", "u1"), ("cbf", "u1"), ("bypass", "u1"), ("qp", "i1"),
                           ("ref", "i1", 2), ("pad", "u1"), ("mv", "<i2", (2, 2))])
assert DB_UNIT_DT.itemsize == 12 and REF_DB_UNIT_DT.itemsize == 18
DB_INTRA, DB_CBF, DB_BYPASS, DB_TU_LEFT, DB_PU_LEFT, DB_TU_TOP, DB_PU_TOP = 1, 2, 4, 8, 16, 32, 64
# PU rectangles (x, y, w, h in quarters of the CU) per PartSize (SIZE_2Nx2N .. SIZE_nRx2N, common.h)
_PU_RECTS = {0: [(0, 0, 4, 4)], 1: [(0, 0, 4, 2), (0, 2, 4, 2)], 2: [(0, 0, 2, 4), (2, 0, 2, 4)], 3: [(0, 0, 2, 2), (2, 0, 2, 2), (0, 2, 2, 2), (2, 2, 2, 2)],
             4: [(0, 0, 4, 1), (0, 1, 4, 3)], 5: [(0, 0, 4, 3), (0, 3, 4, 1)], 6: [(0, 0, 1, 4), (1, 0, 3, 4)], 7: [(0, 0, 3, 4), (3, 0, 1, 4)]}


def deblock_case(depth, seed, width, height, slice_b=True, bypass=False, qp_range=(18, 46)):
    """a random coding quad-tree over a width x height picture (multiples of 8): returns dict with padded planes, the raster
    records for the reference driver (REF_DB_UNIT_DT) and for the oracle / product (DB_UNIT_DT), and the PPS offsets.  qp_range: the half-open range the
    QP of a CU is drawn from (the default is what every committed digest was made with; tests/test_filter_edges.py asks for the whole 0 .. 51)"""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if depth == 8 else np.uint16
    pmax = (1 << depth) - 1
    w4, h4 = width // 4, height // 4
    ru = np.zeros((h4, w4), REF_DB_UNIT_DT)
    du = np.zeros((h4, w4), DB_UNIT_DT)

    def tu_split(x, y, size, d, maxd, cuinfo):
        if d < maxd and size > 4 and (size > 32 or rng.integers(0, 2)):
            for k in range(4):
                tu_split(x + (k & 1) * size // 2, y + (k >> 1) * size // 2, size // 2, d + 1, maxd, cuinfo)
            return
        cbf = int(rng.integers(0, 2))
        ys, xs = slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4)
        ru["tuDepth"][ys, xs] = d; ru["cbf"][ys, xs] = cbf
        du["flags"][ys, xs] |= cbf * DB_CBF
        du["flags"][ys, x // 4] |= DB_TU_LEFT
        du["flags"][y // 4, xs] |= DB_TU_TOP

    def leaf(x, y, size):
        log2 = int(np.log2(size))
        intra = int(rng.integers(0, 4) == 0)
        if intra:
            part = 3 if (size == 8 and rng.integers(0, 2)) else 0
        else:
            part = int(rng.choice([0, 0, 1, 2] + ([4, 5, 6, 7] if size >= 16 else [])))
        qp = int(rng.integers(*qp_range))
        byp = int(bypass and rng.integers(0, 6) == 0)
        ys, xs = slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4)
        ru["log2CU"][ys, xs] = log2; ru["partSize"][ys, xs] = part; ru["intra"][ys, xs] = intra; ru["qp"][ys, xs] = qp; ru["bypass"][ys, xs] = byp
        du["qp"][ys, xs] = qp
        du["flags"][ys, xs] |= intra * DB_INTRA + byp * DB_BYPASS
        q = size // 4
        for (px, py, pw, ph) in _PU_RECTS[part]:
            pys, pxs = slice((y + py * q) // 4, (y + (py + ph) * q) // 4), slice((x + px * q) // 4, (x + (px + pw) * q) // 4)
            if intra:
                refs, mvs = (-1, -1), ((0, 0), (0, 0))
            else:
                kind = int(rng.integers(0, 3)) if slice_b else 0
                refs = [(int(rng.integers(0, 3)), -1), (-1, int(rng.integers(0, 3))), (int(rng.integers(0, 3)), int(rng.integers(0, 3)))][kind]
                base = (int(rng.integers(-6, 7)), int(rng.integers(-6, 7)))
                mvs = tuple((base[0] + int(rng.integers(-3, 4)), base[1] + int(rng.integers(-3, 4))) if refs[l] >= 0 else (0, 0) for l in range(2))
            for arr in (ru, du):
                arr["ref"][pys, pxs] = refs
                arr["mv"][pys, pxs] = mvs
            if px:
                du["flags"][pys, (x + px * q) // 4] |= DB_PU_LEFT
            if py:
                du["flags"][(y + py * q) // 4, pxs] |= DB_PU_TOP
        maxd = int(rng.integers(0, 3))
        if part == 3 or size == 64:
            maxd = max(maxd, 1)
        tu_split(x, y, size, 0, min(maxd, log2 - 2), None)

    def cu(x, y, size):
        if x >= width or y >= height:
            return
        inside = x + size <= width and y + size <= height
        if size > 8 and (not inside or rng.integers(0, 3) > 0):
            for k in range(4):
                cu(x + (k & 1) * size // 2, y + (k >> 1) * size // 2, size // 2)
            return
        leaf(x, y, size)

    for cy in range(0, height, 64):
        for cx in range(0, width, 64):
            cu(cx, cy, 64)
    mx, my = 16, 16
    stride, cstride = width + 2 * mx, width // 2 + mx
    planes = []
    for (w, h, st, m) in ((width, height, stride, mx), (width // 2, height // 2, cstride, mx // 2), (width // 2, height // 2, cstride, mx // 2)):
        base = rng.integers(0, pmax + 1, (h // 8 + 1, w // 8 + 1)).astype(np.int64)
        p = np.kron(base, np.ones((8, 8), np.int64))[:h, :w]
        p = np.clip(p // 3 + pmax // 3 + rng.integers(-2, 3, p.shape) * (1 << (depth - 8)), 0, pmax)     # blocky with small steps: all filter branches fire
        full = np.zeros((h + 2 * m, st), dt)
        full[m:m + h, m:m + w] = p
        planes.append(full)
    return dict(planes=planes, stride=stride, cstride=cstride, org=(my * stride + mx, (my // 2) * cstride + mx // 2), width=width, height=height,
                ref_units=np.ascontiguousarray(ru.ravel()), units=np.ascontiguousarray(du.ravel()),
                beta=int(rng.integers(-3, 4)), tc=int(rng.integers(-3, 4)), cb=int(rng.integers(-4, 5)), cr=int(rng.integers(-4, 5)),
                bypass=int(bypass), slice_p=int(not slice_b))


def deblock_run_host(L, c, passes=3):
    pl = [p.copy() for p in c["planes"]]
    isz = pl[0].itemsize
    ptrs = np.array([pl[0].ctypes.data + c["org"][0] * isz, pl[1].ctypes.data + c["org"][1] * isz, pl[2].ctypes.data + c["org"][1] * isz], np.uint64)
    if L.prefix == "ref_":
        L.lib.ref_deblock_picture(_ptr(ptrs), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), c["width"], c["height"], _ptr(c["ref_units"]),
                                  c["beta"], c["tc"], c["cb"], c["cr"], c["bypass"], c["slice_p"], passes)
    else:
        L.lib.orc_deblock_picture(_ptr(ptrs), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), c["width"], c["height"], _ptr(c["units"]),
                                  c["beta"], c["tc"], c["cb"], c["cr"], c["bypass"], passes)
    return pl


def deblock_run_hip(L, c, passes=3):
    import torch
    isz = c["planes"][0].itemsize
    d = [torch.from_numpy(p.view(np.uint8).copy()).cuda() for p in c["planes"]]
    d_units = torch.from_numpy(c["units"].view(np.uint8).copy()).cuda()
    rc = L.lib.x265amd_deblock_picture(None, C.c_void_p(d[0].data_ptr() + c["org"][0] * isz), C.c_void_p(d[1].data_ptr() + c["org"][1] * isz),
                                       C.c_void_p(d[2].data_ptr() + c["org"][1] * isz), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), c["width"], c["height"],
                                       C.c_void_p(d_units.data_ptr()), c["beta"], c["tc"], c["cb"], c["cr"], c["bypass"], passes)
    assert rc == 0
    torch.cuda.synchronize()
    return [t.cpu().numpy().view(c["planes"][0].dtype).reshape(p.shape) for t, p in zip(d, c["planes"])]


# ---- sample adaptive offset: statistics and application over a picture ----
SAO_CTU_DT = np.dtype([("type", "i1", 2), ("bandPos", "u1", 3), ("offset", "i1", (3, 4)), ("pad", "u1", 3)])
assert SAO_CTU_DT.itemsize == 20


def sao_case(depth, seed, width, height):
    rng = np.random.default_rng(seed)
    dt = np.uint8 if depth == 8 else np.uint16
    pmax = (1 << depth) - 1
    mx = 16
    stride, cstride = width + 2 * mx, width // 2 + mx
    rec, fenc = [], []
    for (w, h, st, m) in ((width, height, stride, mx), (width // 2, height // 2, cstride, mx // 2), (width // 2, height // 2, cstride, mx // 2)):
        base = rng.integers(0, pmax + 1, (h // 4 + 2, w // 4 + 2)).astype(np.int64)
        p = np.kron(base, np.ones((4, 4), np.int64))[:h + 2 * m, :st] if False else None
        full = rng.integers(0, pmax + 1, (h + 2 * m, st)).astype(np.int64)
        smooth = (full + np.roll(full, 1, 0) + np.roll(full, 1, 1) + np.roll(full, -1, 0)) // 4
        kind = rng.integers(0, 2)
        r = smooth if kind else (smooth // 8) * 8 + rng.integers(0, 3, smooth.shape)
        f = np.clip(r + rng.integers(-6, 7, r.shape), 0, pmax)
        rec.append(np.ascontiguousarray(np.clip(r, 0, pmax).astype(dt))); fenc.append(np.ascontiguousarray(f.astype(dt)))
    nctu = ((width + 63) // 64) * ((height + 63) // 64)
    params = np.zeros(nctu, SAO_CTU_DT)
    params["type"] = rng.integers(-1, 5, (nctu, 2))
    params["bandPos"] = rng.integers(0, 32, (nctu, 3))
    params["offset"] = rng.integers(-7, 8, (nctu, 3, 4)) * (1 if depth == 8 else 3)
    return dict(rec=rec, fenc=fenc, stride=stride, cstride=cstride, org=(mx * stride + mx, (mx // 2) * cstride + mx // 2), width=width, height=height,
                params=params, nctu=nctu)


def _plane_ptrs(planes, org):
    isz = planes[0].itemsize
    return np.array([planes[0].ctypes.data + org[0] * isz, planes[1].ctypes.data + org[1] * isz, planes[2].ctypes.data + org[1] * isz], np.uint64)


def sao_run_host(L, c):
    """returns (count, offsetOrg, offset planes)"""
    n = c["nctu"] * 3 * 5 * 32
    cnt = np.zeros(n, np.int32); org = np.zeros(n, np.int32)
    rp, fp = _plane_ptrs(c["rec"], c["org"]), _plane_ptrs(c["fenc"], c["org"])
    getattr(L.lib, L.prefix + "sao_stats_picture")(_ptr(rp), _ptr(fp), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), c["width"], c["height"], _ptr(cnt), _ptr(org))
    if L.prefix == "ref_":
        work = [p.copy() for p in c["rec"]]
        L.lib.ref_sao_apply_picture(_ptr(_plane_ptrs(work, c["org"])), _ptr(rp), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), c["width"], c["height"], _ptr(c["params"]))
        out = work
    else:
        out = [p.copy() for p in c["rec"]]
        L.lib.orc_sao_apply_picture(_ptr(rp), _ptr(_plane_ptrs(out, c["org"])), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), c["width"], c["height"], _ptr(c["params"]))
    return cnt, org, out


def sao_run_hip(L, c):
    import torch
    isz = c["rec"][0].itemsize
    d_rec = [torch.from_numpy(p.view(np.uint8).copy()).cuda() for p in c["rec"]]
    d_fenc = [torch.from_numpy(p.view(np.uint8).copy()).cuda() for p in c["fenc"]]
    d_out = [torch.from_numpy(p.view(np.uint8).copy()).cuda() for p in c["rec"]]
    tab = lambda ds: np.array([ds[0].data_ptr() + c["org"][0] * isz, ds[1].data_ptr() + c["org"][1] * isz, ds[2].data_ptr() + c["org"][1] * isz], np.uint64)
    n = c["nctu"] * 3 * 5 * 32
    d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda"); d_org = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_par = torch.from_numpy(c["params"].view(np.uint8).copy()).cuda()
    assert L.lib.x265amd_sao_stats(None, _ptr(tab(d_rec)), _ptr(tab(d_fenc)), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), c["width"], c["height"],
                                   C.c_void_p(d_cnt.data_ptr()), C.c_void_p(d_org.data_ptr())) == 0
    assert L.lib.x265amd_sao_apply(None, _ptr(tab(d_rec)), _ptr(tab(d_out)), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), c["width"], c["height"],
                                   C.c_void_p(d_par.data_ptr())) == 0
    torch.cuda.synchronize()
    dt = c["rec"][0].dtype
    return d_cnt.cpu().numpy(), d_org.cpu().numpy(), [t.cpu().numpy().view(dt).reshape(p.shape) for t, p in zip(d_out, c["rec"])]


# ---- final entropy coding of CTUs (x265amd_cabac_*): random valid coding trees ----
CU_UNIT_DT = np.dtype([("depth", "u1"), ("pred_mode", "u1"), ("part_size", "u1"), ("tu_depth", "u1"), ("luma_dir", "u1"), ("chroma_dir", "u1"),
                       ("merge_flag", "u1"), ("inter_dir", "u1"), ("cbf", "u1", 3), ("tq_bypass", "u1"), ("qp", "i1"), ("ref_idx", "i1", 2),
                       ("mvp_idx", "u1", 2), ("reserved", "u1"), ("mvd", "<i2", (2, 2))])
SLICE_INFO_DT = np.dtype([(n, "<i4") for n in ("pic_width", "pic_height", "slice_type", "slice_qp")] + [("num_ref_idx", "<i4", 2)] +
                         [(n, "<i4") for n in ("max_num_merge_cand", "use_dqp", "max_cu_dqp_depth", "sign_hide", "tq_bypass_enabled", "wpp", "max_cu_depth",
                                               "max_amp_depth", "tu_log2_min", "tu_log2_max", "tu_max_depth_inter", "tu_max_depth_intra")])
assert CU_UNIT_DT.itemsize == 26 and SLICE_INFO_DT.itemsize == 72
MODE_NONE, MODE_INTER, MODE_INTRA, MODE_SKIP = 0, 1, 2, 3
CTU_COEFFS = 64 * 64 + 2 * 32 * 32


def _zorder(x4, y4):
    z = 0
    for b in range(4):
        z |= ((x4 >> b) & 1) << (2 * b) | ((y4 >> b) & 1) << (2 * b + 1)
    return z


def cabac_case(seed, width, height, slice_type, dense=False):
    """random picture of valid CU / PU / TU decisions + levels: dict(si, units (h4 x w4), coeff (numCtu x CTU_COEFFS))"""
    rng = np.random.default_rng(seed)
    w4, h4 = width // 4, height // 4
    ctuW, ctuH = (width + 63) // 64, (height + 63) // 64
    si = np.zeros(1, SLICE_INFO_DT)[0]
    si["pic_width"], si["pic_height"], si["slice_type"], si["slice_qp"] = width, height, slice_type, int(rng.integers(20, 40))
    si["num_ref_idx"] = (int(rng.integers(1, 5)), int(rng.integers(1, 4)) if slice_type == 0 else 0)
    si["max_num_merge_cand"] = int(rng.integers(1, 6))
    si["use_dqp"], si["max_cu_dqp_depth"] = int(rng.integers(0, 2)), int(rng.integers(0, 3))
    si["sign_hide"], si["tq_bypass_enabled"], si["wpp"] = int(rng.integers(0, 2)), int(rng.integers(0, 4) == 0), int(rng.integers(0, 2))
    si["max_cu_depth"], si["max_amp_depth"] = 3, int(rng.choice([0, 3]))
    si["tu_log2_min"], si["tu_log2_max"] = 2, 5
    si["tu_max_depth_inter"], si["tu_max_depth_intra"] = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    units = np.zeros((h4, w4), CU_UNIT_DT)
    coeff = np.zeros((ctuW * ctuH, CTU_COEFFS), np.int16)
    qg = 64 >> int(si["max_cu_dqp_depth"])
    qgqp = {}

    def levels(n):
        a = np.zeros(n * n, np.int16)
        k = int(rng.integers(1, max(2, (n * n) // (2 if dense else 6))))
        idx = rng.choice(n * n, size=min(k, n * n), replace=False)
        mag = rng.choice([1, 1, 1, 2, 2, 3, 4, 7, 15, 40, 300], size=len(idx))
        a[idx] = (mag * rng.choice([-1, 1], size=len(idx))).astype(np.int16)
        if rng.integers(0, 3) == 0:         # low-frequency concentration like real transforms
            a[n * 2:] = 0 if n > 4 else a[n * 2:]
            if not a.any():
                a[0] = 1
        return a

    def put(plane, x, y, n, a):
        addr = (y // 64) * ctuW + (x // 64)
        z = _zorder((x % 64) // 4, (y % 64) // 4)
        off = (z << 4) if plane == 0 else (64 * 64 + (plane - 1) * 32 * 32 + ((z << 4) >> 2))
        coeff[addr, off:off + n * n] = a

    def tu(x, y, log2, d, cu):
        """returns (cbfY, cbfU, cbfV) ORs of the subtree; sets tu_depth and cbf bits"""
        size = 1 << log2
        intra, part, lo = cu["intra"], cu["part"], cu["lo"]
        if intra and part != 0 and log2 == 3:
            sub = True
        elif (not intra) and part != 0 and d == 0 and si["tu_max_depth_inter"] == 1:
            sub = True
        elif log2 > si["tu_log2_max"]:
            sub = True
        elif log2 == si["tu_log2_min"] or log2 == lo:
            sub = False
        else:
            sub = bool(rng.integers(0, 2))
        ys, xs = slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4)
        if sub:
            small_child = log2 - 1 == 2          # children are 4x4 luma: chroma stays at this level
            res = [tu(x + (k & 1) * size // 2, y + (k >> 1) * size // 2, log2 - 1, d + 1, cu) for k in range(4)]
            cy = any(r[0] for r in res)
            if small_child:
                cu_, cv_ = bool(rng.integers(0, 2)) and not cu["nores"], bool(rng.integers(0, 2)) and not cu["nores"]
                for c, v in ((1, cu_), (2, cv_)):
                    if v:
                        units["cbf"][ys, xs, c] |= (1 << d) | (1 << (d + 1))
                        put(c, x, y, 4, levels(4))
            else:
                cu_, cv_ = any(r[1] for r in res), any(r[2] for r in res)
                for c, v in ((1, cu_), (2, cv_)):
                    if v:
                        units["cbf"][ys, xs, c] |= 1 << d
            if cy:
                units["cbf"][ys, xs, 0] |= 1 << d
            return cy, cu_, cv_
        units["tu_depth"][ys, xs] = d
        out = []
        for c in range(3):
            if c and log2 == 2:
                out.append(False)
                continue
            v = bool(rng.integers(0, 3) > 0) and not cu["nores"]
            if v:
                units["cbf"][ys, xs, c] |= 1 << d
                n = size if c == 0 else size // 2
                put(c, x, y, n, levels(n))
            out.append(v)
        return tuple(out)

    def leaf(x, y, size, depth):
        ys, xs = slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4)
        u = units[ys, xs]
        u["depth"] = depth
        key = (x // qg, y // qg)
        if size >= qg or key not in qgqp:
            qgqp[key] = int(si["slice_qp"]) + int(rng.integers(-6, 7))
        u["qp"] = qgqp[key]
        u["tq_bypass"] = int(si["tq_bypass_enabled"] and rng.integers(0, 5) == 0)
        kind = 2 if slice_type == 2 else int(rng.choice([0, 1, 1, 2]))      # 0 skip, 1 inter, 2 intra
        log2 = int(np.log2(size))
        cu = dict(intra=kind == 2, part=0, nores=False)
        if kind == 0:
            u["pred_mode"], u["part_size"], u["merge_flag"] = MODE_SKIP, 0, 1
            u["mvp_idx"] = (int(rng.integers(0, si["max_num_merge_cand"])), 0)
            u["inter_dir"] = 1
            units[ys, xs] = u
            return
        if kind == 2:
            part = 3 if (size == 8 and rng.integers(0, 2)) else 0
            u["pred_mode"], u["part_size"] = MODE_INTRA, part
            units[ys, xs] = u
            if part == 3:
                for k in range(4):
                    units["luma_dir"][y // 4 + (k >> 1), x // 4 + (k & 1)] = int(rng.integers(0, 35))
            else:
                units["luma_dir"][ys, xs] = int(rng.integers(0, 35))
            first = int(units["luma_dir"][y // 4, x // 4])
            c = int(rng.choice([0, 26, 10, 1, 36]))
            if c != 36 and c == first:
                c = 34
            units["chroma_dir"][ys, xs] = c
            cu["part"] = part
            maxd, split = int(si["tu_max_depth_intra"]), int(part != 0)
        else:
            parts = [0, 0, 1, 2] + ([4, 5, 6, 7] if (depth < si["max_amp_depth"] and size >= 16) else [])
            part = int(rng.choice(parts))
            u["pred_mode"], u["part_size"] = MODE_INTER, part
            units[ys, xs] = u
            q = size // 4
            all_merge = True
            for (px, py, pw, ph) in _PU_RECTS[part]:
                pys, pxs = slice((y + py * q) // 4, (y + (py + ph) * q) // 4), slice((x + px * q) // 4, (x + (px + pw) * q) // 4)
                mf = int(rng.integers(0, 3) == 0)
                all_merge &= bool(mf)
                units["merge_flag"][pys, pxs] = mf
                if mf:
                    units["mvp_idx"][pys, pxs] = (int(rng.integers(0, si["max_num_merge_cand"])), 0)
                    units["inter_dir"][pys, pxs] = 1
                    continue
                if slice_type == 0:
                    idir = int(rng.integers(1, 3)) if (size == 8 and part != 0) else int(rng.integers(1, 4))
                else:
                    idir = 1
                units["inter_dir"][pys, pxs] = idir
                refs = [int(rng.integers(0, si["num_ref_idx"][l])) if idir & (1 << l) else -1 for l in range(2)]
                units["ref_idx"][pys, pxs] = refs
                units["mvp_idx"][pys, pxs] = (int(rng.integers(0, 2)), int(rng.integers(0, 2)))
                units["mvd"][pys, pxs] = [[int(rng.choice([0, 0, 1, -1, 2, -3, 17, -250, 4000])), int(rng.choice([0, 0, 1, -1, 5, -2, 33, 700]))] for _ in range(2)]
            cu["part"] = part
            cu["nores"] = bool(rng.integers(0, 4) == 0) and not (part == 0 and all_merge)     # root cbf 0 (a 2Nx2N merge without residual would be a skip)
            maxd, split = int(si["tu_max_depth_inter"]), int(si["tu_max_depth_inter"] == 1 and part != 0)
        lo = log2 - (maxd - 1 + split)
        cu["lo"] = min(max(lo, int(si["tu_log2_min"])), int(si["tu_log2_max"]))
        cy, cu_, cv_ = tu(x, y, log2, 0, cu)
        if kind == 1 and part == 0 and units["merge_flag"][y // 4, x // 4] and not (cy or cu_ or cv_):
            # merged 2Nx2N without a coded root flag implies residual: give the first TU a level
            d = int(units["tu_depth"][y // 4, x // 4])
            n = size >> d
            for dd in range(d + 1):
                units["cbf"][y // 4:(y + (size >> dd)) // 4, x // 4:(x + (size >> dd)) // 4, 0] |= 1 << dd
            put(0, x, y, n, levels(n))
        elif kind == 1 and not cu["nores"] and not (cy or cu_ or cv_):
            pass

    def walk(x, y, size, depth):
        if x >= width or y >= height:
            return
        inside = x + size <= width and y + size <= height
        if size > 8 and (not inside or rng.integers(0, 3) > 0):
            for k in range(4):
                walk(x + (k & 1) * size // 2, y + (k >> 1) * size // 2, size // 2, depth + 1)
            return
        leaf(x, y, size, depth)

    for cy in range(0, height, 64):
        for cx in range(0, width, 64):
            walk(cx, cy, 64, 0)
    return dict(si=si, units=np.ascontiguousarray(units), coeff=coeff, ctus=ctuW * ctuH)


def cabac_run_ref(R, c, bits_only=0):
    out = np.zeros(1 << 22, np.uint8); ctx = np.zeros(160, np.uint8); qp = np.zeros(c["units"].size, np.int8)
    si = np.array([c["si"]], SLICE_INFO_DT)
    R.lib.ref_encode_ctus.restype = C.c_size_t
    n = R.lib.ref_encode_ctus(_ptr(si), _ptr(c["units"]), _ptr(c["coeff"]), bits_only, _ptr(out), C.c_size_t(out.size), _ptr(ctx), _ptr(qp))
    return out[:n].copy(), ctx[:CTX_COUNT].copy(), qp


def cabac_run_product(L, c, bits_only=0):
    units = c["units"].copy()
    si = np.array([c["si"]], SLICE_INFO_DT)
    L.lib.x265amd_cabac_open.restype = C.c_void_p
    L.lib.x265amd_cabac_finish_slice.restype = C.c_size_t
    L.lib.x265amd_cabac_frac_bits.restype = C.c_uint64
    h = C.c_void_p(L.lib.x265amd_cabac_open(_ptr(si), _ptr(units), bits_only))
    assert h.value
    for a in range(c["ctus"]):
        row = c["coeff"][a]
        rc = L.lib.x265amd_cabac_encode_ctu(h, a, off(row, 0), off(row, 64 * 64), off(row, 64 * 64 + 32 * 32))
        assert rc == 0
    out = np.zeros(1 << 22, np.uint8); ctx = np.zeros(160, np.uint8)
    n = L.lib.x265amd_cabac_finish_slice(h, _ptr(out), C.c_size_t(out.size))
    L.lib.x265amd_cabac_get_contexts(h, _ptr(ctx))
    L.lib.x265amd_cabac_close(h)
    return out[:n].copy(), ctx[:CTX_COUNT].copy(), units["qp"].ravel().copy()


# ---- motion vector prediction (merge / AMVP candidates) ----
MV_UNIT_DT = np.dtype([("pred_mode", "u1"), ("inter_dir", "u1"), ("ref_idx", "i1", 2), ("mv", "<i2", (2, 2))])
MVPRED_INFO_DT = np.dtype([("pic_width", "<i4"), ("pic_height", "<i4"), ("is_inter_b", "<i4"), ("num_ref_idx", "<i4", 2), ("max_num_merge_cand", "<i4"),
                           ("temporal_mvp", "<i4"), ("col_from_l0", "<i4"), ("check_ldc", "<i4"), ("poc", "<i4"), ("ref_poc", "<i4", (2, 16)),
                           ("col_poc", "<i4"), ("col_ref_poc", "<i4", (2, 16))])
MERGE_CAND_DT = np.dtype([("mv", "<i2", (2, 2)), ("ref_idx", "i1", 2), ("dir", "u1"), ("reserved", "u1")])
assert MV_UNIT_DT.itemsize == 12 and MERGE_CAND_DT.itemsize == 12 and MVPRED_INFO_DT.itemsize == 4 * (10 + 32 + 1 + 32)


def mv_field(rng, width, height, is_b, nref, block=8):
    """random motion field, constant over block x block areas (with some 4-sample detail), about a quarter intra"""
    w4, h4 = width // 4, height // 4
    f = np.zeros((h4, w4), MV_UNIT_DT)
    for by in range(0, h4, block // 4):
        for bx in range(0, w4, block // 4):
            sl = f[by:by + block // 4, bx:bx + block // 4]
            k = int(rng.integers(0, 8))
            if k == 0:
                sl["pred_mode"], sl["ref_idx"] = MODE_INTRA, (-1, -1)
                continue
            sl["pred_mode"] = MODE_SKIP if k == 1 else MODE_INTER
            idir = int(rng.integers(1, 4)) if is_b else 1
            sl["inter_dir"] = idir
            base = (int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
            for l in range(2):
                if idir & (1 << l):
                    sl["ref_idx"][..., l] = int(rng.integers(0, nref[l]))
                    sl["mv"][..., l, 0] = base[0] * 4 + int(rng.integers(-1, 2)) * int(rng.integers(0, 2))
                    sl["mv"][..., l, 1] = base[1] * 4 + int(rng.integers(-1, 2)) * int(rng.integers(0, 2))
                else:
                    sl["ref_idx"][..., l] = -1
    return f


def mvpred_case(seed, width, height, is_b):
    rng = np.random.default_rng(seed)
    info = np.zeros(1, MVPRED_INFO_DT)[0]
    nref = (int(rng.integers(1, 5)), int(rng.integers(1, 4)) if is_b else 0)
    info["pic_width"], info["pic_height"], info["is_inter_b"], info["num_ref_idx"] = width, height, int(is_b), nref
    info["max_num_merge_cand"], info["temporal_mvp"] = int(rng.integers(1, 6)), int(rng.integers(0, 4) > 0)
    info["col_from_l0"], info["check_ldc"] = int(rng.integers(0, 2)), int(rng.integers(0, 2))
    poc = int(rng.integers(8, 40))
    info["poc"] = poc
    rp = np.zeros((2, 16), np.int32)
    rp[0, :] = poc - 1 - np.arange(16) * int(rng.integers(1, 3))
    rp[1, :] = (poc + 1 + np.arange(16)) if rng.integers(0, 2) else rp[0, :]          # forward references, or a low-delay style list
    info["ref_poc"] = rp
    info["col_poc"] = int(rp[0, 0])
    info["col_ref_poc"] = np.stack([rp[0, 0] - 1 - np.arange(16) * 2, rp[0, 0] + 2 + np.arange(16)])
    cur = mv_field(rng, width, height, is_b, nref)
    col = mv_field(rng, width, height, True, (4, 3), block=16)
    # the CUs / PUs to predict: random positions and shapes
    pus = []
    for _ in range(60):
        log2 = int(rng.integers(3, 7))
        size = 1 << log2
        if size > min(width, height):
            continue
        x, y = int(rng.integers(0, (width - size) // size + 1)) * size, int(rng.integers(0, (height - size) // size + 1)) * size
        part = int(rng.choice([0, 1, 2] + ([4, 5, 6, 7] if size >= 16 else [])))
        pus.append((x, y, log2, part, int(rng.integers(0, 1 if part == 0 else 2))))
    return dict(info=info, cur=np.ascontiguousarray(cur.ravel()), col=np.ascontiguousarray(col.ravel()), pus=pus)


def mvpred_run(L, c):
    """list per PU of (merge array, {(list, ref): (amvp 2x2, mvc k x 2)})"""
    info = np.array([c["info"]], MVPRED_INFO_DT)
    nref = c["info"]["num_ref_idx"]
    out = []
    for (x, y, log2, part, pu) in c["pus"]:
        merge = np.zeros(5, MERGE_CAND_DT)
        if L.prefix == "ref_":
            nm = C.c_int(0)
            amvp = np.zeros((2, 16, 2, 2), np.int16); mvc = np.zeros((2, 16, 12, 2), np.int16); nmvc = np.zeros((2, 16), np.int32)
            L.lib.ref_mv_pred(_ptr(info), _ptr(c["cur"]), _ptr(c["col"]), x, y, log2, part, pu, _ptr(merge), C.byref(nm), _ptr(amvp), _ptr(mvc), _ptr(nmvc))
            res = {(l, r): (amvp[l, r].copy(), mvc[l, r, :nmvc[l, r]].copy()) for l in range(2 if c["info"]["is_inter_b"] else 1) for r in range(int(nref[l]))}
            out.append((merge[:nm.value].copy(), res))
        else:
            nm = L.lib.x265amd_merge_candidates(_ptr(info), _ptr(c["cur"]), _ptr(c["col"]), x, y, log2, part, pu, _ptr(merge))
            res = {}
            for l in range(2 if c["info"]["is_inter_b"] else 1):
                for r in range(int(nref[l])):
                    a = np.zeros((2, 2), np.int16); m = np.zeros((12, 2), np.int16)
                    k = L.lib.x265amd_amvp_candidates(_ptr(info), _ptr(c["cur"]), _ptr(c["col"]), x, y, log2, part, pu, l, r, _ptr(a), _ptr(m))
                    res[(l, r)] = (a, m[:k].copy())
            out.append((merge[:nm].copy(), res))
    return out


# ---- predInterSearch: whole-CU inter search (AMVP, ME, merge, bi-prediction, choice, final MC) ----
SEARCH_PARAMS_DT = np.dtype([("searchMethod", "<i4"), ("subpelRefine", "<i4"), ("searchRange", "<i4"), ("qp", "<i4"), ("bChromaMC", "<i4"), ("numPics", "<i4"),
                             ("refPic", "<i4", (2, 16))])
PU_RESULT_DT = np.dtype([("merge_flag", "u1"), ("inter_dir", "u1"), ("ref_idx", "i1", 2), ("mvp_idx", "u1", 2), ("pad", "u1", 2), ("mv", "<i2", (2, 2)), ("mvd", "<i2", (2, 2))])
assert PU_RESULT_DT.itemsize == 24


def inter_scene(depth, seed, npics=4):
    """npics padded 4:2:0 pictures that are displaced, noisy views of one textured picture (last one = the source): returns
    (list of flat arrays Y|U|V, stride, cstride, origins) with the geometry of mc_make_refs"""
    rng = np.random.default_rng(seed)
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    stride, cstride = MC_W + 2 * MC_MX, MC_W // 2 + MC_MX
    big = rng.integers(0, pmax + 1, ((MC_H + 64) // 8 + 2, (MC_W + 64) // 8 + 2)).astype(np.int64)
    big = np.kron(big, np.ones((8, 8), np.int64))
    big = (big + np.roll(big, 3, 0) + np.roll(big, 5, 1) + np.roll(big, -2, 1)) // 4
    cb = (np.roll(big, 7, 0)[::2, ::2] + big[1::2, 1::2]) // 2
    cr = (np.roll(big, 11, 1)[::2, ::2] + big[::2, 1::2]) // 2
    pics = []
    for k in range(npics):
        dx, dy = (0, 0) if k == npics - 1 else (int(rng.integers(-6, 7)) * 2, int(rng.integers(-5, 6)) * 2)
        planes = []
        for (src, w, h, m_x, m_y, sx, sy) in ((big, MC_W, MC_H, MC_MX, MC_MY, dx, dy), (cb, MC_W // 2, MC_H // 2, MC_MX // 2, MC_MY // 2, dx // 2, dy // 2),
                                             (cr, MC_W // 2, MC_H // 2, MC_MX // 2, MC_MY // 2, dx // 2, dy // 2)):
            o = 16 if src is big else 8
            core = src[o + sy:o + sy + h, o + sx:o + sx + w] + rng.integers(-2, 3, (h, w)) * (1 << (depth - 8))
            core = np.clip(core, 0, pmax).astype(dt)
            planes.append(np.pad(core, ((m_y, m_y), (m_x, m_x)), mode="edge").ravel())
        pics.append(np.concatenate(planes))
    ysz, csz = (MC_H + 2 * MC_MY) * stride, (MC_H // 2 + MC_MY) * cstride
    org = (MC_MY * stride + MC_MX, ysz + (MC_MY // 2) * cstride + MC_MX // 2, ysz + csz + (MC_MY // 2) * cstride + MC_MX // 2)
    return pics, stride, cstride, org


def inter_search_case(depth, seed, is_b):
    rng = np.random.default_rng(seed)
    pics, stride, cstride, org = inter_scene(depth, seed)
    c = mvpred_case(seed, MC_W, MC_H, is_b)
    info = c["info"]
    sp = np.zeros(1, SEARCH_PARAMS_DT)[0]
    sp["searchMethod"], sp["subpelRefine"] = int(rng.choice([ME_HEX, ME_STAR, ME_DIA])), int(rng.choice([1, 2, 3]))
    sp["searchRange"], sp["qp"], sp["numPics"] = 57, int(rng.integers(22, 40)), len(pics)
    sp["bChromaMC"] = int(rng.integers(0, 2))
    rp = np.zeros((2, 16), np.int32)
    for l in range(2):
        for r in range(16):
            rp[l, r] = (r + l) % (len(pics) - 1)
    sp["refPic"] = rp
    cus = []
    for _ in range(14):
        log2 = int(rng.integers(3, 7))
        size = 1 << log2
        x, y = int(rng.integers(0, MC_W // size)) * size, int(rng.integers(0, MC_H // size)) * size
        part = int(rng.choice([0, 0, 1, 2] + ([4, 5, 6, 7] if size >= 16 else [])))
        cus.append((x, y, log2, part))
    return dict(pics=pics, stride=stride, cstride=cstride, org=org, info=info, sp=sp, cur=c["cur"], col=c["col"], cus=cus)


def inter_search_run_ref(R, c):
    isz = c["pics"][0].itemsize
    planes = np.array([p.ctypes.data + c["org"][k] * isz for p in c["pics"] for k in range(3)], np.uint64)
    info = np.array([c["info"]], MVPRED_INFO_DT); sp = np.array([c["sp"]], SEARCH_PARAMS_DT)
    out = []
    dt = c["pics"][0].dtype
    for (x, y, log2, part) in c["cus"]:
        res = np.zeros(2, PU_RESULT_DT)
        py, pu, pv = np.zeros((64, 64), dt), np.zeros((32, 32), dt), np.zeros((32, 32), dt)
        bits = R.lib.ref_pred_inter_search(_ptr(info), _ptr(sp), _ptr(c["cur"]), _ptr(c["col"]), _ptr(planes), C.c_int64(c["stride"]), C.c_int64(c["cstride"]),
                                           MC_MX, MC_MY, x, y, log2, part, _ptr(res), _ptr(py), _ptr(pu), _ptr(pv))
        n = 1 << log2
        out.append((int(bits), res[:(1 if part == 0 else 2)].copy(), py[:n, :n].copy(), pu[:n // 2, :n // 2].copy(), pv[:n // 2, :n // 2].copy()))
    return out


INTER_CU_DT = np.dtype([("x", "<i2"), ("y", "<i2"), ("log2", "u1"), ("part", "u1"), ("reserved", "u1", 2)])
WEIGHT_DT = np.dtype([("w", "<i2"), ("o", "<i2"), ("denom", "u1"), ("present", "u1")])          # x265amd_weight: WeightParam's inputWeight, inputOffset, log2WeightDenom, wtPresent
INTER_SP_DT = np.dtype([("search_method", "<i4"), ("subpel_refine", "<i4"), ("search_range", "<i4"), ("qp", "<i4"), ("chroma_mc", "<i4"), ("ref_pic", "<i4", (2, 16)), ("frame_parallel", "<i4"), ("lazy_sync", "<i4"),
                        ("lowres_blocks_in_row", "<i4"), ("me_pic", "<i4", (2, 16)), ("weighted", "<i4"), ("wp", WEIGHT_DT, (2, 16, 3)), ("pad_wp", "u1", 4), ("lowres_mvs", "<u8", (2, 16))])
assert INTER_SP_DT.itemsize == 1128 and INTER_SP_DT.fields["me_pic"][1] == 160 and INTER_SP_DT.fields["wp"][1] == 292 and INTER_SP_DT.fields["lowres_mvs"][1] == 872


def inter_search_run_hip(L, me, c):
    """x265amd_pred_inter_search on the whole CU list of the case; same return shape as inter_search_run_ref"""
    import torch
    isz = c["pics"][0].itemsize
    dt = c["pics"][0].dtype
    d_pics = [torch.from_numpy(p.view(np.uint8)).cuda() for p in c["pics"]]
    planes = np.array([d.data_ptr() + c["org"][k] * isz for d in d_pics for k in range(3)], np.uint64)
    info = np.array([c["info"]], MVPRED_INFO_DT)
    sp = np.zeros(1, INTER_SP_DT)
    for a, b in (("search_method", "searchMethod"), ("subpel_refine", "subpelRefine"), ("search_range", "searchRange"), ("qp", "qp"), ("chroma_mc", "bChromaMC")):
        sp[0][a] = c["sp"][b]
    sp[0]["ref_pic"] = c["sp"]["refPic"]
    n = len(c["cus"])
    cus = np.zeros(n, INTER_CU_DT)
    for i, (x, y, log2, part) in enumerate(c["cus"]):
        cus[i] = (x, y, log2, part, 0)
    out = np.zeros(2 * n, PU_RESULT_DT); bits = np.zeros(n, np.int32)
    per = (64 * 64 + 2 * 32 * 32) * isz
    d_pred = torch.zeros(n * per, dtype=torch.uint8, device="cuda")
    cur = c["cur"].copy()
    with call_stream(L) as st_:
        rc = L.lib.x265amd_pred_inter_search(me.ctx, st_, _ptr(info), _ptr(sp), _ptr(cur), _ptr(c["col"]), _ptr(planes), len(c["pics"]), C.c_int64(c["stride"]),
                                             C.c_int64(c["cstride"]), _ptr(cus), n, _ptr(out), _ptr(bits), C.c_uint64(d_pred.data_ptr()), C.c_size_t(per))
    assert rc == 0, L.lib.x265amd_last_error()
    assert np.array_equal(cur, c["cur"])            # the motion field is restored
    pred = d_pred.cpu().numpy().reshape(n, per)
    res = []
    for i, (x, y, log2, part) in enumerate(c["cus"]):
        s = 1 << log2
        py = pred[i, :64 * 64 * isz].view(dt).reshape(64, 64)[:s, :s].copy()
        pu = pred[i, 64 * 64 * isz:(64 * 64 + 32 * 32) * isz].view(dt).reshape(32, 32)[:s // 2, :s // 2].copy()
        pv = pred[i, (64 * 64 + 32 * 32) * isz:].view(dt).reshape(32, 32)[:s // 2, :s // 2].copy()
        if not c["sp"]["bChromaMC"]:
            pu[:] = 0; pv[:] = 0
        res.append((int(bits[i]), out[2 * i:2 * i + (1 if part == 0 else 2)].copy(), py, pu, pv))
    return res


# ---- residual RD of inter CUs (x265amd_inter_residual_rd vs Search::encodeResAndCalcRdInterCU) ----
RD_PARAMS_DT = np.dtype([("psy_rd", "<f8"), ("rd_level", "<i4"), ("strong", "<i4"), ("rdoq_level", "<i4"), ("psy_rdoq_scale", "<i4"), ("fast_intra", "<i4"), ("limit_tu", "<i4")])
RD_RESULT_DT = np.dtype([("rd_cost", "<u8"), ("distortion", "<u8"), ("frac_bits", "<u8"), ("total_bits", "<u4"), ("mv_bits", "<u4"), ("coeff_bits", "<u4"),
                         ("psy_energy", "<u4"), ("luma_distortion", "<u4"), ("chroma_distortion", "<u4"), ("res_energy", "<u4"), ("reserved", "<u4"),
                         ("ctx", "u1", 160)])
RD_CU_DT = np.dtype([("x", "<i2"), ("y", "<i2"), ("log2_size", "u1"), ("qp", "i1"), ("reserved", "u1", 2), ("frac_bits", "<u8"), ("ctx", "u1", 160)])
assert RD_RESULT_DT.itemsize == 216 and RD_CU_DT.itemsize == 176
RD_TILE = 64 * 64 + 2 * 32 * 32


def rd_case(depth, seed, slice_type, tu_inter_depth, psy_rd, ncu=10, width=128, height=128, strength=None):
    """a random coded neighbourhood (cabac_case), a textured source picture, and `ncu` candidate inter CUs each with its own prediction tile
    (the source block disturbed so that the residual has realistic structure), start contexts and QP"""
    rng = np.random.default_rng(seed + 77)
    base = cabac_case(seed, width, height, slice_type)
    si = base["si"].copy()
    si["tq_bypass_enabled"] = 0
    si["tu_max_depth_inter"] = tu_inter_depth
    units = base["units"].copy()
    units["tq_bypass"] = 0
    dt = np.uint8 if depth == 8 else np.uint16
    pmax = (1 << depth) - 1
    def plane(w, h, sd):
        r = np.random.default_rng(sd)
        b = r.integers(pmax // 8, pmax - pmax // 8, (h // 8 + 2, w // 8 + 2)).astype(np.int64)
        up = np.kron(b, np.ones((8, 8), np.int64))[:h, :w]
        sm = (up + np.roll(up, 2, 0) + np.roll(up, 3, 1) + np.roll(up, (5, 4), (0, 1)) + 2) >> 2
        return np.clip(sm + r.integers(-4, 5, sm.shape), 0, pmax)
    src = [plane(width, height, seed * 3 + 1), plane(width // 2, height // 2, seed * 3 + 2), plane(width // 2, height // 2, seed * 3 + 3)]
    cus = np.zeros(ncu, RD_CU_DT)
    preds = np.zeros((ncu, RD_TILE), dt)
    cu_units = np.zeros((ncu, 256), CU_UNIT_DT)
    maps = []
    ctx_pool = [entropy_reset_np(int(si["slice_type"]), q) for q in (22, 30, 37)]
    for i in range(ncu):
        log2 = int(rng.choice([3, 4, 4, 5, 5, 6]))
        size = 1 << log2
        x, y = int(rng.integers(0, width // size)) * size, int(rng.integers(0, height // size)) * size
        qp = int(rng.integers(18, 42))
        cus[i]["x"], cus[i]["y"], cus[i]["log2_size"], cus[i]["qp"] = x, y, log2, qp
        ctx = ctx_pool[int(rng.integers(0, 3))].copy()
        # disturb some context states so that the walk does not start from initial values
        idx = rng.choice(CTX_COUNT, size=40, replace=False)
        ctx[idx] = rng.integers(0, 126, size=40).astype(np.uint8)
        cus[i]["ctx"][:CTX_COUNT] = ctx[:CTX_COUNT]
        cus[i]["frac_bits"] = int(rng.integers(0, 32768))
        # the candidate's prediction fields
        depth_cu = 6 - log2
        parts = [0, 0, 0, 1, 2] + ([4, 5, 6, 7] if (depth_cu < si["max_amp_depth"] and size >= 16) else [])
        part = int(rng.choice(parts))
        m = units.copy()
        ys, xs = slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4)
        u = np.zeros((size // 4, size // 4), CU_UNIT_DT)
        u["depth"], u["pred_mode"], u["part_size"], u["qp"] = depth_cu, MODE_INTER, part, qp
        q = size // 4
        for (px, py, pw, ph) in _PU_RECTS[part]:
            pys, pxs = slice((py * q) // 4, ((py + ph) * q) // 4), slice((px * q) // 4, ((px + pw) * q) // 4)
            mf = int(rng.integers(0, 3) == 0)
            u["merge_flag"][pys, pxs] = mf
            if mf:
                u["mvp_idx"][pys, pxs] = (int(rng.integers(0, si["max_num_merge_cand"])), 0)
                u["inter_dir"][pys, pxs] = 1
                u["ref_idx"][pys, pxs] = (0, -1)
                continue
            idir = (int(rng.integers(1, 3)) if (size == 8 and part != 0) else int(rng.integers(1, 4))) if slice_type == 0 else 1
            u["inter_dir"][pys, pxs] = idir
            u["ref_idx"][pys, pxs] = [int(rng.integers(0, si["num_ref_idx"][l])) if idir & (1 << l) else -1 for l in range(2)]
            u["mvp_idx"][pys, pxs] = (int(rng.integers(0, 2)), int(rng.integers(0, 2)))
            u["mvd"][pys, pxs] = [[int(rng.choice([0, 0, 1, -1, 2, -3, 17])), int(rng.choice([0, 0, 1, -1, 5, -2, 33]))] for _ in range(2)]
        m[ys, xs] = u
        maps.append(m)
        cu_units[i, :u.size] = u.ravel()
        # prediction: the source block, smoothed and offset, with noise whose strength varies from "skip-like" to "busy"
        st = int(rng.choice([0, 1, 2, 4, 8, 16])) if strength is None else strength
        t = preds[i]
        for p in range(3):
            s = size if p == 0 else size // 2
            px, py = (x, y) if p == 0 else (x // 2, y // 2)
            blk = src[p][py:py + s, px:px + s]
            sm = (blk * 2 + np.roll(blk, 1, 0) + np.roll(blk, 1, 1) + 2) >> 2 if st else blk
            dist = sm + rng.integers(-st, st + 1, blk.shape) + (int(rng.integers(-3, 4)) if st else 0)
            if st and rng.integers(0, 2):       # a localised error so that TU splits pay off
                hy, hx = int(rng.integers(0, s)), int(rng.integers(0, s))
                dist[hy:hy + max(2, s // 4), hx:hx + max(2, s // 4)] += int(rng.integers(-40, 41)) << (depth - 8)
            tile = np.clip(dist, 0, pmax).astype(dt)
            o = 0 if p == 0 else 4096 + (p - 1) * 1024
            st_ = 64 if p == 0 else 32
            view = t[o:o + st_ * st_].reshape(st_, st_)
            view[:s, :s] = tile
    rp = np.zeros(1, RD_PARAMS_DT)
    rp["psy_rd"], rp["rd_level"] = psy_rd, 3
    return dict(si=si, units=units, maps=maps, src=[np.ascontiguousarray(p.astype(dt)) for p in src], cus=cus, preds=preds, cu_units=cu_units, rp=rp,
                width=width, height=height, depth=depth)


def entropy_reset_np(slice_type, qp):
    """context initialisation by rule (H.265 9.3.2.2) -- only used to seed plausible start states for tests"""
    from_lib = getattr(entropy_reset_np, "_lib", None)
    if from_lib is None:
        entropy_reset_np._lib = from_lib = load_oracle(8)
    return entropy_reset(from_lib, slice_type, qp)


def rd_run_ref(R, c):
    """Search::encodeResAndCalcRdInterCU per CU: returns (results, cu_units_out (n x 256), coeff (n x RD_TILE), recon (n x RD_TILE))"""
    n = len(c["cus"])
    dt = c["preds"].dtype
    res = np.zeros(n, RD_RESULT_DT); uo = np.zeros((n, 256), CU_UNIT_DT); coeff = np.zeros((n, RD_TILE), np.int16); recon = np.zeros((n, RD_TILE), dt)
    si = np.array([c["si"]], SLICE_INFO_DT)
    planes = np.array([p.ctypes.data for p in c["src"]], np.uint64)
    for i in range(n):
        cu = c["cus"][i]
        ctx = np.zeros(160, np.uint8); ctx[:] = cu["ctx"]
        m = np.ascontiguousarray(c["maps"][i])
        pr = c["preds"][i]
        R.lib.ref_inter_residual_rd(_ptr(si), _ptr(c["rp"]), _ptr(m), _ptr(planes), C.c_ssize_t(c["width"]), C.c_ssize_t(c["width"] // 2),
                                    int(cu["x"]), int(cu["y"]), int(cu["log2_size"]), int(cu["qp"]), _ptr(ctx), C.c_uint64(int(cu["frac_bits"])),
                                    off(pr, 0), off(pr, 4096), off(pr, 4096 + 1024), off(uo[i], 0), off(coeff[i], 0),
                                    off(recon[i], 0), off(recon[i], 4096), off(recon[i], 4096 + 1024), off(res, i))
    return res, uo, coeff, recon


CU_MEASURE_DT = np.dtype([("sse", "<u8", 3), ("psy", "<u4"), ("sa8d", "<u4"), ("sa8d_luma", "<u4"), ("src_mean", "<u4"), ("src_homo", "<u4"), ("reserved", "<u4")])
RD_SCRATCH_ELEMS = 4 * 4096 + 6 * 1024
RD_SEL_BYTES = 384


def cu_measure_expected(O, depth, src_planes, stride, cstride, cus, tiles):
    """the whole x265amd_cu_measure record per CU from the primitives of `O` (oracle, or the reference build) and numpy: src_planes = [Y, U, V] flat source
    planes with strides in samples, cus = RD_CU_DT records (x, y, log2_size), tiles[i] = CU i's RD_TILE (Y stride 64 | U | V stride 32).
      sse[p] = sse_pp; psy = psyCost_pp on luma; sa8d_luma = cu[log2 - 2].sa8d; sa8d = luma + cu[log2 - 3].sa8d of U and V (the 4x4 chroma of an 8x8 CU:
      cu[0].sa8d = satd_4x4, pixel.cpp:1171); src_mean = sum // S^2; src_homo = sum |v - mean| // S^2 (Analysis::complexityCheckCU, analysis.cpp:3538-3559)"""
    dt = np.uint8 if depth == 8 else np.uint16
    out = np.zeros(len(cus), CU_MEASURE_DT)
    for i, cu in enumerate(cus):
        log2 = int(cu["log2_size"]); S = 1 << log2
        for p in range(3):
            s, ts, st = (S, 64, stride) if p == 0 else (S // 2, 32, cstride)
            o = 0 if p == 0 else 4096 + (p - 1) * 1024
            x, y = (int(cu["x"]), int(cu["y"])) if p == 0 else (int(cu["x"]) // 2, int(cu["y"]) // 2)
            plane = np.asarray(src_planes[p]).reshape(-1, st)
            fenc = np.ascontiguousarray(plane[y:y + s, x:x + s].astype(dt))
            blk = np.ascontiguousarray(np.asarray(tiles[i])[o:o + ts * ts].reshape(ts, ts)[:s, :s].astype(dt))
            idx = log2 - 2 if p == 0 else log2 - 3
            out[i]["sse"][p] = O.call("sse_pp", idx, fenc, s, blk, s)
            sa = O.call("sa8d", idx, fenc, s, blk, s)
            out[i]["sa8d"] += sa
            if p == 0:
                out[i]["psy"] = O.call("psy_cost_pp", idx, fenc, s, blk, s)
                out[i]["sa8d_luma"] = sa
                v = fenc.astype(np.int64)
                mean = int(v.sum()) // (S * S)
                out[i]["src_mean"] = mean
                out[i]["src_homo"] = int(np.abs(v - mean).sum()) // (S * S)
    return out


MEASURE_KINDS = ("random", "both 0", "both pmax", "source pmax, tile 0", "checkerboard", "tile = source")
MEASURE_W = 128


def measure_case(depth, seed=1):
    """CU measurement cases: a 128x128 source picture whose 64x64 quadrants hold noise | 0 / pmax | a 0 / pmax checkerboard of pitch 1 (chroma alike), and 72 CUs
    -- every size 8..64 with every content of MEASURE_KINDS three times over, shuffled, at aligned positions of the quadrant that has their source -- each with
    an RD_TILE (Y stride 64, U and V stride 32) whose samples outside the block carry a pattern.  CU 0 is the 64x64 CU of the largest difference a block can
    have (source pmax against tile 0)."""
    rng = np.random.default_rng(seed * 977 + depth)
    dt = np.uint8 if depth == 8 else np.uint16
    pmax = (1 << depth) - 1
    W = MEASURE_W
    src = []
    for p in range(3):
        w = W if p == 0 else W // 2
        h = w // 2
        yy, xx = np.mgrid[0:w, 0:w]
        pl = rng.integers(0, pmax + 1, (w, w))
        pl[:h, h:] = 0                                  # top right: 0
        pl[h:, :h] = pmax                               # bottom left: pmax
        pl[h:, h:] = ((yy + xx) & 1)[h:, h:] * pmax     # bottom right: checkerboard
        src.append(np.ascontiguousarray(pl.astype(dt)))
    combos = [(log2, k) for k in range(len(MEASURE_KINDS)) for log2 in (3, 4, 5, 6)] * 3
    order = rng.permutation(len(combos))
    combos = [combos[i] for i in order]
    first = combos.index((6, 3))
    combos[0], combos[first] = combos[first], combos[0]
    n = len(combos)
    cus = np.zeros(n, RD_CU_DT)
    tiles = ((np.arange(n * RD_TILE, dtype=np.int64) * 7 + 3) % pmax + 1).astype(dt).reshape(n, RD_TILE)       # never 0: a sample read from outside the block shows
    quadrant = {0: (0, 0), 1: (64, 0), 2: (0, 64), 3: (0, 64), 4: (64, 64), 5: (0, 0)}
    for i, (log2, k) in enumerate(combos):
        S = 1 << log2
        qx, qy = quadrant[k]
        x, y = qx + int(rng.integers(0, 64 // S)) * S, qy + int(rng.integers(0, 64 // S)) * S
        cus[i]["x"], cus[i]["y"], cus[i]["log2_size"], cus[i]["qp"] = x, y, log2, 30
        for p in range(3):
            s, ts = (S, 64) if p == 0 else (S // 2, 32)
            px, py = (x, y) if p == 0 else (x // 2, y // 2)
            o = 0 if p == 0 else 4096 + (p - 1) * 1024
            view = tiles[i][o:o + ts * ts].reshape(ts, ts)
            blk = src[p][py:py + s, px:px + s]
            if k == 0:
                view[:s, :s] = rng.integers(0, pmax + 1, (s, s))
            elif k in (1, 3):
                view[:s, :s] = 0
            elif k == 2:
                view[:s, :s] = pmax
            elif k == 4:
                view[:s, :s] = pmax - blk       # the other colour of the board: +-pmax, alternating
            else:
                view[:s, :s] = blk
    return dict(depth=depth, src=src, cus=cus, tiles=tiles, kinds=[k for _, k in combos], stride=W, cstride=W // 2)


def cu_measure_run_hip(L, c, idx, stream=None, tile_list=False, seed=0):
    """x265amd_measure_tiles (tile_list: x265amd_measure_tile_list with the tiles at shuffled addresses) on the CUs `idx` of a measure_case; returns
    (records [n] CU_MEASURE_DT, tiles as they are afterwards [n, RD_TILE] in the order of idx, source planes as they are afterwards)"""
    import torch
    n = len(idx)
    dt = c["tiles"].dtype
    isz = dt.itemsize
    cus = np.ascontiguousarray(c["cus"][idx])
    place = np.random.default_rng(seed + n).permutation(n) if tile_list else np.arange(n)      # CU i's tile is the place[i]-th of the buffer
    buf = np.zeros((n, RD_TILE), dt)
    buf[place] = c["tiles"][idx]
    d_src = [torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1)).cuda() for p in c["src"]]
    planes = np.array([d.data_ptr() for d in d_src], np.uint64)
    d_tiles = torch.from_numpy(buf.view(np.uint8).reshape(-1)).cuda()
    addrs = np.array([d_tiles.data_ptr() + int(k) * RD_TILE * isz for k in place], np.uint64)
    out = np.zeros(n, CU_MEASURE_DT)
    out["reserved"] = 0xFFFFFFFF
    with stream_scope(stream) as st:
        if tile_list:
            rc = L.lib.x265amd_measure_tile_list(st, _ptr(planes), C.c_ssize_t(c["stride"]), C.c_ssize_t(c["cstride"]), _ptr(cus), n, _ptr(addrs), _ptr(out))
        else:
            rc = L.lib.x265amd_measure_tiles(st, _ptr(planes), C.c_ssize_t(c["stride"]), C.c_ssize_t(c["cstride"]), _ptr(cus), n, C.c_uint64(d_tiles.data_ptr()),
                                             C.c_size_t(RD_TILE * isz), _ptr(out))
    assert rc == 0, L.lib.x265amd_last_error()
    back = d_tiles.cpu().numpy().view(dt).reshape(n, RD_TILE)[place].copy()
    return out, back, [d.cpu().numpy().view(dt).reshape(p.shape) for d, p in zip(d_src, c["src"])]


def _rd_layer_offset(plane, layer):
    return 4 * 4096 + ((layer - 2) * 2 + plane - 1) * 1024 if plane else (layer - 2) * 4096


def rd_measure_cpu(O, c, scratch, sel, recon_out):
    """CPU stand-in of the product's k_cu_measure for the staged host test: assemble (sel is None: prediction only), reconstruct, measure
    with the oracle's sse_pp / psyCost_pp"""
    n = len(c["cus"])
    dt = c["preds"].dtype
    isz = dt.itemsize
    per = RD_SCRATCH_ELEMS * (4 + isz)
    pmax = (1 << c["depth"]) - 1
    out = np.zeros(n, CU_MEASURE_DT)
    O.lib.orc_sse_pp.restype = C.c_uint64
    for i in range(n):
        cu = c["cus"][i]
        log2 = int(cu["log2_size"]); S = 1 << log2
        resi = scratch[i * per + RD_SCRATCH_ELEMS * 2:i * per + RD_SCRATCH_ELEMS * 4].view(np.int16)
        for p in range(3):
            s = S if p == 0 else S // 2
            ts = 64 if p == 0 else 32
            o = 0 if p == 0 else 4096 + (p - 1) * 1024
            tile = c["preds"][i][o:o + ts * ts].reshape(ts, ts).astype(np.int64)
            if sel is not None:
                for uy in range(s // 4):
                    for ux in range(s // 4):
                        layer = int(sel[i * RD_SEL_BYTES + (uy * 16 + ux if p == 0 else 256 + (p - 1) * 64 + uy * 8 + ux)])
                        if layer != 0xFF:
                            r = resi[_rd_layer_offset(p, layer):_rd_layer_offset(p, layer) + ts * ts].reshape(ts, ts)
                            tile[uy * 4:uy * 4 + 4, ux * 4:ux * 4 + 4] = np.clip(tile[uy * 4:uy * 4 + 4, ux * 4:ux * 4 + 4] + r[uy * 4:uy * 4 + 4, ux * 4:ux * 4 + 4], 0, pmax)
            rec = np.ascontiguousarray(tile.astype(dt))
            recon_out[i][o:o + ts * ts] = rec.ravel()
            src = c["src"][p]
            x, y = (int(cu["x"]), int(cu["y"])) if p == 0 else (int(cu["x"]) // 2, int(cu["y"]) // 2)
            fenc = np.ascontiguousarray(src[y:y + s, x:x + s])
            blk = np.ascontiguousarray(rec[:s, :s])
            cuidx = int(np.log2(s)) - 2
            out[i]["sse"][p] = O.lib.orc_sse_pp(cuidx, _ptr(fenc), C.c_int64(s), _ptr(blk), C.c_int64(s))
            if p == 0:
                out[i]["psy"] = O.lib.orc_psy_cost_pp(cuidx, _ptr(fenc), C.c_int64(s), _ptr(blk), C.c_int64(s))
    return out


def rd_run_stages_cpu(L, O, c):
    """the product's host stages (plan / walk / finish) with the oracle executing the transform-chain jobs and the CU measurements:
    checks the host logic without a GPU"""
    n = len(c["cus"])
    dt = c["preds"].dtype
    isz = dt.itemsize
    lib = L.lib
    lib.x265amd_inter_rd_scratch_bytes.restype = C.c_size_t
    per = lib.x265amd_inter_rd_scratch_bytes()
    assert per == RD_SCRATCH_ELEMS * (4 + isz)
    scratch = np.zeros(n * per, np.uint8)
    si = np.array([c["si"]], SLICE_INFO_DT)
    planes = np.array([p.ctypes.data for p in c["src"]], np.uint64)
    cu_units = c["cu_units"].copy()
    preds = np.ascontiguousarray(c["preds"])
    args = (_ptr(si), _ptr(c["cus"]), n, _ptr(cu_units), _ptr(planes), C.c_ssize_t(c["width"]), C.c_ssize_t(c["width"] // 2),
            C.c_uint64(preds.ctypes.data), C.c_size_t(RD_TILE * isz), C.c_uint64(scratch.ctypes.data))
    nj = lib.x265amd_inter_rd_plan(*args, None, 0)
    assert nj > 0
    jobs = np.zeros(nj, TU_JOB_DT)
    assert lib.x265amd_inter_rd_plan(*args, _ptr(jobs), nj) == nj
    res = np.zeros(nj, TU_RESULT_DT)
    assert O.lib.orc_tu_chain_batch(_ptr(jobs), nj, _ptr(res)) == nj
    dump = np.zeros((n, RD_TILE), dt)
    m0 = rd_measure_cpu(O, c, scratch, None, dump)
    sel = np.zeros(n * RD_SEL_BYTES, np.uint8)
    out = np.zeros(n, RD_RESULT_DT)
    coeff = np.zeros((n, RD_TILE), np.int16)
    units = np.ascontiguousarray(c["units"].copy())
    # every candidate has its own neighbourhood map in the test case: one CU per walk call
    for i in range(n):
        m = np.ascontiguousarray(c["maps"][i].copy())
        before = m.copy()
        # the walk indexes results globally, so hand it the whole arrays with CU i as a batch of its own would shift indices: run all, map per CU
        rc = lib.x265amd_inter_rd_walk(_ptr(si), _ptr(c["rp"]), _ptr(m), off(c["cus"], i), 1, off(cu_units, i * 256),
                                       off(res, _rd_first_job(lib, args, c, i)), C.c_void_p(scratch.ctypes.data + i * per), C.c_size_t(per),
                                       off(m0, i), off(sel, i * RD_SEL_BYTES), off(out, i), off(coeff[i], 0))
        assert rc == 0
        assert (m == before).all(), "the picture map must be restored"
    recon = np.zeros((n, RD_TILE), dt)
    m1 = rd_measure_cpu(O, c, scratch, sel, recon)
    lib.x265amd_inter_rd_finish(_ptr(si), _ptr(c["rp"]), _ptr(c["cus"]), n, _ptr(m1), _ptr(out))
    return out, cu_units, coeff, recon


def _rd_first_job(lib, args, c, i):
    """index of CU i's first job = number of jobs of the CUs before it"""
    if i == 0:
        return 0
    a = list(args)
    a[2] = i
    return lib.x265amd_inter_rd_plan(*a, None, 0)


def rd_compare(got, want, c, what):
    """(results, cu_units, coeff, recon) of the product vs the reference driver"""
    gr, gu, gc, grec = got
    wr, wu, wc, wrec = want
    for i in range(len(wr)):
        cu = c["cus"][i]
        n4 = (1 << int(cu["log2_size"])) // 4
        tag = "%s CU %d (log2 %d qp %d)" % (what, i, cu["log2_size"], cu["qp"])
        for f in ("total_bits", "mv_bits", "coeff_bits", "luma_distortion", "chroma_distortion", "distortion", "psy_energy", "res_energy", "rd_cost", "frac_bits"):
            assert int(gr[i][f]) == int(wr[i][f]), "%s: %s %d != %d" % (tag, f, gr[i][f], wr[i][f])
        assert (gr[i]["ctx"][:CTX_COUNT] == wr[i]["ctx"][:CTX_COUNT]).all(), tag + ": contexts"
        for f in ("tu_depth", "cbf", "pred_mode", "qp"):
            assert (gu[i][f][:n4 * n4] == wu[i][f][:n4 * n4]).all(), "%s: unit field %s" % (tag, f)
        S = 1 << int(cu["log2_size"])
        for p in range(3):
            s = S if p == 0 else S // 2
            ts = 64 if p == 0 else 32
            o = 0 if p == 0 else 4096 + (p - 1) * 1024
            assert (grec[i][o:o + ts * ts].reshape(ts, ts)[:s, :s] == wrec[i][o:o + ts * ts].reshape(ts, ts)[:s, :s]).all(), "%s: recon plane %d" % (tag, p)
        if wu[i]["cbf"][:n4 * n4].any():
            assert (gc[i][:S * S] == wc[i][:S * S]).all(), tag + ": luma levels"
            assert (gc[i][4096:4096 + S * S // 4] == wc[i][4096:4096 + S * S // 4]).all(), tag + ": U levels"
            assert (gc[i][5120:5120 + S * S // 4] == wc[i][5120:5120 + S * S // 4]).all(), tag + ": V levels"


def rd_run_hip(L, c, stream=None):
    """x265amd_inter_residual_rd on the whole candidate list (one call); same return shape as rd_run_ref"""
    import torch
    n = len(c["cus"])
    dt = c["preds"].dtype
    isz = dt.itemsize
    d_src = [torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1)).cuda() for p in c["src"]]
    planes = np.array([d.data_ptr() for d in d_src], np.uint64)
    d_pred = torch.from_numpy(np.ascontiguousarray(c["preds"]).view(np.uint8).reshape(-1)).cuda()
    d_recon = torch.zeros(n * RD_TILE * isz, dtype=torch.uint8, device="cuda")
    si = np.array([c["si"]], SLICE_INFO_DT)
    units = np.ascontiguousarray(c["units"].copy())
    cu_units = c["cu_units"].copy()
    out = np.zeros(n, RD_RESULT_DT)
    coeff = np.zeros((n, RD_TILE), np.int16)
    with (stream_scope(stream) if stream is not None else call_stream(L)) as st_:
        rc = L.lib.x265amd_inter_residual_rd(st_, _ptr(si), _ptr(c["rp"]), _ptr(units), _ptr(planes), C.c_ssize_t(c["width"]), C.c_ssize_t(c["width"] // 2),
                                             _ptr(c["cus"]), n, _ptr(cu_units), C.c_uint64(d_pred.data_ptr()), C.c_uint64(d_recon.data_ptr()),
                                             C.c_size_t(RD_TILE * isz), _ptr(out), _ptr(coeff))
    assert rc == 0, L.lib.x265amd_last_error()
    assert np.array_equal(units, c["units"])           # the picture map is restored
    recon = d_recon.cpu().numpy().view(dt).reshape(n, RD_TILE).copy()
    return out, cu_units, coeff, recon


def rd_pack(res, c):
    """golden form of (results, cu_units, coeff, recon): the compared fields only"""
    r, u, co, rec = res
    keep = []
    for i in range(len(r)):
        cu = c["cus"][i]
        S = 1 << int(cu["log2_size"]); n4 = S // 4
        d = dict(res=np.array([int(r[i][f]) for f in ("total_bits", "mv_bits", "coeff_bits", "luma_distortion", "chroma_distortion", "distortion", "psy_energy",
                                                        "res_energy", "rd_cost", "frac_bits")], np.uint64),
                 ctx=r[i]["ctx"][:CTX_COUNT].copy(),
                 # columns: tu_depth, cbf Y/U/V, pred_mode, qp
                 units=np.concatenate([u[i][f][:n4 * n4].astype(np.int16).reshape(n4 * n4, -1) for f in ("tu_depth", "cbf", "pred_mode", "qp")], 1))
        planes = []
        for p in range(3):
            s = S if p == 0 else S // 2
            ts = 64 if p == 0 else 32
            o = 0 if p == 0 else 4096 + (p - 1) * 1024
            planes.append(rec[i][o:o + ts * ts].reshape(ts, ts)[:s, :s].astype(np.uint16).ravel())
        d["recon"] = np.concatenate(planes)
        if u[i]["cbf"][:n4 * n4].any():
            d["coeff"] = np.concatenate([co[i][:S * S], co[i][4096:4096 + S * S // 4], co[i][5120:5120 + S * S // 4]])
        else:
            d["coeff"] = np.zeros(0, np.int16)
        keep.append(d)
    return keep


def skip_case(depth, seed, slice_type, psy_rd, ncu=10):
    """rd_case with every candidate a merged 2Nx2N CU (the only kind encodeResAndCalcRdSkipCU sees)"""
    c = rd_case(depth, seed, slice_type, 1, psy_rd, ncu=ncu)
    rng = np.random.default_rng(seed + 5)
    for i in range(len(c["cus"])):
        cu = c["cus"][i]
        n4 = (1 << int(cu["log2_size"])) // 4
        u = c["cu_units"][i]
        u["part_size"][:n4 * n4] = 0
        u["merge_flag"][:n4 * n4] = 1
        u["mvp_idx"][:n4 * n4] = (int(rng.integers(0, c["si"]["max_num_merge_cand"])), 0)
        u["inter_dir"][:n4 * n4] = 1
        u["ref_idx"][:n4 * n4] = (0, -1)
        u["mvd"][:n4 * n4] = 0
        x, y = int(cu["x"]), int(cu["y"])
        c["maps"][i][y // 4:y // 4 + n4, x // 4:x // 4 + n4] = u[:n4 * n4].reshape(n4, n4)
    return c


def skip_run_ref(R, c):
    n = len(c["cus"])
    dt = c["preds"].dtype
    res = np.zeros(n, RD_RESULT_DT); uo = np.zeros((n, 256), CU_UNIT_DT); coeff = np.zeros((n, RD_TILE), np.int16); recon = np.zeros((n, RD_TILE), dt)
    si = np.array([c["si"]], SLICE_INFO_DT)
    planes = np.array([p.ctypes.data for p in c["src"]], np.uint64)
    for i in range(n):
        cu = c["cus"][i]
        ctx = np.zeros(160, np.uint8); ctx[:] = cu["ctx"]
        m = np.ascontiguousarray(c["maps"][i])
        pr = c["preds"][i]
        R.lib.ref_skip_rd(_ptr(si), _ptr(c["rp"]), _ptr(m), _ptr(planes), C.c_ssize_t(c["width"]), C.c_ssize_t(c["width"] // 2),
                          int(cu["x"]), int(cu["y"]), int(cu["log2_size"]), int(cu["qp"]), _ptr(ctx), C.c_uint64(int(cu["frac_bits"])),
                          off(pr, 0), off(pr, 4096), off(pr, 4096 + 1024), off(uo[i], 0), off(coeff[i], 0),
                          off(recon[i], 0), off(recon[i], 4096), off(recon[i], 4096 + 1024), off(res, i))
    return res, uo, coeff, recon


def skip_run_host_cpu(L, O, c):
    n = len(c["cus"])
    dt = c["preds"].dtype
    recon = np.zeros((n, RD_TILE), dt)
    m = rd_measure_cpu(O, c, np.zeros(n * RD_SCRATCH_ELEMS * (4 + dt.itemsize), np.uint8), None, recon)
    si = np.array([c["si"]], SLICE_INFO_DT)
    units = np.ascontiguousarray(c["units"].copy())
    cu_units = c["cu_units"].copy()
    out = np.zeros(n, RD_RESULT_DT)
    rc = L.lib.x265amd_skip_rd_host(_ptr(si), _ptr(c["rp"]), _ptr(units), _ptr(c["cus"]), n, _ptr(cu_units), _ptr(m), _ptr(out))
    assert rc == 0
    assert np.array_equal(units, c["units"])
    return out, cu_units, np.zeros((n, RD_TILE), np.int16), recon


def skip_run_hip(L, c):
    import torch
    n = len(c["cus"])
    dt = c["preds"].dtype
    isz = dt.itemsize
    d_src = [torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1)).cuda() for p in c["src"]]
    planes = np.array([d.data_ptr() for d in d_src], np.uint64)
    d_pred = torch.from_numpy(np.ascontiguousarray(c["preds"]).view(np.uint8).reshape(-1)).cuda()
    d_recon = torch.zeros(n * RD_TILE * isz, dtype=torch.uint8, device="cuda")
    si = np.array([c["si"]], SLICE_INFO_DT)
    units = np.ascontiguousarray(c["units"].copy())
    cu_units = c["cu_units"].copy()
    out = np.zeros(n, RD_RESULT_DT)
    with call_stream(L) as st_:
        rc = L.lib.x265amd_skip_rd(st_, _ptr(si), _ptr(c["rp"]), _ptr(units), _ptr(planes), C.c_ssize_t(c["width"]), C.c_ssize_t(c["width"] // 2),
                                   _ptr(c["cus"]), n, _ptr(cu_units), C.c_uint64(d_pred.data_ptr()), C.c_uint64(d_recon.data_ptr()), C.c_size_t(RD_TILE * isz), _ptr(out))
    assert rc == 0, L.lib.x265amd_last_error()
    assert np.array_equal(units, c["units"])
    recon = d_recon.cpu().numpy().view(dt).reshape(n, RD_TILE).copy()
    return out, cu_units, np.zeros((n, RD_TILE), np.int16), recon


# ---- CTU analysis of inter slices (x265amd_compress_ctu_inter vs Analysis::compressCTU) ----
ANALYSIS_PARAMS_DT = np.dtype([("psy_rd", "<f8"), ("rd_level", "<i4"), ("early_skip", "<i4"), ("rskip", "<i4"), ("limit_refs", "<i4"), ("b_intra", "<i4"),
                               ("rect", "<i4"), ("amp", "<i4"), ("limit_modes", "<i4"), ("strong", "<i4"), ("use_sao", "<i4"), ("rdoq_level", "<i4"), ("psy_rdoq_scale", "<i4"), ("fast_intra", "<i4"), ("reserved", "<i4")])
CU_STAT_DT = np.dtype([("count", "<u4", 4), ("pad", "<u4", 2), ("avg_cost", "<u8", 4)])
CTU_RESULT_DT = np.dtype([("rd_cost", "<u8"), ("distortion", "<u8"), ("frac_bits", "<u8"), ("total_bits", "<u4"), ("reserved", "<u4"), ("ctx", "u1", 160)])
assert CU_STAT_DT.itemsize == 56 and CTU_RESULT_DT.itemsize == 192 and ANALYSIS_PARAMS_DT.itemsize == 64


def ctu_case(depth, seed, is_b=True, early_skip=1, rskip=1, psy_rd=2.0, tu_inter_depth=1, nctu=3, detail=1.0, limit_refs=0, b_intra=0, strong=1, intra_slice=False,
             rect=0, amp=0, limit_modes=0, rd_level=3, rdoq_level=0, psy_rdoq_scale=0, fast_intra=0):
    """a picture in the middle of being coded: reference pictures + source (inter_scene, plus one picture that receives the reconstruction),
    the unit map and motion field of the CTUs coded so far, the reference pictures' depth maps, running cost statistics, and the CTUs to analyse"""
    rng = np.random.default_rng(seed + 901)
    pics, stride, cstride, org = inter_scene(depth, seed, npics=4)
    recon = np.zeros_like(pics[0])
    width, height = MC_W, MC_H
    # local detail in the source so that small CUs pay off: blocks moved differently from their surroundings, and blocks of plain noise
    src = pics[3].copy()
    pmax = (1 << depth) - 1
    ysz = (MC_H + 2 * MC_MY) * stride
    csz = (MC_H // 2 + MC_MY) * cstride
    views = [(src[:ysz].reshape(-1, stride), pics[0][:ysz].reshape(-1, stride), MC_MX, MC_MY, 1),
             (src[ysz:ysz + csz].reshape(-1, cstride), pics[0][ysz:ysz + csz].reshape(-1, cstride), MC_MX // 2, MC_MY // 2, 2),
             (src[ysz + csz:].reshape(-1, cstride), pics[0][ysz + csz:].reshape(-1, cstride), MC_MX // 2, MC_MY // 2, 2)]
    for _ in range(int(detail * 30)):
        bs = int(rng.choice([8, 8, 16, 16, 32]))
        bx, by = int(rng.integers(0, width // bs)) * bs, int(rng.integers(0, height // bs)) * bs
        kind = int(rng.integers(0, 3))
        dx, dy = int(rng.integers(-8, 9)) * 2, int(rng.integers(-6, 7)) * 2
        for (sv, rv, mx_, my_, sub) in views:
            b, x0, y0 = bs // sub, bx // sub + mx_, by // sub + my_
            if kind == 0:
                sv[y0:y0 + b, x0:x0 + b] = rng.integers(pmax // 4, 3 * pmax // 4, (b, b))
            else:
                sv[y0:y0 + b, x0:x0 + b] = rv[y0 + dy // sub:y0 + dy // sub + b, x0 + dx // sub:x0 + dx // sub + b]
    if rect or amp:
        # CUs whose two halves / quarter + three quarters move differently, so that two-part prediction pays off
        rng2 = np.random.default_rng(seed + 977)
        for _ in range(60):
            bs = int(rng2.choice([16, 16, 32, 32, 64] if amp else [8, 16, 16, 32, 64]))
            bx, by = int(rng2.integers(0, width // bs)) * bs, int(rng2.integers(0, height // bs)) * bs
            shape = int(rng2.choice(([1, 2] if rect else []) + ([4, 5, 6, 7] if amp else [])))
            cut = {1: bs // 2, 2: bs // 2, 4: bs // 4, 5: 3 * bs // 4, 6: bs // 4, 7: 3 * bs // 4}[shape]
            horiz = shape in (1, 4, 5)
            for k in range(2):
                dx, dy = int(rng2.integers(-6, 7)) * 2, int(rng2.integers(-5, 6)) * 2
                px, py = (bx, by + (cut if k else 0)) if horiz else (bx + (cut if k else 0), by)
                pw, ph = (bs, (bs - cut) if k else cut) if horiz else ((bs - cut) if k else cut, bs)
                for (sv, rv, mx_, my_, sub) in views:
                    x0, y0, w_, h_ = px // sub + mx_, py // sub + my_, pw // sub, ph // sub
                    sv[y0:y0 + h_, x0:x0 + w_] = rv[y0 + dy // sub:y0 + dy // sub + h_, x0 + dx // sub:x0 + dx // sub + w_]
    recon[:] = np.clip(src.astype(np.int64) + rng.integers(-3, 4, src.shape), 0, pmax).astype(src.dtype)      # what earlier CTUs left (intra neighbours)
    pics = pics[:3] + [recon, src]                  # refs 0..2, reconstruction, source
    w4, h4, ctuW, ctuH = width // 4, height // 4, width // 64, height // 64
    mp = mvpred_case(seed, width, height, is_b)
    info = mp["info"].copy()
    info["max_num_merge_cand"] = int(rng.integers(2, 6))
    nref = info["num_ref_idx"]
    base = cabac_case(seed, width, height, 2 if intra_slice else (0 if is_b else 1))
    si = base["si"].copy()
    si["slice_type"] = 2 if intra_slice else (0 if is_b else 1)
    si["tq_bypass_enabled"], si["use_dqp"], si["max_cu_dqp_depth"] = 0, 0, 0
    si["tu_max_depth_inter"], si["max_num_merge_cand"], si["num_ref_idx"] = tu_inter_depth, info["max_num_merge_cand"], nref
    si["slice_qp"] = int(rng.integers(24, 38))
    si["max_amp_depth"] = 3 if amp else 0          # sps.maxAMPDepth = bEnableAMP ? maxCUDepth : 0
    units = base["units"].copy()
    units["tq_bypass"] = 0
    units["qp"] = si["slice_qp"]
    # a motion field that agrees with the unit map's prediction modes
    cur = np.zeros((h4, w4), MV_UNIT_DT)
    cur["ref_idx"] = -1
    for by in range(0, h4, 2):
        for bx in range(0, w4, 2):
            pm = int(units["pred_mode"][by, bx])
            sl = cur[by:by + 2, bx:bx + 2]
            sl["pred_mode"] = units["pred_mode"][by:by + 2, bx:bx + 2]
            if pm in (MODE_INTER, MODE_SKIP):
                idir = int(rng.integers(1, 4)) if is_b else 1
                sl["inter_dir"] = idir
                for l in range(2):
                    if idir & (1 << l):
                        sl["ref_idx"][..., l] = int(rng.integers(0, nref[l]))
                        sl["mv"][..., l, 0] = int(rng.integers(-10, 11)) * 2
                        sl["mv"][..., l, 1] = int(rng.integers(-8, 9)) * 2
                units["inter_dir"][by:by + 2, bx:bx + 2] = idir
                units["ref_idx"][by:by + 2, bx:bx + 2] = sl["ref_idx"]
    sp = np.zeros(1, SEARCH_PARAMS_DT)[0]
    sp["searchMethod"], sp["subpelRefine"] = int(rng.choice([ME_HEX, ME_STAR])), int(rng.choice([1, 2, 3]))
    sp["searchRange"], sp["qp"], sp["numPics"] = 57, int(si["slice_qp"]), len(pics)
    sp["bChromaMC"] = 1
    rp = np.zeros((2, 16), np.int32)
    for l in range(2):
        for r in range(16):
            rp[l, r] = (r + l) % 3
    sp["refPic"] = rp
    ap = np.zeros(1, ANALYSIS_PARAMS_DT)
    ap["psy_rd"], ap["rd_level"], ap["early_skip"], ap["rskip"], ap["limit_refs"], ap["b_intra"], ap["strong"] = psy_rd, 3, early_skip, rskip, limit_refs, b_intra, strong
    ap["rect"], ap["amp"], ap["limit_modes"] = rect, amp, limit_modes
    ap["rd_level"] = rd_level
    ap["rdoq_level"], ap["psy_rdoq_scale"], ap["fast_intra"] = rdoq_level, psy_rdoq_scale, fast_intra
    # reference pictures' CU depths (two lists) and CTU QPs; running cost statistics of the CTUs coded so far
    ref_depth = np.zeros((2, h4, w4), np.uint8)
    for l in range(2):
        for by in range(0, h4, 4):
            for bx in range(0, w4, 4):
                ref_depth[l, by:by + 4, bx:bx + 4] = int(rng.integers(0, 4))
        for cy in range(ctuH):                       # some CTUs entirely at depth 0 / 1
            for cx in range(ctuW):
                if rng.integers(0, 4) == 0:
                    ref_depth[l, cy * 16:cy * 16 + 16, cx * 16:cx * 16 + 16] = int(rng.integers(0, 2))
    ref_qp0 = rng.integers(int(si["slice_qp"]) - 4, int(si["slice_qp"]) + 5, (2, ctuW * ctuH)).astype(np.int8)
    stat = np.zeros(ctuW * ctuH + 1, CU_STAT_DT)
    ctus = sorted(int(a) for a in rng.choice(np.arange(1, ctuW * ctuH), size=nctu, replace=False))
    maps = []
    ctx_pool = [entropy_reset_np(int(si["slice_type"]), q) for q in (26, 32)]
    starts = []
    for a in ctus:
        u = units.copy(); m = cur.copy()
        for addr in range(a, ctuW * ctuH):
            cx, cy = (addr % ctuW) * 16, (addr // ctuW) * 16
            u["pred_mode"][cy:cy + 16, cx:cx + 16] = MODE_NONE
            m["pred_mode"][cy:cy + 16, cx:cx + 16] = MODE_NONE
            m["ref_idx"][cy:cy + 16, cx:cx + 16] = -1
        st = stat.copy()
        for addr in range(a):
            st[addr]["count"] = rng.integers(0, 6, 4)
            st[addr]["avg_cost"] = rng.integers(2000, 60000, 4) * (st[addr]["count"] > 0)
        ctx = ctx_pool[int(rng.integers(0, 2))].copy()
        idx = rng.choice(CTX_COUNT, size=30, replace=False)
        ctx[idx] = rng.integers(0, 126, size=30).astype(np.uint8)
        maps.append((np.ascontiguousarray(u), np.ascontiguousarray(m), st))
        starts.append((ctx, int(rng.integers(0, 32768))))
    return dict(pics=pics, stride=stride, cstride=cstride, org=org, info=info, sp=sp, si=si, ap=ap, col=mp["col"], ref_depth=ref_depth, ref_qp0=ref_qp0,
                ctus=ctus, maps=maps, starts=starts, width=width, height=height, depth=depth)


def ctu_run_ref(R, c):
    """Analysis::compressCTU for each listed CTU (independently, each on its own 'coded so far' state):
    list of (result, units 16x16, motion 16x16, coeff, recon planes of the CTU, stats)"""
    isz = c["pics"][0].itemsize
    info = np.array([c["info"]], MVPRED_INFO_DT); sp = np.array([c["sp"]], SEARCH_PARAMS_DT); si = np.array([c["si"]], SLICE_INFO_DT)
    out = []
    for k, a in enumerate(c["ctus"]):
        pics = [p.copy() for p in c["pics"]]
        planes = np.array([p.ctypes.data + c["org"][j] * isz for p in pics for j in range(3)], np.uint64)
        u, m, st = c["maps"][k]
        st = st.copy()
        ctx = np.zeros(160, np.uint8); ctx[:len(c["starts"][k][0])] = c["starts"][k][0]
        uo = np.zeros((16, 16), CU_UNIT_DT); mo = np.zeros((16, 16), MV_UNIT_DT); coeff = np.zeros(RD_TILE, np.int16); res = np.zeros(1, CTU_RESULT_DT)
        R.lib.ref_compress_ctu(_ptr(info), _ptr(sp), _ptr(si), _ptr(c["ap"]), _ptr(u), _ptr(m), _ptr(c["col"]), _ptr(c["ref_depth"]), _ptr(c["ref_qp0"]),
                               _ptr(planes), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), MC_MX, MC_MY, _ptr(st), a, _ptr(ctx),
                               C.c_uint64(c["starts"][k][1]), _ptr(uo), _ptr(mo), _ptr(coeff), _ptr(res))
        out.append((res[0].copy(), uo, mo, coeff, ctu_recon(c, pics[-2], a), st))
    return out


def ctu_recon(c, recon_pic, addr):
    """the three planes of CTU addr cut out of a flat padded picture"""
    ctuW = c["width"] // 64
    x, y = (addr % ctuW) * 64, (addr // ctuW) * 64
    out = []
    for p in range(3):
        st = c["stride"] if p == 0 else c["cstride"]
        s = 64 if p == 0 else 32
        px, py = (x, y) if p == 0 else (x // 2, y // 2)
        o = c["org"][p] + py * st + px
        out.append(np.stack([recon_pic[o + r * st:o + r * st + s] for r in range(s)]))
    return out


def ctu_run_hip(L, me, c, ex=False):
    """x265amd_compress_ctu_inter (ex: x265amd_compress_ctu_inter_ex with edge = NULL) for each listed CTU, each on its own 'coded so far' state; same return shape as
    ctu_run_ref"""
    import torch
    isz = c["pics"][0].itemsize
    info = np.array([c["info"]], MVPRED_INFO_DT); si = np.array([c["si"]], SLICE_INFO_DT)
    sp = np.zeros(1, INTER_SP_DT)
    for a, b in (("search_method", "searchMethod"), ("subpel_refine", "subpelRefine"), ("search_range", "searchRange"), ("qp", "qp"), ("chroma_mc", "bChromaMC")):
        sp[0][a] = c["sp"][b]
    sp[0]["ref_pic"] = c["sp"]["refPic"]
    out = []
    w4 = c["width"] // 4
    ctuW = c["width"] // 64
    for k, a in enumerate(c["ctus"]):
        d_pics = [torch.from_numpy(p.view(np.uint8)).cuda() for p in c["pics"]]
        planes = np.array([d.data_ptr() + c["org"][j] * isz for d in d_pics for j in range(3)], np.uint64)
        u, m, st = c["maps"][k]
        u = u.copy(); m = m.copy(); st = st.copy()
        ctx = np.zeros(160, np.uint8); ctx[:len(c["starts"][k][0])] = c["starts"][k][0]
        coeff = np.zeros(RD_TILE, np.int16); res = np.zeros(1, CTU_RESULT_DT)
        with call_stream(L) as st_:
            fn = L.lib.x265amd_compress_ctu_inter_ex if ex else L.lib.x265amd_compress_ctu_inter
            rc = fn(me.ctx, st_, _ptr(info), _ptr(sp), _ptr(si), _ptr(c["ap"]), _ptr(u), _ptr(m), _ptr(c["col"]), _ptr(c["ref_depth"]), _ptr(c["ref_qp0"]), _ptr(planes),
                    len(c["pics"]), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), _ptr(st), a, _ptr(ctx), C.c_uint64(c["starts"][k][1]), _ptr(coeff), _ptr(res),
                    *([None] if ex else []))
        assert rc == 0, L.lib.x265amd_last_error()
        cx, cy = (a % ctuW) * 16, (a // ctuW) * 16
        recon_pic = d_pics[-2].cpu().numpy().view(c["pics"][0].dtype)
        out.append((res[0].copy(), u[cy:cy + 16, cx:cx + 16].copy(), m.reshape(-1, w4)[cy:cy + 16, cx:cx + 16].copy(), coeff, ctu_recon(c, recon_pic, a), st))
    return out


def _ctu_first_fields(u, first):
    """merge_flag, mvp_idx, mvd at the first unit of each CU, and only where the syntax codes them: the merge index (mvp_idx[0]) of merged
    CUs, mvp_idx[l] / mvd[l] of the lists a non-merged CU uses (the reference leaves stale values elsewhere)"""
    f = first.reshape(256) & (u["pred_mode"].reshape(256) != MODE_NONE)
    mf = u["merge_flag"].reshape(256).astype(np.int16)
    idir = u["inter_dir"].reshape(256).astype(np.int16)
    cols = [mf * f]
    for l in range(2):
        used = f & (((mf == 0) & ((idir >> l) & 1 == 1)) | ((mf == 1) & (l == 0)))
        cols.append(u["mvp_idx"].reshape(256, 2)[:, l].astype(np.int16) * used)
    for l in range(2):
        used = f & (mf == 0) & ((idir >> l) & 1 == 1)
        for k in range(2):
            cols.append(u["mvd"].reshape(256, 2, 2)[:, l, k].astype(np.int16) * used)
    return np.stack(cols, 1)


def ctu_pack(results):
    """golden form of ctu_run_* results: only what the product is specified to reproduce (see x265amd_compress_ctu_inter)"""
    out = []
    for (r, u, m, coeff, rec, st) in results:
        first = np.zeros((16, 16), bool)            # first unit of each CU
        for y in range(16):
            for x in range(16):
                n = 16 >> int(u["depth"][y, x])
                ps = int(u["part_size"][y, x]) if int(u["pred_mode"][y, x]) != MODE_INTRA else 0
                xs = {2: (0, n // 2), 6: (0, n // 4), 7: (0, 3 * n // 4)}.get(ps, (0,))        # first unit of each PU
                ys = {1: (0, n // 2), 4: (0, n // 4), 5: (0, 3 * n // 4)}.get(ps, (0,))
                first[y, x] = (x % n in xs) and (y % n in ys)
        d = dict(res=np.array([int(r["rd_cost"]), int(r["distortion"]), int(r["total_bits"]), int(r["frac_bits"])], np.uint64), ctx=r["ctx"][:CTX_COUNT].copy(),
                 units=np.concatenate([u[f].astype(np.int16).reshape(256, -1) * (1 if f not in ("inter_dir", "ref_idx") else (u["pred_mode"].reshape(256, 1) != MODE_INTRA))
                                       for f in ("depth", "pred_mode", "part_size", "tu_depth", "cbf", "inter_dir", "ref_idx", "qp")], 1),
                 first=_ctu_first_fields(u, first),
                 motion=np.concatenate([m[f].astype(np.int16).reshape(256, -1) * (1 if f == "pred_mode" else (m["pred_mode"].reshape(256, 1) != MODE_INTRA))
                                        for f in ("pred_mode", "inter_dir", "ref_idx", "mv")], 1),
                 intra=np.stack([u[f].astype(np.int16).reshape(256) * (u["pred_mode"].reshape(256) == MODE_INTRA) for f in ("luma_dir", "chroma_dir")], 1),
                 recon=np.concatenate([p.astype(np.uint16).ravel() for p in rec]),
                 stat=np.concatenate([st["count"].astype(np.uint64).ravel(), st["avg_cost"].ravel()]))
        # levels of coded blocks only: mask by the luma / chroma coded block flags at each unit's own transform depth
        keep = np.zeros(RD_TILE, bool)
        for y in range(16):
            for x in range(16):
                z = _zorder(x, y)
                td = int(u["tu_depth"][y, x])
                if (int(u["cbf"][y, x, 0]) >> td) & 1:
                    keep[z * 16:z * 16 + 16] = True
        d["coeff"] = (coeff[:4096] * keep[:4096]).astype(np.int16)
        out.append(d)
    return out


# ---- intra candidates of inter slices (x265amd_intra_in_inter vs Search::checkIntraInInter + encodeIntraInInter) ----
def intra_rd_case(depth, seed, slice_type, psy_rd, ncu=10, strong=1):
    """rd_case plus a reconstructed picture (the source with coding-like noise) that supplies the intra neighbours; CU sizes 8..32"""
    c = rd_case(depth, seed, slice_type, 1, psy_rd, ncu=ncu)
    rng = np.random.default_rng(seed + 313)
    dt = c["preds"].dtype
    pmax = (1 << depth) - 1
    c["rec"] = [np.ascontiguousarray(np.clip(p.astype(np.int64) + rng.integers(-3, 4, p.shape), 0, pmax).astype(dt)) for p in c["src"]]
    for i in range(ncu):
        cu = c["cus"][i]
        log2 = int(rng.choice([3, 3, 4, 4, 5]))
        size = 1 << log2
        edge = int(rng.integers(0, 4))
        x = 0 if edge == 0 else int(rng.integers(0, c["width"] // size)) * size
        y = 0 if edge == 1 else int(rng.integers(0, c["height"] // size)) * size
        cu["x"], cu["y"], cu["log2_size"] = x, y, log2
    c["rp"]["strong"] = strong
    return c


def intra_rd_run_ref(R, c):
    """returns (results, cu_units_out, coeff, recon tiles, pred luma tiles, info (n x 4))"""
    n = len(c["cus"])
    dt = c["preds"].dtype
    res = np.zeros(n, RD_RESULT_DT); uo = np.zeros((n, 256), CU_UNIT_DT); coeff = np.zeros((n, RD_TILE), np.int16); recon = np.zeros((n, RD_TILE), dt)
    pred = np.zeros((n, 4096), dt); info = np.zeros((n, 4), np.uint64)
    si = np.array([c["si"]], SLICE_INFO_DT)
    planes = np.array([p.ctypes.data for p in c["src"]], np.uint64)
    for i in range(n):
        cu = c["cus"][i]
        rec = [p.copy() for p in c["rec"]]
        rplanes = np.array([p.ctypes.data for p in rec], np.uint64)
        ctx = np.zeros(160, np.uint8); ctx[:] = cu["ctx"]
        m = np.ascontiguousarray(c["units"])
        R.lib.ref_intra_in_inter(_ptr(si), _ptr(c["rp"]), _ptr(m), _ptr(planes), _ptr(rplanes), C.c_ssize_t(c["width"]), C.c_ssize_t(c["width"] // 2),
                                 int(cu["x"]), int(cu["y"]), int(cu["log2_size"]), int(cu["qp"]), _ptr(ctx), C.c_uint64(int(cu["frac_bits"])), int(c["rp"]["strong"][0]),
                                 off(uo[i], 0), off(coeff[i], 0), off(pred[i], 0), off(recon[i], 0), off(recon[i], 4096), off(recon[i], 4096 + 1024), off(res, i), off(info[i], 0))
    return res, uo, coeff, recon, pred, info


def intra_rd_run_hip(L, c):
    """x265amd_intra_in_inter per candidate, each on a fresh copy of the reconstructed picture; same return shape as intra_rd_run_ref"""
    import torch
    n = len(c["cus"])
    dt = c["preds"].dtype
    isz = dt.itemsize
    d_src = [torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1)).cuda() for p in c["src"]]
    planes = np.array([d.data_ptr() for d in d_src], np.uint64)
    si = np.array([c["si"]], SLICE_INFO_DT)
    res = np.zeros(n, RD_RESULT_DT); uo = np.zeros((n, 256), CU_UNIT_DT); coeff = np.zeros((n, RD_TILE), np.int16); recon = np.zeros((n, RD_TILE), dt)
    pred = np.zeros((n, 4096), dt); info = np.zeros((n, 4), np.uint64)
    for i in range(n):
        d_rec = [torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1)).cuda() for p in c["rec"]]
        rplanes = np.array([d.data_ptr() for d in d_rec], np.uint64)
        d_pred = torch.zeros(RD_TILE * isz, dtype=torch.uint8, device="cuda")
        d_recon = torch.zeros(RD_TILE * isz, dtype=torch.uint8, device="cuda")
        units = np.ascontiguousarray(c["units"].copy())
        with call_stream(L) as st_:
            rc = L.lib.x265amd_intra_in_inter(st_, _ptr(si), _ptr(c["rp"]), _ptr(units), _ptr(planes), _ptr(rplanes), C.c_ssize_t(c["width"]), C.c_ssize_t(c["width"] // 2),
                                              off(c["cus"], i), off(uo[i], 0), C.c_uint64(d_pred.data_ptr()), C.c_uint64(d_recon.data_ptr()), off(res, i), off(coeff[i], 0),
                                              off(info[i], 0))
        assert rc == 0, L.lib.x265amd_last_error()
        assert np.array_equal(units, c["units"])
        recon[i] = d_recon.cpu().numpy().view(dt)
        pred[i] = d_pred.cpu().numpy().view(dt)[:4096]
    return res, uo, coeff, recon, pred, info


def intra_rd_pack(r, c):
    """golden form: rd_pack's fields plus the intra directions, the luma prediction and the scan's choice"""
    res, uo, coeff, recon, pred, info = r
    base = rd_pack((res, uo, coeff, recon), c)
    for i, d in enumerate(base):
        cu = c["cus"][i]
        S = 1 << int(cu["log2_size"]); n4 = S // 4
        d["dirs"] = np.stack([uo[i]["luma_dir"][:n4 * n4], uo[i]["chroma_dir"][:n4 * n4], uo[i]["part_size"][:n4 * n4]], 1).astype(np.int16)
        d["pred"] = pred[i].reshape(64, 64)[:S, :S].astype(np.uint16).ravel()
        d["info"] = info[i].copy()
        # an intra CU's levels are always exported
        d["coeff"] = np.concatenate([coeff[i][:S * S], coeff[i][4096:4096 + S * S // 4], coeff[i][5120:5120 + S * S // 4]])
    return base


# ---- Search::checkIntra (I slices / rd 5-6): x265amd_check_intra ----
def check_intra_case(depth, seed, slice_type, psy_rd, ncu=10, strong=1, tu_intra=0):
    c = intra_rd_case(depth, seed, slice_type, psy_rd, ncu=ncu, strong=strong)
    if tu_intra:
        c["si"]["tu_max_depth_intra"] = tu_intra
    rng = np.random.default_rng(seed + 717)
    c["parts"] = [3 if (int(c["cus"][i]["log2_size"]) == 3 and rng.integers(0, 2)) else 0 for i in range(ncu)]
    return c


def check_intra_run_ref(R, c):
    n = len(c["cus"])
    dt = c["preds"].dtype
    res = np.zeros(n, RD_RESULT_DT); uo = np.zeros((n, 256), CU_UNIT_DT); coeff = np.zeros((n, RD_TILE), np.int16); recon = np.zeros((n, RD_TILE), dt)
    pred = np.zeros((n, 4096), dt); info = np.zeros((n, 4), np.uint64)
    si = np.array([c["si"]], SLICE_INFO_DT)
    planes = np.array([p.ctypes.data for p in c["src"]], np.uint64)
    for i in range(n):
        cu = c["cus"][i]
        rec = [p.copy() for p in c["rec"]]
        rplanes = np.array([p.ctypes.data for p in rec], np.uint64)
        ctx = np.zeros(160, np.uint8); ctx[:] = cu["ctx"]
        m = np.ascontiguousarray(c["units"])
        R.lib.ref_check_intra(_ptr(si), _ptr(c["rp"]), _ptr(m), _ptr(planes), _ptr(rplanes), C.c_ssize_t(c["width"]), C.c_ssize_t(c["width"] // 2),
                              int(cu["x"]), int(cu["y"]), int(cu["log2_size"]), int(cu["qp"]), _ptr(ctx), C.c_uint64(int(cu["frac_bits"])), int(c["rp"]["strong"][0]),
                              int(c["parts"][i]), off(uo[i], 0), off(coeff[i], 0), off(pred[i], 0), off(recon[i], 0), off(recon[i], 4096), off(recon[i], 4096 + 1024), off(res, i))
    return res, uo, coeff, recon, pred, info


def check_intra_run_hip(L, c):
    import torch
    n = len(c["cus"])
    dt = c["preds"].dtype
    isz = dt.itemsize
    d_src = [torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1)).cuda() for p in c["src"]]
    planes = np.array([d.data_ptr() for d in d_src], np.uint64)
    si = np.array([c["si"]], SLICE_INFO_DT)
    res = np.zeros(n, RD_RESULT_DT); uo = np.zeros((n, 256), CU_UNIT_DT); coeff = np.zeros((n, RD_TILE), np.int16); recon = np.zeros((n, RD_TILE), dt)
    pred = np.zeros((n, 4096), dt); info = np.zeros((n, 4), np.uint64)
    for i in range(n):
        d_rec = [torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1)).cuda() for p in c["rec"]]
        rplanes = np.array([d.data_ptr() for d in d_rec], np.uint64)
        d_pred = torch.zeros(RD_TILE * isz, dtype=torch.uint8, device="cuda")
        d_recon = torch.zeros(RD_TILE * isz, dtype=torch.uint8, device="cuda")
        units = np.ascontiguousarray(c["units"].copy())
        with call_stream(L) as st_:
            rc = L.lib.x265amd_check_intra(st_, _ptr(si), _ptr(c["rp"]), _ptr(units), _ptr(planes), _ptr(rplanes), C.c_ssize_t(c["width"]), C.c_ssize_t(c["width"] // 2),
                                           off(c["cus"], i), int(c["parts"][i]), off(uo[i], 0), C.c_uint64(d_pred.data_ptr()), C.c_uint64(d_recon.data_ptr()), off(res, i),
                                           off(coeff[i], 0))
        assert rc == 0, L.lib.x265amd_last_error()
        assert np.array_equal(units, c["units"])
        recon[i] = d_recon.cpu().numpy().view(dt)
        pred[i] = d_pred.cpu().numpy().view(dt)[:4096]
    return res, uo, coeff, recon, pred, info


# ---- frame pipeline (x265amd_analyse_frame) against the reference encoder itself ----
FRAME_CLIP_SEED = 4242
FRAME_CLI_ARGS = ["--preset", "medium", "--qp", "30", "--aq-mode", "0", "--no-cutree", "--no-weightp", "--no-weightb", "--bframes", "0", "--b-adapt", "0",
                  "--no-scenecut", "--keyint", "250", "--rd", "3", "--no-sao", "--no-deblock", "--no-wpp", "--frame-threads", "1", "--pools", "none",
                  "--rdoq-level", "0", "--psy-rdoq", "0", "--ref", "3", "--max-merge", "3", "--no-info", "--no-open-gop", "--rc-lookahead", "0",
                  "--lookahead-slices", "0"]


STREAM_PARAMS_DT = np.dtype([("tier_flag", "<i4"), ("profile_idc", "<i4"), ("profile_compatibility_flags", "<u4"),
                             ("progressive_source", "<i4"), ("interlaced_source", "<i4"), ("non_packed_constraint", "<i4"), ("frame_only_constraint", "<i4"),
                             ("bit_depth_constraint", "<i4"), ("chroma_format_constraint", "<i4"), ("intra_constraint", "<i4"), ("one_picture_only_constraint", "<i4"),
                             ("lower_bit_rate_constraint", "<i4"), ("level_idc", "<i4"),
                             ("max_temporal_sub_layers", "<i4"), ("max_dec_pic_buffering", "<i4", 8), ("num_reorder_pics", "<i4", 8), ("max_latency_increase", "<i4", 8),
                             ("chroma_format_idc", "<i4"), ("pic_width", "<i4"), ("pic_height", "<i4"), ("conformance_window", "<i4"), ("conf_win_offsets", "<i4", 4),
                             ("bit_depth", "<i4"), ("log2_max_poc_lsb", "<i4"), ("log2_min_cu_size", "<i4"), ("log2_diff_max_min_cu_size", "<i4"),
                             ("tu_log2_min", "<i4"), ("tu_log2_max", "<i4"), ("tu_max_depth_inter", "<i4"), ("tu_max_depth_intra", "<i4"),
                             ("amp", "<i4"), ("sao", "<i4"), ("temporal_mvp", "<i4"), ("strong_intra_smoothing", "<i4"),
                             ("aspect_ratio_idc", "<i4"), ("sar_width", "<i4"), ("sar_height", "<i4"),
                             ("overscan_info_present", "<i4"), ("overscan_appropriate", "<i4"), ("video_signal_type_present", "<i4"), ("video_format", "<i4"),
                             ("video_full_range", "<i4"), ("colour_description_present", "<i4"), ("colour_primaries", "<i4"), ("transfer_characteristics", "<i4"),
                             ("matrix_coefficients", "<i4"), ("chroma_loc_info_present", "<i4"), ("chroma_sample_loc_top", "<i4"), ("chroma_sample_loc_bottom", "<i4"),
                             ("field_seq", "<i4"), ("frame_field_info_present", "<i4"), ("default_display_window", "<i4"), ("def_disp_win_offsets", "<i4", 4),
                             ("emit_timing_info", "<i4"), ("num_units_in_tick", "<u4"), ("time_scale", "<u4"),
                             ("sign_hide", "<i4"), ("num_ref_idx_default", "<i4", 2), ("init_qp_minus26", "<i4"), ("constrained_intra_pred", "<i4"), ("transform_skip", "<i4"),
                             ("use_dqp", "<i4"), ("max_cu_dqp_depth", "<i4"), ("cb_qp_offset", "<i4"), ("cr_qp_offset", "<i4"), ("slice_chroma_qp_offsets_present", "<i4"),
                             ("weighted_pred", "<i4"), ("weighted_bipred", "<i4"), ("transquant_bypass", "<i4"), ("wpp", "<i4"), ("loop_filter_across_slices", "<i4"),
                             ("deblocking_filter_control_present", "<i4"), ("pic_disable_deblocking", "<i4"), ("beta_offset_div2", "<i4"), ("tc_offset_div2", "<i4")])


def frame_stream_params(bframes=0, deblock=False, wpp=False, sao=False, amp=False, qp=30):
    """what the reference encoder configures for FRAME_CLI_ARGS (+ the variations of the end-to-end goldens) on the MC_W x MC_H clip at 30 fps:
    Main profile, level 2, 8-bit 4:2:0, CTU 64 / min CU 8, TU 4..32 with depth 1, --ref 3"""
    p = np.zeros(1, STREAM_PARAMS_DT)[0]
    p["profile_idc"], p["profile_compatibility_flags"], p["progressive_source"], p["frame_only_constraint"], p["level_idc"] = 1, 0x6, 1, 1, 60
    p["max_temporal_sub_layers"] = 1
    p["num_reorder_pics"][0] = 1 if bframes else 0                          # no b-pyramid
    p["max_dec_pic_buffering"][0] = min(16, max(p["num_reorder_pics"][0] + 2, 3) + 1)     # maxNumReferences 3 (Encoder::initSPS / initVPS)
    p["max_latency_increase"][0] = bframes                                   # Encoder::initSPS: maxLatencyIncrease = param.bframes
    p["chroma_format_idc"], p["pic_width"], p["pic_height"], p["bit_depth"], p["log2_max_poc_lsb"] = 1, MC_W, MC_H, 8, 8
    p["log2_min_cu_size"], p["log2_diff_max_min_cu_size"], p["tu_log2_min"], p["tu_log2_max"], p["tu_max_depth_inter"], p["tu_max_depth_intra"] = 3, 3, 2, 5, 1, 1
    p["amp"], p["sao"], p["temporal_mvp"], p["strong_intra_smoothing"] = int(amp), int(sao), 1, 1
    p["aspect_ratio_idc"] = 1
    p["emit_timing_info"], p["num_units_in_tick"], p["time_scale"] = 1, 1, 30
    p["sign_hide"], p["num_ref_idx_default"] = 1, (1, 1)
    p["init_qp_minus26"] = 0
    p["wpp"], p["loop_filter_across_slices"] = int(wpp), 1
    p["deblocking_filter_control_present"], p["pic_disable_deblocking"] = int(not deblock), int(not deblock)
    return p


def frame_stream_headers(L, **config):
    lib = L.lib
    lib.x265amd_write_stream_headers.restype = C.c_size_t
    p = np.array([frame_stream_params(**config)])
    out = np.zeros(512, np.uint8)
    n = lib.x265amd_write_stream_headers(_ptr(p), _ptr(out), C.c_size_t(out.size))
    assert 0 < n <= out.size
    return out[:n].copy()


def frame_clip(depth=8, nframes=4):
    """source frames (padded flat Y|U|V arrays in inter_scene geometry), in coding order"""
    pics, stride, cstride, org = inter_scene(depth, FRAME_CLIP_SEED, npics=4)
    order = [pics[3], pics[0], pics[1], pics[2]][:nframes]
    return order, stride, cstride, org


def frame_planes(pic, stride, cstride, org):
    out = []
    for k in range(3):
        st = stride if k == 0 else cstride
        w, h = (MC_W, MC_H) if k == 0 else (MC_W // 2, MC_H // 2)
        out.append(np.stack([pic[org[k] + r * st:org[k] + r * st + w] for r in range(h)]))
    return out


SAO_CTU_PROD_DT = np.dtype([("type", "i1", 2), ("band_pos", "u1", 3), ("offset", "i1", (3, 4)), ("merge", "u1"), ("reserved", "u1", 2)])
SLICE_HEADER_DT = np.dtype([(n, "<i4") for n in ("nal_unit_type", "temporal_id_plus1", "first_in_access_unit", "slice_type", "poc", "last_idr_poc", "log2_max_poc_lsb",
                                                    "rps_idx", "num_rps_in_sps", "num_negative", "num_positive")] + [("delta_poc", "<i4", 16), ("used", "<i4", 16)] +
                           [(n, "<i4") for n in ("temporal_mvp_enabled", "use_sao", "sao_luma", "sao_chroma", "selective_sao")] +
                           [("num_ref_idx", "<i4", 2), ("num_ref_idx_default", "<i4", 2)] +
                           [(n, "<i4") for n in ("col_from_l0", "col_ref_idx", "max_num_merge_cand", "slice_qp", "pps_init_qp", "chroma_qp_offsets_present", "cb_qp_offset",
                                                 "cr_qp_offset", "deblocking_disabled", "slfase_flag", "wpp", "weighted_pred", "luma_log2_weight_denom", "chroma_log2_weight_denom", "weighted_bipred")] +
                           [("wp", np.dtype([("w", "<i2"), ("o", "<i2"), ("denom", "u1"), ("present", "u1")]), (2, 16, 3))])
assert SLICE_HEADER_DT.itemsize == 844


def frame_clip_b(depth=8):
    """7 source frames in display order for the B-frame clip"""
    pics, stride, cstride, org = inter_scene(depth, 777, npics=7)
    return pics, stride, cstride, org


def frame_slice_header(k, sched, slice_qp, deblock, wpp, dpb, sao_flags=None):
    """the slice header fields of the k-th coded frame as the reference's DPB / encoder set them (dpb.cpp: prepareEncode / computeRPS,
    encoder.cpp); dpb: POCs of the reference pictures kept so far"""
    stype, poc, referenced = int(sched[0]), int(sched[1]), int(sched[2])
    l0 = [int(v) for v in sched[3:7] if v >= 0]; l1 = [int(v) for v in sched[7:11] if v >= 0]
    h = np.zeros(1, SLICE_HEADER_DT)
    h["nal_unit_type"] = 20 if stype == 2 else (1 if referenced else 0)     # IDR_N_LP / TRAIL_R / TRAIL_N
    h["first_in_access_unit"] = 1                       # each picture's slice NAL opens its own NAL list (the stream headers are emitted separately)
    h["slice_type"], h["poc"], h["log2_max_poc_lsb"], h["rps_idx"] = stype, poc, 8, -1
    neg = sorted([p for p in dpb if p < poc], reverse=True); pos = sorted([p for p in dpb if p > poc])
    h["num_negative"], h["num_positive"] = len(neg), len(pos)
    for j, p in enumerate(neg + pos):
        h["delta_poc"][0, j] = p - poc; h["used"][0, j] = 1
    h["temporal_mvp_enabled"] = 1
    h["num_ref_idx"] = (len(l0), len(l1)); h["num_ref_idx_default"] = (1, 1); h["col_from_l0"] = int(stype != 0); h["max_num_merge_cand"] = 3
    h["slice_qp"], h["pps_init_qp"], h["deblocking_disabled"], h["wpp"] = slice_qp, 26, int(not deblock), int(wpp)
    h["slfase_flag"] = (0x5f4e4a53 >> (poc % 31)) & 1   # SLFASE_CONSTANT (dpb.cpp:294)
    if sao_flags is not None:
        h["use_sao"], h["sao_luma"], h["sao_chroma"] = 1, int(sao_flags[0]), int(sao_flags[1])
    return h


def frame_pipeline_run_hip(L, me, slice_qps, nframes=4, depth=8, deblock=False, wpp=False, schedule=None, frames=None, sao=False, rect=0, amp=0, limit_modes=0,
                           rd_level=3):
    """frames through x265amd_analyse_frame the way the reference's frame encoder strings them together (CQP, no AQ, optional deblocking and
    wavefront sub-streams).  schedule: per coded frame (type 2 I / 1 P / 0 B, poc, referenced, 4 L0 pocs, 4 L1 pocs), default I P P P.
    Returns per coded frame (poc, recon planes, the slice NAL unit with its start code)"""
    import torch
    if frames is None:
        frames, stride, cstride, org = frame_clip(depth, nframes)
    else:
        frames, stride, cstride, org = frames
    if schedule is None:
        schedule = [[2 if k == 0 else 1, k, 1] + (list(range(k - 1, max(-1, k - 4), -1)) + [-1] * 4)[:4] + [-1] * 4 for k in range(nframes)]
    isz = frames[0].itemsize
    W, H = MC_W, MC_H
    w4, h4, nctu = W // 4, H // 4, (W // 64) * (H // 64)
    lib = L.lib
    lib.x265amd_write_slice_nal.restype = C.c_size_t
    d_src = {p: torch.from_numpy(frames[p].view(np.uint8)).cuda() for p in range(len(frames))}
    d_rec = {}
    def addr(d):
        return [d.data_ptr() + org[k] * isz for k in range(3)]
    fields, unit_maps, refpocs, qp_of, dpb, out = {}, {}, {}, {}, [], []
    depth_sao_rate = np.zeros(8, np.float64)
    for k, sc in enumerate(schedule):
        stype, poc, referenced = int(sc[0]), int(sc[1]), int(sc[2])
        lists = [[int(v) for v in sc[3:7] if v >= 0], [int(v) for v in sc[7:11] if v >= 0]]
        d_rec[poc] = torch.zeros_like(d_src[poc])
        planes, index = [], {}
        for l in range(2):
            for r in lists[l]:
                if r not in index:
                    index[r] = len(planes) // 3
                    planes += addr(d_rec[r])
        planes += addr(d_rec[poc]) + addr(d_src[poc])
        planes = np.array(planes, np.uint64)
        info = np.zeros(1, MVPRED_INFO_DT)
        info["pic_width"], info["pic_height"], info["is_inter_b"], info["max_num_merge_cand"] = W, H, int(stype == 0), 3
        info["num_ref_idx"] = (len(lists[0]), len(lists[1]))
        info["temporal_mvp"], info["col_from_l0"], info["check_ldc"], info["poc"] = 1, int(stype != 0), int(stype != 0), poc
        rp = np.zeros((2, 16), np.int32)
        for l in range(2):
            rp[l, :len(lists[l])] = lists[l]
        info["ref_poc"] = rp
        col_poc = None
        if stype != 2:
            col_poc = lists[0][0] if stype == 1 else lists[1][0]
            info["col_poc"] = col_poc
            info["col_ref_poc"] = refpocs[col_poc]
        sp = np.zeros(1, INTER_SP_DT)
        sp["search_method"], sp["subpel_refine"], sp["search_range"], sp["qp"], sp["chroma_mc"] = ME_HEX, 2, 57, slice_qps[k], 1
        rpic = np.zeros((2, 16), np.int32)
        for l in range(2):
            rpic[l, :len(lists[l])] = [index[r] for r in lists[l]]
        sp["ref_pic"] = rpic
        si = np.zeros(1, SLICE_INFO_DT)
        si["pic_width"], si["pic_height"], si["slice_type"], si["slice_qp"] = W, H, stype, slice_qps[k]
        si["num_ref_idx"] = (len(lists[0]), len(lists[1]))
        si["max_num_merge_cand"], si["sign_hide"], si["max_cu_depth"], si["tu_log2_min"], si["tu_log2_max"] = 3, 1, 3, 2, 5
        si["tu_max_depth_inter"], si["tu_max_depth_intra"], si["wpp"] = 1, 1, int(wpp)
        ap = np.zeros(1, ANALYSIS_PARAMS_DT)
        ap["psy_rd"], ap["early_skip"], ap["rskip"], ap["limit_refs"], ap["b_intra"], ap["strong"] = 2.0, 1, 1, 3, 1, 1
        ap["use_sao"] = int(sao)
        ap["rect"], ap["amp"], ap["limit_modes"], ap["rd_level"] = rect, amp, limit_modes, rd_level
        si["max_amp_depth"] = 3 if amp else 0
        units = np.zeros((h4, w4), CU_UNIT_DT); cur = np.zeros((h4, w4), MV_UNIT_DT)
        col = fields[col_poc] if col_poc is not None else np.zeros((h4, w4), MV_UNIT_DT)
        ref_depth = np.zeros((2, h4, w4), np.uint8)
        ref_qp0 = np.zeros((2, nctu), np.int8)
        for l in range(2):
            if lists[l]:
                ref_depth[l] = unit_maps[lists[l][0]]["depth"]
                ref_qp0[l, :] = qp_of[lists[l][0]]
        stat = np.zeros(nctu + 1, CU_STAT_DT)
        coeff = np.zeros((nctu, RD_TILE), np.int16)
        data = np.zeros(1 << 20, np.uint8); sizes = np.zeros(64, np.uint32); nsub = C.c_int(0)
        rc = lib.x265amd_analyse_frame(me.ctx, None, _ptr(info), _ptr(sp), _ptr(si), _ptr(ap), _ptr(units), _ptr(cur), _ptr(col), _ptr(ref_depth), _ptr(ref_qp0),
                                       _ptr(planes), len(planes) // 3, C.c_int64(stride), C.c_int64(cstride), _ptr(stat), _ptr(coeff), None,
                                       None if sao else _ptr(data), C.c_size_t(data.size), _ptr(sizes), C.byref(nsub))
        assert rc == 0, lib.x265amd_last_error()
        if deblock:
            # FrameFilter: in-loop deblocking of the finished picture (default offsets), before it becomes a reference
            dbu = np.zeros(w4 * h4, DB_UNIT_DT)
            assert lib.x265amd_deblock_units(_ptr(si), _ptr(info), _ptr(units), _ptr(cur), _ptr(dbu)) == 0
            d_dbu = torch.from_numpy(dbu.view(np.uint8)).cuda()
            pl = addr(d_rec[poc])
            assert lib.x265amd_deblock_picture(None, C.c_void_p(pl[0]), C.c_void_p(pl[1]), C.c_void_p(pl[2]), C.c_int64(stride), C.c_int64(cstride), W, H,
                                               C.c_void_p(d_dbu.data_ptr()), 0, 0, 0, 0, 0, 3) == 0
            torch.cuda.synchronize()
        sao_flags = None
        if sao:
            # SAO: statistics of all CTUs on the deblocked picture (GPU), parameter decision (host), offsets applied out of place (GPU),
            # then the slice data with the SAO syntax in front of every CTU
            n_stat = nctu * 3 * 5 * 32
            d_count = torch.zeros(n_stat, dtype=torch.int32, device="cuda"); d_org = torch.zeros(n_stat, dtype=torch.int32, device="cuda")
            recp = np.array(addr(d_rec[poc]), np.uint64); srcp = np.array(addr(d_src[poc]), np.uint64)
            assert lib.x265amd_sao_stats(None, _ptr(recp), _ptr(srcp), C.c_int64(stride), C.c_int64(cstride), W, H, C.c_void_p(d_count.data_ptr()),
                                         C.c_void_p(d_org.data_ptr())) == 0
            torch.cuda.synchronize()
            cnt = d_count.cpu().numpy(); orgs = d_org.cpu().numpy()
            sparams = np.zeros(nctu, SAO_CTU_PROD_DT); sao_flags = np.zeros(2, np.int32)
            assert lib.x265amd_sao_rdo(_ptr(si), referenced, 1, 0, 69, _ptr(units), _ptr(cnt), _ptr(orgs), _ptr(depth_sao_rate), _ptr(sparams), _ptr(sao_flags)) == 0
            d_params = torch.from_numpy(sparams.view(np.uint8)).cuda()
            d_out = d_rec[poc].clone()
            dstp = np.array(addr(d_out), np.uint64)
            assert lib.x265amd_sao_apply(None, _ptr(recp), _ptr(dstp), C.c_int64(stride), C.c_int64(cstride), W, H, C.c_void_p(d_params.data_ptr())) == 0
            torch.cuda.synchronize()
            d_rec[poc] = d_out
            assert lib.x265amd_encode_slice_data(_ptr(si), _ptr(units), _ptr(coeff), _ptr(sparams), _ptr(sao_flags), _ptr(data), C.c_size_t(data.size), _ptr(sizes),
                                                 C.byref(nsub)) == 0
        # the reconstruction becomes a reference: extend its borders (PicYuv margins 96 / 80)
        for p in range(3):
            w, h, mx, my, st = (W, H, MC_MX, MC_MY, stride) if p == 0 else (W // 2, H // 2, MC_MX // 2, MC_MY // 2, cstride)
            assert lib.x265amd_extend_pic_border(None, C.c_void_p(d_rec[poc].data_ptr() + org[p] * isz), C.c_int64(st), w, h, mx, my) == 0
        torch.cuda.synchronize()
        fields[poc] = np.ascontiguousarray(cur); unit_maps[poc] = units; refpocs[poc] = rp; qp_of[poc] = slice_qps[k]
        rec = d_rec[poc].cpu().numpy().view(frames[0].dtype)
        nal = np.zeros(1 << 20, np.uint8)
        hdr = frame_slice_header(k, sc, slice_qps[k], deblock, wpp, dpb, sao_flags)
        n = lib.x265amd_write_slice_nal(_ptr(hdr), _ptr(data), _ptr(sizes), nsub.value, _ptr(nal), C.c_size_t(nal.size))
        assert 0 < n <= nal.size
        if referenced:
            dpb.append(poc)
        out.append((poc, frame_planes(rec, stride, cstride, org), nal[:n].copy()))
    return out


# ---- the encoder object (include/x265amd_encoder.h): x265_encoder_open / headers / encode / close over the frame pipeline ----
class EncParam(C.Structure):
    _fields_ = [("sourceWidth", C.c_int32), ("sourceHeight", C.c_int32), ("fpsNum", C.c_uint32), ("fpsDenom", C.c_uint32), ("bframes", C.c_int32),
                ("keyframeMax", C.c_int32), ("maxNumReferences", C.c_int32), ("qp", C.c_int32), ("ipFactor", C.c_double), ("pbFactor", C.c_double),
                ("rdLevel", C.c_int32), ("bEnableRectInter", C.c_int32), ("bEnableAMP", C.c_int32), ("limitModes", C.c_int32), ("limitReferences", C.c_int32),
                ("bEnableEarlySkip", C.c_int32), ("recursionSkipMode", C.c_int32), ("bIntraInBFrames", C.c_int32), ("psyRd", C.c_double),
                ("searchMethod", C.c_int32), ("subpelRefine", C.c_int32), ("searchRange", C.c_int32), ("maxNumMergeCand", C.c_int32),
                ("bEnableSignHiding", C.c_int32), ("bEnableStrongIntraSmoothing", C.c_int32), ("bEnableTemporalMvp", C.c_int32),
                ("tuQTMaxInterDepth", C.c_int32), ("tuQTMaxIntraDepth", C.c_int32), ("bEnableLoopFilter", C.c_int32), ("bEnableSAO", C.c_int32),
                ("bEnableWavefront", C.c_int32), ("aspectRatioIdc", C.c_int32), ("rdoqLevel", C.c_int32), ("psyRdoqFix8", C.c_int32), ("bEnableFastIntra", C.c_int32), ("firstFrame", C.c_int32), ("frameNumThreads", C.c_int32), ("scenecutThreshold", C.c_int32), ("lookaheadDepth", C.c_int32),
                ("keyframeMin", C.c_int32), ("shardRank", C.c_int32), ("shardCount", C.c_int32), ("bFrameAdaptive", C.c_int32), ("bOpenGOP", C.c_int32), ("bBPyramid", C.c_int32), ("lookaheadSlices", C.c_int32), ("bEnableWeightedPred", C.c_int32), ("bEnableWeightedBiPred", C.c_int32),
                ("rateControlMode", C.c_int32), ("rfConstant", C.c_double), ("aqStrength", C.c_double), ("qCompress", C.c_double), ("aqMode", C.c_int32), ("cuTree", C.c_int32),
                ("qgSize", C.c_int32), ("bEmitInfoSEI", C.c_int32), ("qpMin", C.c_int32), ("qpMax", C.c_int32), ("bRepeatHeaders", C.c_int32), ("reserved2", C.c_int32), ("vuiSarWidth", C.c_int32), ("vuiSarHeight", C.c_int32), ("vuiOverscanInfoPresent", C.c_int32),
                ("vuiOverscanAppropriate", C.c_int32), ("vuiVideoSignalTypePresent", C.c_int32), ("vuiVideoFormat", C.c_int32), ("vuiFullRange", C.c_int32), ("vuiColorDescriptionPresent", C.c_int32),
                ("vuiColorPrimaries", C.c_int32), ("vuiTransfer", C.c_int32), ("vuiMatrix", C.c_int32), ("vuiChromaLocPresent", C.c_int32), ("vuiChromaLocTop", C.c_int32), ("vuiChromaLocBottom", C.c_int32),
                ("vuiDisplayWindow", C.c_int32), ("vuiDispWinLeft", C.c_int32), ("vuiDispWinRight", C.c_int32), ("vuiDispWinTop", C.c_int32), ("vuiDispWinBottom", C.c_int32), ("reserved3", C.c_int32),
                ("bEnableAccessUnitDelimiters", C.c_int32), ("bEmitHDR10SEI", C.c_int32), ("bEmitCLL", C.c_int32), ("maxCLL", C.c_int32), ("maxFALL", C.c_int32), ("hasMasteringDisplay", C.c_int32),
                ("masteringDisplay", C.c_uint32 * 10), ("decodedPictureHashSEI", C.c_int32), ("reserved4", C.c_int32), ("deblockingFilterTCOffset", C.c_int32), ("deblockingFilterBetaOffset", C.c_int32), ("limitTU", C.c_int32), ("reserved5", C.c_int32)]


class RowExport(C.Structure):       # x265amd_row_export (include/x265amd_encoder.h)
    _fields_ = [("coding_index", C.c_uint64), ("ctu_row", C.c_int32), ("reserved", C.c_int32), ("src", C.c_void_p * 3), ("plane_offset", C.c_uint64 * 3), ("plane_bytes", C.c_uint64 * 3),
                ("units", C.c_void_p), ("units_bytes", C.c_uint64), ("motion", C.c_void_p), ("motion_bytes", C.c_uint64), ("map_offset_units", C.c_uint64), ("map_offset_motion", C.c_uint64)]


class EncNal(C.Structure):
    _fields_ = [("type", C.c_uint32), ("sizeBytes", C.c_uint32), ("payload", C.POINTER(C.c_uint8))]


class EncPicture(C.Structure):
    _fields_ = [("planes", C.c_void_p * 3), ("stride", C.c_int32 * 3), ("poc", C.c_int32), ("sliceType", C.c_int32), ("qp", C.c_int32)]


def encoder_run(L, planes_per_frame, width, height, want_headers=True, input_on_device=False, **overrides):
    """x265amd_encoder_open -> headers -> encode every frame -> flush -> close.  planes_per_frame: per frame (Y, U, V) arrays in display order.
    input_on_device: the frames are put on the GPU first (torch) and go in through x265amd_encoder_encode_device.
    Returns (whole byte stream, [(poc, slice type, qp, recon planes)] in coding order)"""
    lib = L.lib
    lib.x265amd_encoder_encode_device.argtypes = [C.c_void_p, C.POINTER(C.POINTER(EncNal)), C.POINTER(C.c_uint32), C.POINTER(EncPicture), C.POINTER(EncPicture)]
    lib.x265amd_encoder_open.restype = C.c_void_p
    lib.x265amd_encoder_open.argtypes = [C.POINTER(EncParam)]
    lib.x265amd_encoder_headers.argtypes = [C.c_void_p, C.POINTER(C.POINTER(EncNal)), C.POINTER(C.c_uint32)]
    lib.x265amd_encoder_encode.argtypes = [C.c_void_p, C.POINTER(C.POINTER(EncNal)), C.POINTER(C.c_uint32), C.POINTER(EncPicture), C.POINTER(EncPicture)]
    lib.x265amd_encoder_close.argtypes = [C.c_void_p]
    lib.x265amd_param_default.argtypes = [C.POINTER(EncParam)]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight = width, height
    for k, v in overrides.items():
        assert hasattr(prm, k), k
        setattr(prm, k, v)
    enc = lib.x265amd_encoder_open(C.byref(prm))
    assert enc, lib.x265amd_last_error()
    stream = bytearray()
    nal = C.POINTER(EncNal)(); nnal = C.c_uint32(0)
    assert lib.x265amd_encoder_headers(enc, C.byref(nal), C.byref(nnal)) > 0
    for i in range(nnal.value if want_headers else 0):
        stream += bytes(nal[i].payload[:nal[i].sizeBytes])
    dt = planes_per_frame[0][0].dtype
    coded = []

    def take(ret, out, bufs):
        assert ret >= 0, lib.x265amd_last_error()
        if ret:
            for i in range(nnal.value):
                stream.extend(bytes(nal[i].payload[:nal[i].sizeBytes]))
            coded.append((out.poc, out.sliceType, out.qp, [b.copy() for b in bufs]))
        return ret

    def out_picture():
        bufs = [np.zeros((height, width), dt), np.zeros((height // 2, width // 2), dt), np.zeros((height // 2, width // 2), dt)]
        out = EncPicture()
        for k in range(3):
            out.planes[k] = bufs[k].ctypes.data; out.stride[k] = bufs[k].strides[0]
        return out, bufs

    try:
        for planes in planes_per_frame:
            pic = EncPicture()
            keep = [np.ascontiguousarray(pl) for pl in planes]
            if input_on_device:
                import torch
                keep = [torch.from_numpy(k.view(np.uint8).reshape(k.shape[0], -1)).cuda() for k in keep]         # (bytes: torch has no unsigned 16-bit type)
                torch.cuda.synchronize()
                for k in range(3):
                    pic.planes[k] = keep[k].data_ptr(); pic.stride[k] = keep[k].stride(0)
            else:
                for k in range(3):
                    pic.planes[k] = keep[k].ctypes.data; pic.stride[k] = keep[k].strides[0]
            out, bufs = out_picture()
            fn = lib.x265amd_encoder_encode_device if input_on_device else lib.x265amd_encoder_encode
            take(fn(enc, C.byref(nal), C.byref(nnal), C.byref(pic), C.byref(out)), out, bufs)
        while True:
            out, bufs = out_picture()
            if not take(lib.x265amd_encoder_encode(enc, C.byref(nal), C.byref(nnal), None, C.byref(out)), out, bufs):
                break
    finally:
        lib.x265amd_encoder_close(enc)
    return np.frombuffer(bytes(stream), np.uint8), coded


def encoder_run_sharded(L, planes_per_frame, width, height, count, **overrides):
    """`count` encoder objects on one GPU, object r coding the pictures whose place in coding order is r modulo count (x265amd_param.shardRank / shardCount); a pump
    thread carries every finished CTU row from the object that codes it to the others (x265amd_encoder_export_row / _import_row, the calls
    x265-amod_amd/frame_rows.py makes between ranks).  Returns (the stream assembled from the owners' NAL units in coding order, coded pictures as encoder_run gives
    them, taken from the owners)"""
    import threading
    lib = L.lib
    lib.x265amd_encoder_open.restype = C.c_void_p
    lib.x265amd_encoder_open.argtypes = [C.POINTER(EncParam)]
    lib.x265amd_encoder_headers.argtypes = [C.c_void_p, C.POINTER(C.POINTER(EncNal)), C.POINTER(C.c_uint32)]
    lib.x265amd_encoder_encode.argtypes = [C.c_void_p, C.POINTER(C.POINTER(EncNal)), C.POINTER(C.c_uint32), C.POINTER(EncPicture), C.POINTER(EncPicture)]
    lib.x265amd_encoder_close.argtypes = [C.c_void_p]
    lib.x265amd_param_default.argtypes = [C.POINTER(EncParam)]
    lib.x265amd_encoder_export_row.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(RowExport), C.c_int]
    lib.x265amd_encoder_import_row.argtypes = [C.c_void_p, C.POINTER(RowExport)]
    lib.x265amd_encoder_ctu_rows.argtypes = [C.c_void_p]
    lib.x265amd_last_error.restype = C.c_char_p
    encs = []
    for r in range(count):
        prm = EncParam()
        lib.x265amd_param_default(C.byref(prm))
        prm.sourceWidth, prm.sourceHeight = width, height
        for k, v in overrides.items():
            setattr(prm, k, v)
        prm.shardRank, prm.shardCount = r, count
        enc = lib.x265amd_encoder_open(C.byref(prm))
        assert enc, lib.x265amd_last_error()
        encs.append(enc)
    header = bytearray()
    nal = C.POINTER(EncNal)(); nnal = C.c_uint32(0)
    assert lib.x265amd_encoder_headers(encs[0], C.byref(nal), C.byref(nnal)) > 0
    for i in range(nnal.value):
        header += bytes(nal[i].payload[:nal[i].sizeBytes])
    dt = planes_per_frame[0][0].dtype
    n = len(planes_per_frame)
    outputs = [[] for _ in range(count)]          # per object: (nal bytes, (poc, type, qp, planes)) per coded picture, coding order
    errors = []

    def feeder(r):
        try:
            enc = encs[r]
            nal = C.POINTER(EncNal)(); nnal = C.c_uint32(0)

            def call(pic):
                bufs = [np.zeros((height, width), dt), np.zeros((height // 2, width // 2), dt), np.zeros((height // 2, width // 2), dt)]
                out = EncPicture()
                for k in range(3):
                    out.planes[k] = bufs[k].ctypes.data; out.stride[k] = bufs[k].strides[0]
                ret = lib.x265amd_encoder_encode(enc, C.byref(nal), C.byref(nnal), C.byref(pic) if pic is not None else None, C.byref(out))
                assert ret >= 0, lib.x265amd_last_error()
                if ret:
                    outputs[r].append((b"".join(bytes(nal[i].payload[:nal[i].sizeBytes]) for i in range(nnal.value)), (out.poc, out.sliceType, out.qp, bufs)))
                return ret
            for planes in planes_per_frame:
                pic = EncPicture()
                keep = [np.ascontiguousarray(pl) for pl in planes]
                for k in range(3):
                    pic.planes[k] = keep[k].ctypes.data; pic.stride[k] = keep[k].strides[0]
                call(pic)
            while call(None):
                pass
        except BaseException as exc:        # noqa: B902
            errors.append(("feeder %d" % r, repr(exc)))

    lib.x265amd_encoder_is_referenced.argtypes = [C.c_void_p, C.c_uint64]
    referenced = {}
    flight = {"now": set(), "most": 0}
    lock = threading.Lock()

    def pump(src):
        """the publication stream of object `src` (x265-amod_amd/frame_rows.py: one stream per owner): its pictures in coding order, rows top to bottom; pictures that
        are no references stay where they are"""
        try:
            import time
            rows = lib.x265amd_encoder_ctu_rows(encs[0])
            for k in range(src, n, count):
                while True:
                    rc = lib.x265amd_encoder_is_referenced(encs[src], k)
                    assert rc >= 0, lib.x265amd_last_error()
                    if rc != 2 or errors:
                        break
                    time.sleep(0.0005)
                with lock:
                    referenced[k] = rc == 1
                if rc != 1:
                    continue
                for row in range(rows):
                    d = RowExport()
                    while True:
                        rc = lib.x265amd_encoder_export_row(encs[src], k, row, C.byref(d), 120000)
                        assert rc >= 0, lib.x265amd_last_error()
                        if rc == 0 or errors:
                            break
                        time.sleep(0.0005)
                    if row == 0:
                        with lock:
                            flight["now"].add(k); flight["most"] = max(flight["most"], len(flight["now"]))
                    for r in range(count):
                        while r != src and not errors:
                            rc = lib.x265amd_encoder_import_row(encs[r], C.byref(d))
                            assert rc >= 0, lib.x265amd_last_error()
                            if rc == 0:
                                break
                            time.sleep(0.0005)
                    if errors:
                        return
                with lock:
                    flight["now"].discard(k)
        except BaseException as exc:        # noqa: B902
            errors.append(("pump %d" % src, repr(exc)))

    threads = [threading.Thread(target=feeder, args=(r,)) for r in range(count)] + [threading.Thread(target=pump, args=(r,)) for r in range(count)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(600)
        assert not errors, errors
        assert all(not t.is_alive() for t in threads), "a feeder or the pump did not finish"
    finally:
        if all(not t.is_alive() for t in threads):
            for enc in encs:
                lib.x265amd_encoder_close(enc)
    assert all(len(o) == n for o in outputs), [len(o) for o in outputs]
    stream = bytearray(header)
    coded = []
    for k in range(n):
        nalBytes, rec = outputs[k % count][k]
        stream += nalBytes
        coded.append(rec)
        for r in range(count):
            if r != k % count:
                assert outputs[r][k][0] == b"", "an object emitted NAL units for a picture it does not code"
                assert outputs[r][k][1][:3] == rec[:3], "the picture's order / type / QP differs from the owner's"
                if referenced.get(k):       # a picture nobody references does not travel
                    assert all(np.array_equal(a, b) for a, b in zip(outputs[r][k][1][3], rec[3])), "the imported picture differs from the owner's"
    encoder_run_sharded.most_in_flight = flight["most"]      # pictures whose rows were travelling at the same time (one publication stream per owner)
    return np.frombuffer(bytes(stream), np.uint8), coded


def encoder_api_clip(tag, w, h, nframes, depth=8):
    """display-order (Y, U, V) planes of a w x h clip: a textured picture drifting a few samples per frame plus noise (integer only)"""
    rng = np.random.default_rng(w * 1000003 + h * 1009 + nframes)
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    big = rng.integers(0, pmax + 1, ((h + 96) // 8 + 2, (w + 96) // 8 + 2)).astype(np.int64)
    big = np.kron(big, np.ones((8, 8), np.int64))
    big = (big + np.roll(big, 3, 0) + np.roll(big, 5, 1) + np.roll(big, -2, 1)) // 4
    cb = (np.roll(big, 7, 0)[::2, ::2] + big[1::2, 1::2]) // 2
    cr = (np.roll(big, 11, 1)[::2, ::2] + big[::2, 1::2]) // 2
    frames = []
    for t in range(nframes):
        dx, dy = 2 * ((3 * t) % 11), 2 * ((2 * t) % 7)
        planes = []
        for (src, pw, ph, sx, sy) in ((big, w, h, dx, dy), (cb, w // 2, h // 2, dx // 2, dy // 2), (cr, w // 2, h // 2, dx // 2, dy // 2)):
            o = 16 if src is big else 8
            core = src[o + sy:o + sy + ph, o + sx:o + sx + pw] + rng.integers(-2, 3, (ph, pw)) * (1 << (depth - 8))
            planes.append(np.clip(core, 0, pmax).astype(dt))
        frames.append(planes)
    return frames


def encoder_ft_clip(w, h, nframes, depth=8, dy0=30, dy_inc=20, dx_step=6):
    """display-order (Y, U, V) planes of a clip whose content moves UP faster and faster (by dy0, dy0 + dy_inc, ... luma samples from frame to frame), i.e. motion
    vectors point further and further DOWN into the reference picture: the predictors follow the motion, the search (--merange 57 around the predictor) finds
    it, and beyond 57 samples the reference's frame-parallel rules (search.cpp:92, :1934, :2009, :2763) cut vectors off"""
    rng = np.random.default_rng(w * 7919 + h * 104729 + nframes)
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    pos = [0]
    for t in range(1, nframes):
        pos.append(pos[-1] + dy0 + dy_inc * (t - 1))
    th, tw = h + 64 + pos[-1], w + 64 + dx_step * nframes
    big = rng.integers(0, pmax + 1, (th // 8 + 2, tw // 8 + 2)).astype(np.int64)
    big = np.kron(big, np.ones((8, 8), np.int64))
    big = (big + np.roll(big, 3, 0) + np.roll(big, 5, 1) + np.roll(big, -2, 1)) // 4
    cb = (np.roll(big, 7, 0)[::2, ::2] + big[1::2, 1::2]) // 2
    cr = (np.roll(big, 11, 1)[::2, ::2] + big[::2, 1::2]) // 2
    frames = []
    for t in range(nframes):
        dx, dy = 2 * ((dx_step * t) // 2), 2 * (pos[t] // 2)
        planes = []
        for (src, pw, ph, sx, sy) in ((big, w, h, dx, dy), (cb, w // 2, h // 2, dx // 2, dy // 2), (cr, w // 2, h // 2, dx // 2, dy // 2)):
            o = 16 if src is big else 8
            core = src[o + sy:o + sy + ph, o + sx:o + sx + pw] + rng.integers(-2, 3, (ph, pw)) * (1 << (depth - 8))
            planes.append(np.clip(core, 0, pmax).astype(dt))
        frames.append(planes)
    return frames


# cases of tests/test_encoder_api.py::test_frame_parallel_rules: tag -> ((w, h), frames, depth, clip kind, x265amd_param overrides, reference command line on top of FT_CLI)
FT_CLI = ["--preset", "medium", "--qp", "30", "--aq-mode", "0", "--no-cutree", "--no-weightp", "--no-weightb", "--b-adapt", "0", "--no-scenecut", "--keyint", "250", "--rd", "3",
          "--rdoq-level", "0", "--psy-rdoq", "0", "--ref", "3", "--max-merge", "3", "--no-info", "--no-open-gop", "--rc-lookahead", "5", "--lookahead-slices", "0", "--no-b-pyramid",
          "--frame-threads", "3"]
FT_BASE = dict(fpsNum=30, fpsDenom=1, qp=30, aspectRatioIdc=1, bEnableLoopFilter=1, bEnableSAO=1, bEnableWavefront=1, frameNumThreads=3)
FT_CASES = {
    "ft_p/": ((256, 448), 5, 8, "drift", dict(FT_BASE, bframes=0), ["--bframes", "0", "--sao", "--wpp", "--pools", "4"]),
    "ft_b/": ((256, 448), 8, 8, "drift", dict(FT_BASE, bframes=3), ["--bframes", "3", "--sao", "--wpp", "--pools", "4"]),
    "ft_v/": ((256, 448), 6, 8, "down", dict(FT_BASE, bframes=0), ["--bframes", "0", "--sao", "--wpp", "--pools", "4"]),        # vectors beyond the lag: clipped / left out
    "ft_vb/": ((256, 448), 8, 8, "downb", dict(FT_BASE, bframes=1), ["--bframes", "1", "--sao", "--wpp", "--pools", "4"]),
    "ft_vp/": ((192, 320), 4, 8, "down", dict(FT_BASE, bframes=0, bEnableSAO=0, bEnableWavefront=0), ["--bframes", "0", "--no-sao", "--no-wpp", "--pools", "none"]),
    "ft_nofilter/": ((192, 320), 5, 8, "drift", dict(FT_BASE, bframes=2, bEnableSAO=0, bEnableLoopFilter=0), ["--bframes", "2", "--no-sao", "--no-deblock", "--wpp", "--pools", "4"]),
    "ft_hbd/": ((192, 320), 5, 10, "down", dict(FT_BASE, bframes=0, rdLevel=4, bEnableRectInter=1), ["--bframes", "0", "--sao", "--wpp", "--pools", "4", "--rd", "4", "--rect"]),
}


def encoder_ft_frames(tag):
    (w, h), n, depth, kind, _, _ = FT_CASES[tag]
    if kind == "down":
        return encoder_ft_clip(w, h, n, depth)
    if kind == "downb":
        return encoder_ft_clip(w, h, n, depth, dy0=27, dy_inc=2)
    return encoder_api_clip(tag, w, h, n, depth)


# ---- BASELINE.json's configurations at their stated size (SURVEY.md section 8d's synthetic clip) ----
_LCG_FIELDS = {}


def lcg_noise_field(seed, rows, cols):
    """SURVEY.md section 8d's noise: a 32-bit linear congruential generator x' = 1664525 x + 1013904223 (mod 2^32) started at `seed`, one step per sample in raster order, the
    sample = its state's top 24 bits scaled to -12 .. 12.  Integer arithmetic only -- no library's random stream is involved, every machine gets these bytes.  Computed without
    a loop over the samples by doubling: when the states of samples 0 .. L-1 are known as A[n] seed + C[n], those of L .. 2L-1 follow from the jump by L (aL, cL)."""
    key = (seed & 0xFFFFFFFF, rows, cols)
    if key in _LCG_FIELDS:
        return _LCG_FIELDS[key]
    n = rows * cols
    M = np.uint64(0xFFFFFFFF)
    A = np.ones(1, np.uint64); Cc = np.zeros(1, np.uint64)
    aL, cL = np.uint64(1664525), np.uint64(1013904223)
    while len(A) < n:
        A = np.concatenate([A, (A * aL) & M]); Cc = np.concatenate([Cc, (Cc * aL + cL) & M])
        aL, cL = (aL * aL) & M, (aL * cL + cL) & M
    x = (A[:n] * np.uint64(seed & 0xFFFFFFFF) + Cc[:n]) & M
    field = (((x >> np.uint64(8)) * np.uint64(25)) >> np.uint64(24)).astype(np.int64).reshape(rows, cols) - 12
    if len(_LCG_FIELDS) >= 2:
        _LCG_FIELDS.pop(next(iter(_LCG_FIELDS)))
    _LCG_FIELDS[key] = field
    return field


def survey_clip(w, h, depth, cfg_id, first, count, gop=0):
    """frames first .. first + count - 1 (display order) of the synthetic clip SURVEY.md section 8d prescribes: luma = a smooth 2-D integer gradient shifted by
    (2t, t) samples plus a noise field in [-12, 12] (times 4 for 10-bit samples) that moves with it (motion estimation has real work, every block carries a
    residual), chroma = low-frequency integer ramps shifted by (t, t / 2); the noise field is re-seeded every 24th frame (a scene change).  Integer arithmetic
    only, and frame t depends on t alone, so every machine and every rank sees the same pictures.  gop: the closed GOP a rank codes in a multi-GPU run (its own
    noise field behind its IDR picture).  For (1920, 1080, 8, cfg_id 2) these are the frames of bench.py since round 2."""
    def tri(a, period):
        a = a % period
        return np.minimum(a, period - a)
    sc = 1 << (depth - 8)
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    frames = []
    for t in range(first, first + count):
        epoch = t // 24
        noise = lcg_noise_field(0x9E3779B9 ^ (cfg_id << 8) ^ (epoch << 20) ^ (gop << 12), h + 64, w + 128)     # indexed by the moving coordinates
        tt = t % 24
        v = np.arange(h, dtype=np.int64)[:, None] + tt + 24 * epoch
        u = np.arange(w, dtype=np.int64)[None, :] + 2 * tt + 48 * epoch
        luma = 60 + (tri(u, 512) * 96) // 256 + (tri(v, 384) * 64) // 192 + noise[tt:tt + h, 2 * tt:2 * tt + w]
        vc = np.arange(h // 2, dtype=np.int64)[:, None] + t // 2
        uc = np.arange(w // 2, dtype=np.int64)[None, :] + t
        cb = 96 + (tri(uc, 640) * 64) // 320 + (tri(vc, 448) * 16) // 224
        cr = 160 - (tri(uc + 200, 720) * 48) // 360 + (tri(vc + 100, 512) * 16) // 256
        frames.append([np.clip(luma * sc, 0, pmax).astype(dt), np.clip(cb * sc, 0, pmax).astype(dt), np.clip(cr * sc, 0, pmax).astype(dt)])
    return frames


# The reference command line of the full-size cases: the preset in CQP as it comes -- adaptive GOPs (trellis), scene-cut detection, open GOPs, B pyramid, lookahead slices,
# weighted prediction's analysis, the frame threads the reference picks for the machine (three here: frame-parallel rules).  --no-info leaves out the SEI NAL unit with
# the reference build's version and option string.
FULL_CLI = ["--qp", "30", "--no-info"]
# what `--preset medium --qp 30` sets (source/common/param.cpp:140-330: x265_param_default; CQP switches AQ and cutree off, encoder.cpp), as x265amd_param fields
FULL_BASE = dict(fpsNum=30, fpsDenom=1, qp=30, aspectRatioIdc=1, bEnableLoopFilter=1, bEnableSAO=1, bEnableWavefront=1, frameNumThreads=3, bframes=4,
                 scenecutThreshold=40, lookaheadDepth=20, bFrameAdaptive=2, bOpenGOP=1, bBPyramid=1, lookaheadSlices=8, bEnableWeightedPred=1)
# --preset slow on top of it (param.cpp:500-514)
SLOW_TOOLS = dict(bEnableEarlySkip=0, bIntraInBFrames=0, bEnableRectInter=1, rdLevel=4, rdoqLevel=2, psyRdoqFix8=256, subpelRefine=3, searchMethod=3, maxNumReferences=4, limitModes=1,
                  lookaheadDepth=25, lookaheadSlices=4)
VERYSLOW_TOOLS = dict(bEnableEarlySkip=0, bEnableAMP=1, bEnableRectInter=1, tuQTMaxInterDepth=3, tuQTMaxIntraDepth=3, rdLevel=6, rdoqLevel=2, psyRdoqFix8=256, subpelRefine=4,
                      maxNumMergeCand=5, searchMethod=3, maxNumReferences=5, limitReferences=0, limitModes=0)
# --preset veryslow's GOP side on top of FULL_BASE (param.cpp:536-556): eight B frames, forty pictures of lookahead, no lookahead slices, weighted bi-prediction
VERYSLOW_GOP = dict(bframes=8, lookaheadDepth=40, lookaheadSlices=0, bEnableWeightedBiPred=1)
# tag -> ((w, h), frames, depth, cfg_id of the clip, x265amd_param fields, the reference's command line in front of FULL_CLI)
FULL_CASES = {
    "cfg3_2160p_slow/": ((3840, 2160), 12, 8, 3, dict(FULL_BASE, **SLOW_TOOLS), ["--preset", "slow"]),                   # BASELINE.json configs[2]: I + two mini-GOPs of the trellis
    "cfg4_2160p_main10/": ((3840, 2160), 12, 10, 4, dict(FULL_BASE), ["--preset", "medium"]),                             # configs[3]: Main 10 over a full B pyramid and more
    # configs[4] as it comes (round 5: --weightb is coded, nothing is switched off): plain --preset veryslow --rd 6 --qp 30 --no-info
    "cfg5_4320p_veryslow_rd6/": ((7680, 4320), 3, 10, 5, dict(FULL_BASE, **VERYSLOW_TOOLS, **VERYSLOW_GOP), ["--preset", "veryslow", "--rd", "6"]),
    # rd 2 on a picture of 1080 rows: Analysis::complexityCheckCU is active (analysis.cpp:3536-3559, only for pictures of at least 1080 rows at rd 0-2)
    "fhd_rd2/": ((1920, 1080), 3, 8, 2, dict(FULL_BASE, rdLevel=2, bframes=1), ["--preset", "medium", "--rd", "2", "--bframes", "1"]),
    # the bench's configuration over sixty frames: both re-seeds of the clip (frames 24 and 48: scene cuts, I pictures inside open GOPs) and ten mini-GOPs of the trellis
    "fhd_medium_60/": ((1920, 1080), 60, 8, 2, dict(FULL_BASE), ["--preset", "medium"]),
}


def torture_clip(kind, w, h, depth, n):
    """content the survey clip does not have (integer arithmetic only): `noise` -- every sample uniform over the whole range, new every picture (nothing predicts, escapes and
    large levels everywhere); `flat` -- black, then white, then mid grey pictures with one moving square; `edges` -- a high-contrast checkerboard of 8x8 and 3x3 cells sliding
    by (3, 1) with saturated samples; `static` -- one textured picture repeated (everything skips); `jump` -- texture moving 72 samples per picture (beyond the search range);
    `dark` -- a dim noisy gradient (adaptive quantisation's dark-scene bias, low variances)"""
    sc = 1 << (depth - 8)
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    frames = []
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    cy, cx = np.mgrid[0:h // 2, 0:w // 2].astype(np.int64)
    for t in range(n):
        if kind == "noise":
            f = lcg_noise_field(0xC0FFEE + 977 * t, h + h // 2, w)
            x = lcg_noise_field(0xBADF00D + 131 * t, h + h // 2, w)
            full = ((f + 12) * 25 + (x + 12)) % 256                      # 0 .. 255 from two draws of 0 .. 24
            y = full[:h]; u = full[h:h + h // 2, :w // 2]; v = full[h:h + h // 2, w // 2:]
        elif kind == "flat":
            base = (0, 255, 128)[(t // 3) % 3]
            y = np.full((h, w), base, np.int64); u = np.full((h // 2, w // 2), 128, np.int64); v = u.copy()
            y[40 + 3 * t:72 + 3 * t, 60 + 5 * t:92 + 5 * t] = 255 - base
        elif kind == "edges":
            a = (((xx + 3 * t) // 8 + (yy + t) // 8) & 1) * 255
            b = (((xx + 3 * t) // 3 + (yy + t) // 3) & 1) * 255
            y = np.where((yy // 48) & 1, b, a)
            u = 128 + (((cx + t) // 16) & 1) * 90 - 45; v = 128 - (((cy + t) // 12) & 1) * 100 + 50
        elif kind == "static":
            y = 40 + ((xx * 7 + yy * 13) % 97) + lcg_noise_field(0x5747, h, w); u = 100 + (cx % 31); v = 150 - (cy % 29)
        elif kind == "jump":
            y = 50 + (((xx + 72 * t) * 5 + yy * 3) % 131) + lcg_noise_field(0x4A554D50, h, w + 72 * n)[:, 72 * t:72 * t + w]; u = 110 + ((cx + 36 * t) % 23); v = 140 - ((cy + 5 * t) % 19)
        elif kind == "dark":
            y = 4 + (xx + 2 * t) // 40 + (lcg_noise_field(0xDA4C + t // 24, h + 32, w + 64)[t % 24:t % 24 + h, 2 * (t % 24):2 * (t % 24) + w] + 12) // 8; u = 128 + (cx // 64); v = 128 - (cy // 64)
        else:
            raise ValueError(kind)
        frames.append([np.clip(np.asarray(p, np.int64) * sc, 0, pmax).astype(dt) for p in (y, u, v)])
    return frames


def full_case_frames(tag):
    (w, h), n, depth, cfg_id, extra, _ = (FULL_CASES[tag] if tag in FULL_CASES else PRESET_CASES[tag] if tag in PRESET_CASES else RC_CASES[tag] if tag in RC_CASES else CLI_CASES[tag])
    if tag in CLI_CASES and isinstance(extra, dict) and "clip" in extra:
        return torture_clip(extra["clip"], w, h, depth, n)
    return survey_clip(w, h, depth, cfg_id, 0, n)


# ---- the presets AS THEY COME (round 6): no --qp on the reference's command line, i.e. rc.rateControlMode = X265_RC_CRF with rfConstant 28, aq-mode 2, cuTree
# (source/common/param.cpp:266-290) -- BASELINE.json's metric is quoted on exactly this.  PRESET_CLI is everything behind the preset's name. ----
PRESET_CLI = ["--no-info"]
PRESET_RC = dict(rateControlMode=2, rfConstant=28.0, aqMode=2, aqStrength=1.0, cuTree=1, qCompress=0.6, qgSize=32)
PRESET_BASE = dict({k: v for k, v in FULL_BASE.items() if k != "qp"}, **PRESET_RC)
PRESET_CASES = {
    "crf_wqvga_medium_30/": ((416, 240), 30, 8, 2, dict(PRESET_BASE), ["--preset", "medium"]),                       # cut CTUs right and below, a scene change at 24
    "crf_fhd_medium_60/": ((1920, 1080), 60, 8, 2, dict(PRESET_BASE), ["--preset", "medium"]),                      # BASELINE.json configs[1] / the metric's first size
    "crf_2160p_medium_20/": ((3840, 2160), 20, 8, 2, dict(PRESET_BASE), ["--preset", "medium"]),                    # the metric's second size
    "crf_cfg3_2160p_slow/": ((3840, 2160), 26, 8, 3, dict(PRESET_BASE, **SLOW_TOOLS), ["--preset", "slow"]),        # configs[2]: over the clip's re-seed at 24 (a scene cut)
    "crf_cfg4_2160p_main10/": ((3840, 2160), 26, 10, 4, dict(PRESET_BASE), ["--preset", "medium"]),                  # configs[3]
    # configs[4]: ten pictures -- the I picture and a whole mini-GOP of eight B pictures with its pyramid (--preset veryslow: bframes 8, --weightb)
    "crf_cfg5_4320p_veryslow_rd6/": ((7680, 4320), 10, 10, 5, dict(PRESET_BASE, **VERYSLOW_TOOLS, **VERYSLOW_GOP), ["--preset", "veryslow", "--rd", "6"]),
}


# ---- scene-cut detection of the lookahead (x265amd_param.scenecutThreshold): clips whose content changes at given frames ----
def scene_clip(w, h, nframes, cuts, depth=8):
    """display-order (Y, U, V) planes: smooth integer gradients plus a noise field that moves with them (2 samples right, 1 down per frame); from every frame number
    in `cuts` on the gradients take other periods / phases and the noise field is a new one -- what the lookahead's cost estimates see as a scene change"""
    def tri(a, period):
        a = a % period
        return np.minimum(a, period - a)
    sc8 = 1 << (depth - 8)
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    frames = []
    for t in range(nframes):
        scene = sum(1 for c in cuts if t >= c)
        noise = np.random.default_rng(w * 1000003 + h * 1009 + 7919 * scene).integers(-10, 11, (h + 64, w + 128))
        px, py = 160 + 96 * (scene % 3), 128 + 64 * ((scene + 1) % 3)
        v = np.arange(h, dtype=np.int64)[:, None] + t + 37 * scene
        u = np.arange(w, dtype=np.int64)[None, :] + 2 * t + 91 * scene
        luma = 50 + 40 * (scene % 2) + (tri(u, px) * 90) // (px // 2) + (tri(v, py) * 60) // (py // 2) + noise[t:t + h, 2 * t:2 * t + w]
        vc = np.arange(h // 2, dtype=np.int64)[:, None] + t // 2
        uc = np.arange(w // 2, dtype=np.int64)[None, :] + t
        cb = 96 + 20 * (scene % 2) + (tri(uc, 320) * 48) // 160 + (tri(vc, 224) * 16) // 112
        cr = 150 - 25 * (scene % 2) - (tri(uc + 100, 360) * 40) // 180 + (tri(vc + 50, 256) * 16) // 128
        frames.append([np.clip(luma * sc8, 0, pmax).astype(dt), np.clip(cb * sc8, 0, pmax).astype(dt), np.clip(cr * sc8, 0, pmax).astype(dt)])
    return frames


SC_CLI = ["--preset", "medium", "--qp", "30", "--aq-mode", "0", "--no-cutree", "--no-weightp", "--no-weightb", "--b-adapt", "0", "--scenecut", "40", "--keyint", "250", "--rd", "3",
          "--rdoq-level", "0", "--psy-rdoq", "0", "--ref", "3", "--max-merge", "3", "--no-info", "--no-open-gop", "--lookahead-slices", "0", "--no-b-pyramid", "--sao", "--wpp",
          "--pools", "4", "--frame-threads", "3"]
SC_BASE = dict(fpsNum=30, fpsDenom=1, qp=30, aspectRatioIdc=1, bEnableLoopFilter=1, bEnableSAO=1, bEnableWavefront=1, frameNumThreads=3, scenecutThreshold=40)
# tag -> ((w, h), frames, depth, scene changes, x265amd_param fields, the reference's command line behind SC_CLI)
SC_CASES = {
    "sc_i/": ((320, 192), 16, 8, [7], dict(SC_BASE, bframes=4, lookaheadDepth=5), ["--bframes", "4", "--rc-lookahead", "5"]),                    # a cut inside a mini-GOP: non-IDR I picture (min-keyint not reached)
    "sc_idr/": ((320, 192), 16, 8, [6, 12], dict(SC_BASE, bframes=3, lookaheadDepth=8, keyframeMin=4), ["--bframes", "3", "--rc-lookahead", "8", "--min-keyint", "4"]),
    "sc_p/": ((320, 192), 14, 8, [5], dict(SC_BASE, bframes=0, lookaheadDepth=4), ["--bframes", "0", "--rc-lookahead", "4"]),
    "sc_none/": ((320, 192), 12, 8, [], dict(SC_BASE, bframes=4, lookaheadDepth=20), ["--bframes", "4", "--rc-lookahead", "20"]),                 # no cut: the decision must not invent one
    "sc_hbd/": ((320, 192), 12, 10, [5], dict(SC_BASE, bframes=2, lookaheadDepth=5), ["--bframes", "2", "--rc-lookahead", "5"]),
    "sc_flash/": ((320, 192), 16, 8, [6, 7], dict(SC_BASE, bframes=4, lookaheadDepth=10), ["--bframes", "4", "--rc-lookahead", "10"]),            # a one-frame flash
}


def stream_diff(got, want):
    """where two Annex-B streams part: '' when equal, else the NAL (index, type, size) and the byte inside it"""
    got, want = bytes(bytearray(got)), bytes(bytearray(want))
    if got == want:
        return ""
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    starts, i = [], 0
    while True:
        i = want.find(b"\x00\x00\x01", i)
        if i < 0:
            break
        starts.append(i + 3); i += 3
    k = max([j for j, s_ in enumerate(starts) if s_ <= at] or [0])
    end = (starts[k + 1] - 3) if k + 1 < len(starts) else len(want)
    return "lengths %d / %d; first difference at byte %d: NAL %d of %d (type %d, %d bytes), byte %d of it: got %s want %s" % (
        len(got), len(want), at, k, len(starts), (want[starts[k]] >> 1) & 63, end - starts[k], at - starts[k], got[at:at + 8].hex(), want[at:at + 8].hex())


# --b-adapt 2 (the trellis): tag -> ((w, h), frames, depth, clip, x265amd_param fields, the reference's options on top of BA_CLI)
BA_CLI = [o if o != "0" or SC_CLI[i - 1] != "--b-adapt" else "2" for i, o in enumerate(SC_CLI)]
BA_BASE = dict(SC_BASE, bFrameAdaptive=2)
BA_CASES = {
    "ba2_drift/": ((320, 192), 20, 8, ("api", None), dict(BA_BASE, bframes=4, lookaheadDepth=10), ["--bframes", "4", "--rc-lookahead", "10"]),            # textured picture drifting: B pictures pay
    "ba2_cut/": ((320, 192), 18, 8, ("scene", [9]), dict(BA_BASE, bframes=3, lookaheadDepth=8), ["--bframes", "3", "--rc-lookahead", "8"]),                # a scene cut inside
    "ba2_nosc/": ((320, 192), 14, 8, ("ft", None), dict(BA_BASE, bframes=4, lookaheadDepth=6, scenecutThreshold=0), ["--bframes", "4", "--rc-lookahead", "6", "--no-scenecut"]),   # accelerating motion, no scene-cut detection
    "ba2_hbd/": ((256, 192), 12, 10, ("api", None), dict(BA_BASE, bframes=2, lookaheadDepth=5), ["--bframes", "2", "--rc-lookahead", "5"]),
}


# --open-gop (the reference's default): tag -> ((w, h), frames, depth, clip, x265amd_param fields, the reference's options on top of OG_CLI)
OG_CLI = [o for o in BA_CLI if o != "--no-open-gop"] + ["--open-gop"]
OG_BASE = dict(BA_BASE, bOpenGOP=1)
OG_CASES = {
    "og_cut/": ((320, 192), 18, 8, ("scene", [6, 12]), dict(OG_BASE, bframes=3, lookaheadDepth=8, keyframeMin=4), ["--bframes", "3", "--rc-lookahead", "8", "--min-keyint", "4"]),     # scene cuts: CRA pictures
    "og_keyint/": ((320, 192), 20, 8, ("api", None), dict(OG_BASE, bframes=3, lookaheadDepth=5, keyframeMax=7, keyframeMin=7, bFrameAdaptive=0, scenecutThreshold=0),
                   ["--bframes", "3", "--rc-lookahead", "5", "--keyint", "7", "--min-keyint", "7", "--b-adapt", "0", "--no-scenecut"]),     # fixed mini-GOPs: B pictures in front of every keyframe (RASL)
    "og_keyint_ba/": ((320, 192), 22, 8, ("api", None), dict(OG_BASE, bframes=4, lookaheadDepth=10, keyframeMax=9, keyframeMin=2), ["--bframes", "4", "--rc-lookahead", "10", "--keyint", "9", "--min-keyint", "2"]),   # the trellis across keyframes
    "og_hbd/": ((256, 192), 14, 10, ("ft", None), dict(OG_BASE, bframes=2, lookaheadDepth=5, keyframeMax=6, keyframeMin=3), ["--bframes", "2", "--rc-lookahead", "5", "--keyint", "6", "--min-keyint", "3"]),
}


def og_case_frames(tag):
    (w, h), n, depth, (kind, arg), _, _ = OG_CASES[tag]
    if kind == "scene":
        return scene_clip(w, h, n, arg, depth)
    if kind == "ft":
        return encoder_ft_clip(w, h, n, depth, dy0=2, dy_inc=2, dx_step=4)
    return encoder_api_clip(tag, w, h, n, depth)


# --b-pyramid (the reference's default): tag -> ((w, h), frames, depth, clip, x265amd_param fields, the reference's options on top of BP_CLI)
BP_CLI = [o for o in BA_CLI if o != "--no-b-pyramid"] + ["--b-pyramid"]
BP_BASE = dict(BA_BASE, bBPyramid=1)
BP_CASES = {
    "bp_fixed/": ((320, 192), 15, 8, ("api", None), dict(BP_BASE, bframes=3, lookaheadDepth=5, bFrameAdaptive=0, scenecutThreshold=0), ["--bframes", "3", "--rc-lookahead", "5", "--b-adapt", "0", "--no-scenecut"]),
    "bp_ba2/": ((320, 192), 20, 8, ("api", None), dict(BP_BASE, bframes=4, lookaheadDepth=10), ["--bframes", "4", "--rc-lookahead", "10"]),           # the trellis prices the pyramid
    "bp_og_cut/": ((320, 192), 18, 8, ("scene", [9]), dict(BP_BASE, bframes=3, lookaheadDepth=8, bOpenGOP=1, keyframeMax=14, keyframeMin=2),
                   ["--bframes", "3", "--rc-lookahead", "8", "--open-gop", "--keyint", "14", "--min-keyint", "2"]),     # with open GOPs: a scene cut and an interval keyframe
    "bp_ft/": ((320, 192), 26, 8, ("ft", None), dict(BP_BASE, bframes=4, lookaheadDepth=10), ["--bframes", "4", "--rc-lookahead", "10"]),            # accelerating motion: mini-GOPs of varying length over several windows
    "bp_deep/": ((320, 192), 30, 8, ("scene", [17]), dict(BP_BASE, bframes=6, lookaheadDepth=15, maxNumReferences=4, bOpenGOP=1), ["--bframes", "6", "--rc-lookahead", "15", "--ref", "4", "--open-gop"]),
    "bp_hbd/": ((256, 192), 12, 10, ("ft", None), dict(BP_BASE, bframes=3, lookaheadDepth=5, bFrameAdaptive=0), ["--bframes", "3", "--rc-lookahead", "5", "--b-adapt", "0"]),
}


def bp_case_frames(tag):
    (w, h), n, depth, (kind, arg), _, _ = BP_CASES[tag]
    if kind == "scene":
        return scene_clip(w, h, n, arg, depth)
    if kind == "ft":
        return encoder_ft_clip(w, h, n, depth, dy0=2, dy_inc=2, dx_step=4)
    return encoder_api_clip(tag, w, h, n, depth)


# --lookahead-slices (the reference's default 8; only from 720 lines up): tag -> ((w, h), frames, depth, clip, x265amd_param fields, the reference's options on top of LS_CLI)
LS_CLI = [o for i, o in enumerate(BA_CLI) if o not in ("--lookahead-slices", "--no-open-gop", "--no-b-pyramid") and BA_CLI[i - 1] != "--lookahead-slices"] + ["--open-gop", "--b-pyramid"]
LS_BASE = dict(BA_BASE, bOpenGOP=1, bBPyramid=1)
LS_CASES = {
    # the preset's GOP structure as it comes: --b-adapt 2, --bframes 4, B pyramid, open GOPs, scene-cut detection, --lookahead-slices 8 (1280x720: 45 block rows, 4 slices of 11)
    "ls_medium/": ((1280, 720), 14, 8, ("ft", None), dict(LS_BASE, bframes=4, lookaheadDepth=8, lookaheadSlices=8), ["--bframes", "4", "--rc-lookahead", "8", "--lookahead-slices", "8"]),
    "ls_sc/": ((1280, 720), 12, 8, ("ft_cut", 7), dict(LS_BASE, bframes=3, lookaheadDepth=6, lookaheadSlices=3, bFrameAdaptive=0, bBPyramid=0),
               ["--bframes", "3", "--rc-lookahead", "6", "--lookahead-slices", "3", "--b-adapt", "0", "--no-b-pyramid"]),          # fixed mini-GOPs: every estimate is the scene-cut check's, all in slices (3 of 15 rows)
}


def ls_case_frames(tag):
    (w, h), n, depth, (kind, arg), _, _ = LS_CASES[tag]
    if kind == "survey_cut":        # the noise field changes and the picture jumps at frame `arg`
        return survey_clip(w, h, depth, 2, 0, arg, 0) + survey_clip(w, h, depth, 2, 40, n - arg, 3)
    if kind == "ft_cut":            # accelerating motion, then another scene
        return encoder_ft_clip(w, h, arg, depth, dy0=2, dy_inc=2, dx_step=4) + survey_clip(w, h, depth, 2, 40, n - arg, 3)
    if kind == "ft":
        return encoder_ft_clip(w, h, n, depth, dy0=2, dy_inc=2, dx_step=4)
    return survey_clip(w, h, depth, 2, 0, n, 0)


# Command lines as a user of the reference types them, through the command line program alone (x265-amod_amd/bin/x265amd -> the library's x265_api table -> its preset tables and
# x265_param_parse): tag -> ((w, h), frames, depth, cfg_id of the clip, unused, the reference's options).  `--no-info` is added on both sides.  Golden data:
# tests/golden/make_golden.py cli -> encoder_cli_golden.json.  What encoder_open refuses is listed in CLI_REFUSED with the words its error must contain.
CLI_CASES = {
    "cli_veryfast/": ((416, 240), 20, 8, 2, {}, ["--preset", "veryfast"]),
    "cli_faster/": ((416, 240), 20, 8, 2, {}, ["--preset", "faster"]),
    "cli_fast/": ((416, 240), 20, 8, 2, {}, ["--preset", "fast"]),
    "cli_veryslow/": ((416, 240), 14, 8, 2, {}, ["--preset", "veryslow"]),
    "cli_odd_size/": ((424, 232), 20, 8, 2, {}, ["--preset", "medium"]),                        # not a multiple of 16: partial AQ blocks, a lowres picture of odd block counts
    "cli_rect_amp/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--rect", "--amp"]),
    "cli_crf12/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--crf", "12"]),
    "cli_all_intra/": ((416, 240), 8, 8, 2, {}, ["--preset", "medium", "--keyint", "1"]),
    "cli_badapt1_b6/": ((416, 240), 24, 8, 2, {}, ["--preset", "medium", "--b-adapt", "1", "--bframes", "6"]),
    "cli_nowpp_ft2/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--no-wpp", "--frame-threads", "2"]),
    "cli_weightb/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--weightb"]),
    "cli_ref1/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--ref", "1"]),
    # frame rates: the rate factor's base, cuTree's strength and the lookahead's frame durations all hang on fps (the clip's file says 30)
    "cli_fps_ntsc_film/": ((416, 240), 20, 8, 2, {}, ["--preset", "medium", "--fps", "24000/1001"]),
    "cli_fps60/": ((416, 240), 20, 8, 2, {}, ["--preset", "medium", "--fps", "60"]),
    "cli_fps12_5_slow/": ((416, 240), 14, 8, 2, {}, ["--preset", "slow", "--fps", "12.5"]),
    # small pictures (the reference's input readers take nothing below 64x64; a picture of ONE CTU is refused: CLI_REFUSED): two by one CTUs with a partial column and row
    # (a picture of one CTU row or fewer than three CTU columns is coded without wavefronts, and without them the frame threads are half the rows: encoder.cpp:249-254)
    # (presets with options on top)
    "cli_veryfast_crf20_hbd/": ((416, 240), 16, 10, 4, {}, ["--preset", "veryfast", "--crf", "20"]),
    "cli_veryslow_b3/": ((416, 240), 12, 8, 2, {}, ["--preset", "veryslow", "--bframes", "3"]),
    "cli_fast_fastdecode/": ((416, 240), 16, 8, 2, {}, ["--preset", "fast", "--tune", "fastdecode"]),
    "cli_faster_nofilters/": ((416, 240), 16, 8, 2, {}, ["--preset", "faster", "--no-sao", "--no-deblock"]),
    "cli_slow_rd6/": ((416, 240), 10, 8, 2, {}, ["--preset", "slow", "--rd", "6"]),
    "cli_tu3_limit4/": ((416, 240), 12, 8, 2, {}, ["--preset", "medium", "--tu-inter-depth", "3", "--tu-intra-depth", "3", "--limit-tu", "4"]),
    "cli_weightb_b8/": ((416, 240), 24, 8, 2, {}, ["--preset", "medium", "--weightb", "--bframes", "8"]),
    "cli_slower_psnr_hbd/": ((416, 240), 10, 10, 4, {}, ["--preset", "slower", "--tune", "psnr"]),
    "cli_medium_720p_ft2/": ((1280, 720), 10, 8, 2, {}, ["--preset", "medium", "--frame-threads", "2"]),
    "cli_fast_1366x768/": ((1366, 768), 6, 8, 2, {}, ["--preset", "fast"]),
    # (more lines a user types)
    "cli_keyint_inf/": ((416, 240), 20, 8, 2, {}, ["--preset", "medium", "--keyint", "-1"]),
    "cli_bframes0/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--bframes", "0"]),
    "cli_bframes1_badapt0/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--bframes", "1", "--b-adapt", "0"]),
    "cli_rclookahead3/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--rc-lookahead", "3", "--bframes", "2"]),
    "cli_laslices0/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--lookahead-slices", "0"]),
    "cli_scenecut80/": ((416, 240), 30, 8, 2, {}, ["--preset", "medium", "--scenecut", "80"]),
    "cli_crf28_5/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--crf", "28.5"]),
    "cli_crf1/": ((416, 240), 10, 8, 2, {}, ["--preset", "medium", "--crf", "1"]),
    "cli_merange16_ref6/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--merange", "16", "--ref", "6"]),
    "cli_maxmerge5/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--max-merge", "5"]),
    "cli_nopsy/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--psy-rd", "0", "--psy-rdoq", "0"]),
    "cli_nowpp/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--no-wpp"]),
    "cli_nowpp_ft1/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--no-wpp", "--frame-threads", "1"]),
    "cli_128x128/": ((128, 128), 12, 8, 2, {}, ["--preset", "medium"]),
    "cli_128x256/": ((128, 256), 12, 8, 2, {}, ["--preset", "medium"]),
    "cli_256x64/": ((256, 64), 12, 8, 2, {}, ["--preset", "medium"]),
    "cli_136x72_hbd/": ((136, 72), 12, 10, 4, {}, ["--preset", "medium"]),
    # sizes that are no multiple of the smallest CU: coded padded, the SPS's conformance window takes the pad off (and the reconstruction handed out is the window's)
    "cli_w420_h236/": ((420, 236), 16, 8, 2, {}, ["--preset", "medium"]),
    "cli_w418_h238_hbd/": ((418, 238), 12, 10, 4, {}, ["--preset", "slow"]),
    "cli_w854_h480/": ((854, 480), 10, 8, 2, {}, ["--preset", "fast"]),
    # (the options the parser knows and no case had walked through the preset's rate control yet)
    "cli_b_intra/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--b-intra"]),
    "cli_fast_intra/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--fast-intra"]),
    "cli_qpstep2/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--qpstep", "2"]),
    "cli_no_weightp/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--no-weightp"]),
    "cli_slow_b_intra_hbd/": ((416, 240), 12, 10, 4, {}, ["--preset", "slow", "--b-intra", "--fast-intra"]),
    "cli_hbd_ssim/": ((416, 240), 16, 10, 4, {}, ["--preset", "medium", "--tune", "ssim"]),
    "cli_star_subme4/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--me", "star", "--subme", "4", "--merange", "25"]),
    "cli_rdoq2/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--rdoq-level", "2", "--psy-rdoq", "1.0"]),
    "cli_keyint10/": ((416, 240), 26, 8, 2, {}, ["--preset", "medium", "--no-scenecut", "--keyint", "10"]),
    "cli_qpmax30/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--qpmax", "30"]),
    "cli_ratios/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--ipratio", "1.2", "--pbratio", "1.5"]),
    "cli_slow_fastdecode/": ((416, 240), 16, 8, 2, {}, ["--preset", "slow", "--tune", "fastdecode"]),
    "cli_hbd_aq3/": ((416, 240), 16, 10, 4, {}, ["--preset", "medium", "--aq-mode", "3"]),
    "cli_repeat_headers/": ((416, 240), 26, 8, 2, {}, ["--preset", "medium", "--repeat-headers", "--keyint", "10", "--no-scenecut"]),
    "cli_zerolatency/": ((416, 240), 20, 8, 2, {}, ["--preset", "medium", "--tune", "zerolatency"]),
    "cli_fast_psnr/": ((416, 240), 20, 8, 2, {}, ["--preset", "fast", "--tune", "psnr"]),
    "cli_closed_fixed/": ((416, 240), 26, 8, 2, {}, ["--preset", "medium", "--no-open-gop", "--bframes", "3", "--b-adapt", "0", "--no-b-pyramid", "--keyint", "15", "--min-keyint", "15"]),
    "cli_no_filters/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--no-sao", "--no-deblock"]),
    "cli_no_tools/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--no-signhide", "--no-strong-intra-smoothing", "--no-temporal-mvp", "--no-early-skip", "--rskip", "0"]),
    "cli_tu2_rd4/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--max-merge", "5", "--tu-intra-depth", "2", "--tu-inter-depth", "2", "--rd", "4"]),
    "cli_ref4_nolimit/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--limit-refs", "0", "--ref", "4"]),
    "cli_qg64_crf33/": ((448, 256), 16, 8, 2, {}, ["--preset", "medium", "--qg-size", "64", "--crf", "33"]),
    "cli_hbd_fast/": ((416, 240), 16, 10, 4, {}, ["--preset", "fast"]),
    "cli_qpmin20/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--crf", "14", "--qpmin", "20"]),
    "cli_ft1/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--frame-threads", "1"]),
    "cli_la40_b8/": ((416, 240), 30, 8, 2, {}, ["--preset", "medium", "--rc-lookahead", "40", "--bframes", "8"]),
    "cli_aq1_nocutree/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--no-cutree", "--aq-mode", "1", "--aq-strength", "0.5"]),
    "cli_qp_const/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--qp", "27"]),
    "cli_720p_medium/": ((1280, 720), 16, 8, 2, {}, ["--preset", "medium"]),                     # the lookahead's cooperative slices under the rate control
    "cli_720p_fast_noslices/": ((1280, 720), 12, 8, 2, {}, ["--preset", "fast", "--lookahead-slices", "0"]),
    "cli_480p_slow/": ((832, 480), 12, 8, 3, {}, ["--preset", "slow"]),
    "cli_hbd_veryslow/": ((416, 240), 10, 10, 5, {}, ["--preset", "veryslow"]),
    "cli_crf4/": ((416, 240), 12, 8, 2, {}, ["--preset", "medium", "--crf", "4"]),
    "cli_crf51/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--crf", "51"]),
    "cli_keyint2/": ((416, 240), 12, 8, 2, {}, ["--preset", "medium", "--keyint", "2", "--min-keyint", "1"]),
    "cli_b16/": ((416, 240), 40, 8, 2, {}, ["--preset", "medium", "--bframes", "16", "--rc-lookahead", "40"]),
    "cli_b1_nopyr/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--bframes", "1", "--no-b-pyramid"]),
    "cli_dia_subme0/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--me", "dia", "--subme", "0", "--merange", "8"]),
    "cli_subme7/": ((416, 240), 12, 8, 2, {}, ["--preset", "medium", "--subme", "7"]),
    "cli_rd6/": ((416, 240), 10, 8, 2, {}, ["--preset", "medium", "--rd", "6"]),
    "cli_rd5_rdoq1/": ((416, 240), 10, 8, 2, {}, ["--preset", "medium", "--rd", "5", "--rdoq-level", "1"]),
    "cli_nopsy_rdoq2/": ((416, 240), 12, 8, 2, {}, ["--preset", "medium", "--psy-rd", "0", "--psy-rdoq", "0", "--rdoq-level", "2"]),
    "cli_rect_limit/": ((416, 240), 12, 8, 2, {}, ["--preset", "medium", "--rect", "--limit-modes"]),
    "cli_tu4/": ((416, 240), 10, 8, 2, {}, ["--preset", "medium", "--tu-intra-depth", "4", "--tu-inter-depth", "4"]),
    "cli_sar2/": ((416, 240), 8, 8, 2, {}, ["--preset", "medium", "--sar", "2"]),
    "cli_pools_none/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--pools", "none"]),
    "cli_ft4/": ((416, 240), 20, 8, 2, {}, ["--preset", "medium", "--frame-threads", "4"]),
    "cli_aq_strong/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--aq-strength", "3.0"]),
    "cli_qcomp1/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--qcomp", "1.0"]),
    "cli_qcomp05_nocutree/": ((416, 240), 16, 8, 2, {}, ["--preset", "medium", "--qcomp", "0.5", "--no-cutree"]),
    "cli_slow_norect/": ((416, 240), 12, 8, 2, {}, ["--preset", "slow", "--no-rect", "--no-limit-modes"]),
    "cli_hbd_slow_crf20/": ((416, 240), 10, 10, 4, {}, ["--preset", "slow", "--crf", "20"]),
    # other content (torture_clip): nothing predictable, flat pictures, sharp edges with saturated samples, a still picture, motion beyond the search range, a dark scene
    "cli_noise_medium/": ((416, 240), 8, 8, 2, {"clip": "noise"}, ["--preset", "medium"]),
    "cli_noise_slow_hbd/": ((416, 240), 6, 10, 4, {"clip": "noise"}, ["--preset", "slow"]),
    "cli_noise_crf45/": ((416, 240), 8, 8, 2, {"clip": "noise"}, ["--preset", "medium", "--crf", "45"]),
    "cli_flat_medium/": ((416, 240), 12, 8, 2, {"clip": "flat"}, ["--preset", "medium"]),
    "cli_flat_veryslow/": ((416, 240), 10, 8, 2, {"clip": "flat"}, ["--preset", "veryslow"]),
    "cli_edges_medium/": ((416, 240), 12, 8, 2, {"clip": "edges"}, ["--preset", "medium"]),
    "cli_edges_slow/": ((416, 240), 10, 8, 2, {"clip": "edges"}, ["--preset", "slow"]),
    "cli_edges_hbd_fast/": ((416, 240), 10, 10, 4, {"clip": "edges"}, ["--preset", "fast"]),
    "cli_static_medium/": ((416, 240), 16, 8, 2, {"clip": "static"}, ["--preset", "medium"]),
    "cli_jump_medium/": ((416, 240), 12, 8, 2, {"clip": "jump"}, ["--preset", "medium"]),
    "cli_jump_slow/": ((416, 240), 8, 8, 2, {"clip": "jump"}, ["--preset", "slow"]),
    "cli_dark_aq3/": ((416, 240), 16, 8, 2, {"clip": "dark"}, ["--preset", "medium", "--aq-mode", "3"]),
    "cli_dark_medium_hbd/": ((416, 240), 12, 10, 4, {"clip": "dark"}, ["--preset", "medium"]),
    "cli_static_keyint_inf/": ((416, 240), 20, 8, 2, {"clip": "static"}, ["--preset", "medium", "--keyint", "-1"]),
    "cli_flat_crf1_hbd/": ((416, 240), 8, 10, 4, {"clip": "flat"}, ["--preset", "medium", "--crf", "1"]),
    "cli_noise_veryfast_b0/": ((416, 240), 10, 8, 2, {"clip": "noise"}, ["--preset", "veryfast", "--bframes", "0"]),
    "cli_edges_slower/": ((416, 240), 8, 8, 2, {"clip": "edges"}, ["--preset", "slower"]),
    "cli_jump_faster_ref5/": ((416, 240), 12, 8, 2, {"clip": "jump"}, ["--preset", "faster", "--ref", "5"]),
    "cli_dark_crf40_psnr/": ((416, 240), 16, 8, 2, {"clip": "dark"}, ["--preset", "medium", "--crf", "40", "--tune", "psnr"]),
    "cli_edges_odd_size/": ((420, 236), 10, 8, 2, {"clip": "edges"}, ["--preset", "medium"]),
    "cli_noise_allintra_hbd/": ((416, 240), 6, 10, 4, {"clip": "noise"}, ["--preset", "medium", "--keyint", "1"]),
    "cli_static_nowpp_ft1/": ((416, 240), 16, 8, 2, {"clip": "static"}, ["--preset", "medium", "--no-wpp", "--frame-threads", "1"]),
    "cli_jump_fps60/": ((416, 240), 16, 8, 2, {"clip": "jump"}, ["--preset", "medium", "--fps", "60"]),
    # (the round's last options at the large sizes)
    "cli_uhd_nowpp_ft1/": ((3840, 2160), 4, 8, 2, {}, ["--preset", "medium", "--no-wpp", "--frame-threads", "1"]),
    "cli_uhd_fps60/": ((3840, 2160), 5, 8, 2, {}, ["--preset", "medium", "--fps", "60"]),
    "cli_uhd_odd_size/": ((3838, 2158), 4, 8, 2, {}, ["--preset", "fast"]),
    "cli_fhd_b0_noslices/": ((1920, 1080), 8, 8, 2, {}, ["--preset", "medium", "--bframes", "0", "--lookahead-slices", "0"]),
    "cli_fhd_zerolatency/": ((1920, 1080), 8, 8, 2, {}, ["--preset", "medium", "--tune", "zerolatency"]),
    "cli_fhd_keyint_inf/": ((1920, 1080), 8, 8, 2, {}, ["--preset", "medium", "--keyint", "-1"]),
    "cli_fhd_noise/": ((1920, 1080), 6, 8, 2, {"clip": "noise"}, ["--preset", "medium"]),
    "cli_fhd_edges/": ((1920, 1080), 8, 8, 2, {"clip": "edges"}, ["--preset", "medium"]),
    "cli_720p_jump_slow/": ((1280, 720), 8, 8, 2, {"clip": "jump"}, ["--preset", "slow"]),
    "cli_fhd_static_hbd/": ((1920, 1080), 10, 10, 4, {"clip": "static"}, ["--preset", "medium"]),
    # the video usability information (signalling only): colour description, range, HDR-style transfer with a chroma location, an extended sample aspect ratio with overscan,
    # video format and a display window
    "cli_vui_bt709/": ((416, 240), 4, 8, 2, {}, ["--preset", "medium", "--colorprim", "bt709", "--transfer", "bt709", "--colormatrix", "bt709", "--range", "limited"]),
    "cli_vui_hdr_hbd/": ((416, 240), 4, 10, 4, {}, ["--preset", "medium", "--colorprim", "bt2020", "--transfer", "smpte2084", "--colormatrix", "bt2020nc", "--chromaloc", "2", "--range", "full"]),
    "cli_vui_sar_window/": ((416, 240), 4, 8, 2, {}, ["--preset", "medium", "--sar", "7:5", "--overscan", "crop", "--videoformat", "pal", "--display-window", "8,4,8,4"]),
    # units around the slices: HDR10's SEI units with repeated parameter sets, access unit delimiters, the decoded picture hash in its three forms
    "cli_hdr10_hbd/": ((416, 240), 12, 10, 4, {}, ["--preset", "medium", "--colorprim", "bt2020", "--transfer", "smpte2084", "--colormatrix", "bt2020nc", "--master-display",
                                                   "G(13250,34500)B(7500,3000)R(34000,16000)WP(15635,16450)L(10000000,5)", "--max-cll", "1000,400", "--repeat-headers", "--keyint", "6", "--no-scenecut"]),
    "cli_aud_md5/": ((416, 240), 10, 8, 2, {}, ["--preset", "medium", "--aud", "--hash", "1"]),
    "cli_crc_hbd_odd/": ((424, 232), 8, 10, 4, {}, ["--preset", "medium", "--hash", "2"]),
    "cli_checksum_aud_repeat/": ((416, 240), 10, 8, 2, {}, ["--preset", "medium", "--hash", "3", "--aud", "--repeat-headers"]),
    "cli_maxcll_only/": ((416, 240), 4, 8, 2, {}, ["--preset", "medium", "--max-cll", "600,0"]),
    "cli_deblock_offsets/": ((416, 240), 12, 8, 2, {}, ["--preset", "medium", "--deblock", "-2:3"]),
    "cli_animation/": ((416, 240), 20, 8, 2, {}, ["--preset", "medium", "--tune", "animation"]),
    "cli_animation_hbd_slow/": ((416, 240), 12, 10, 4, {}, ["--preset", "slow", "--tune", "animation"]),
    # --limit-tu: the inter residual quadtree bounded by the CU's first quarter (2), by the neighbouring and co-located CTUs' records (3), by both (4: --preset slower)
    "cli_slower/": ((416, 240), 12, 8, 2, {}, ["--preset", "slower"]),
    "cli_slower_hbd/": ((416, 240), 8, 10, 4, {}, ["--preset", "slower"]),
    "cli_limit_tu2/": ((416, 240), 12, 8, 2, {}, ["--preset", "medium", "--limit-tu", "2", "--tu-inter-depth", "3"]),
    "cli_limit_tu3/": ((416, 240), 12, 8, 2, {}, ["--preset", "medium", "--limit-tu", "3", "--tu-inter-depth", "3", "--tu-intra-depth", "3"]),
    "cli_limit_tu4_rdoq/": ((416, 240), 12, 8, 2, {}, ["--preset", "slow", "--limit-tu", "4", "--tu-inter-depth", "2"]),
    "cli_limit_tu_off/": ((416, 240), 8, 8, 2, {}, ["--preset", "medium", "--limit-tu", "4"]),           # tu-inter-depth 1: switched off by the configuration
    "cli_slower_edges/": ((416, 240), 8, 8, 2, {"clip": "edges"}, ["--preset", "slower"]),
}
# what the command line program must refuse, with words of the reason (x265amd_last_error)
CLI_REFUSED = {
    "ultrafast": (["--preset", "ultrafast"], "maxCUSize"),
    "limit_tu_1": (["--preset", "medium", "--limit-tu", "1", "--tu-inter-depth", "3"], "limitTU"),
    "placebo": (["--preset", "placebo"], "TransformSkip"),
    "bitrate": (["--preset", "medium", "--bitrate", "1000"], "rateControlMode"),
    "grain": (["--preset", "medium", "--tune", "grain"], "Grain"),
    "chroma_qp": (["--preset", "medium", "--cbqpoffs", "2"], "unknown option"),
    "umh": (["--preset", "medium", "--me", "umh"], "searchMethod"),
    "qg16": (["--preset", "medium", "--qg-size", "16"], "qgSize"),
    "nosuchoption": (["--preset", "medium", "--no-such-option"], "unknown option"),
    "max_tu16": (["--preset", "medium", "--max-tu-size", "16"], "maxTUSize"),
    "min_cu16": (["--preset", "medium", "--min-cu-size", "16"], "minCUSize"),
    "level41": (["--preset", "medium", "--level-idc", "41"], "levelIdc"),
    "fhd_b0_slices": (["--preset", "medium", "--bframes", "0"], "lookaheadSlices"),       # (on a 1920x1080 clip; with --lookahead-slices 0 it is a CLI_CASES line)
    "one_ctu": (["--preset", "medium"], "single CTU"),           # (on a 64x64 clip: tests/test_encoder_api.py)      # (with a rate factor the reference turns VBV on for a forced level: level.cpp:393-404)
}


# --weightp (the reference's default): tag -> ((w, h), frames, depth, clip, x265amd_param fields, the reference's options on top of WP_CLI).  The decision is built, the weighted
# paths are not: clips on which the reference's analysis ends without weights
WP_CLI = [o for o in LS_CLI if o != "--no-weightp"] + ["--weightp"]
WP_BASE = dict(LS_BASE, bEnableWeightedPred=1)
WP_CASES = {
    "wp_ft/": ((320, 192), 16, 8, ("ft", None), dict(WP_BASE, bframes=4, lookaheadDepth=8), ["--bframes", "4", "--rc-lookahead", "8"]),
    "wp_api_hbd/": ((256, 192), 12, 10, ("api", None), dict(WP_BASE, bframes=3, lookaheadDepth=6, maxNumReferences=2), ["--bframes", "3", "--rc-lookahead", "6", "--ref", "2"]),
    # the whole preset: --preset medium --qp 30 at 1280x720, nothing switched off but the option-string SEI
    "wp_medium/": ((1280, 720), 12, 8, ("ft", None), dict(WP_BASE, bframes=4, lookaheadDepth=20, lookaheadSlices=8), []),
}


def wp_fade_frames(w=320, h=192, n=14, depth=8, rate=0.045):
    """a fade: the accelerating-texture clip with its luma scaled towards black by `rate` per frame -- the reference's weight analysis picks a weight for the first P picture
    already (and, behind the luma weight, chroma weights: mcChroma's vectors make the unweighted chroma planes look different enough)"""
    out = []
    sc = 1 << (depth - 8)
    dt = np.uint8 if depth == 8 else np.uint16
    for k, f in enumerate(encoder_ft_clip(w, h, n, depth, dy0=2, dy_inc=2, dx_step=4)):
        y = np.clip((f[0].astype(np.float64) - 16 * sc) * (1.0 - rate * k) + 16 * sc + 0.5, 0, 256 * sc - 1).astype(dt)
        out.append([y, f[1], f[2]])
    return out


WP_FADE_CFG = dict(WP_BASE, bframes=3, lookaheadDepth=8)
WP_FADE_CLI = ["--bframes", "3", "--rc-lookahead", "8"]
# clips on which the reference's analysis DOES pick weights (round 5: coded with them): tag -> ((w, h), frames, depth, fade per frame, x265amd_param fields, the reference's options
# on top of WP_CLI).  Golden data (tests/golden/make_golden.py fade): the stream, the reconstructions, the frame types and the reference's "weights:" log lines
FADE_CASES = {
    "wp_fade/": ((320, 192), 14, 8, 0.045, WP_FADE_CFG, WP_FADE_CLI),                                                                                  # P pictures only (the trellis finds no use for B)
    "wp_fade_hbd/": ((320, 192), 12, 10, 0.045, dict(WP_BASE, bframes=2, lookaheadDepth=6), ["--bframes", "2", "--rc-lookahead", "6"]),                 # Main 10
    # sub-sample refinement with chroma (subme 3): the searches read weighted CHROMA planes too (MotionReference::numInterpPlanes, reference.cpp:56)
    "wp_fade_sub3/": ((320, 192), 10, 8, 0.04, dict(WP_BASE, bframes=3, lookaheadDepth=8, subpelRefine=3), ["--bframes", "3", "--rc-lookahead", "8", "--subme", "3"]),
    # B pictures with weights (--weightb): fixed mini-GOPs so that there ARE B pictures in a fade; both lists analysed, bi-prediction weighted (addWeightBi)
    "wp_fade_b/": ((320, 192), 13, 8, 0.03, dict(WP_BASE, bframes=2, lookaheadDepth=6, bFrameAdaptive=0, bBPyramid=0, bEnableWeightedBiPred=1),
                   ["--bframes", "2", "--rc-lookahead", "6", "--b-adapt", "0", "--no-b-pyramid", "--weightb"]),
    # ... and with the bidirectional candidate measured by motionCompensation (chroma SATD, subme 4) and the B pyramid
    "wp_fade_b4_hbd/": ((256, 192), 11, 10, 0.035, dict(WP_BASE, bframes=3, lookaheadDepth=6, bFrameAdaptive=0, bEnableWeightedBiPred=1, subpelRefine=4),
                        ["--bframes", "3", "--rc-lookahead", "6", "--b-adapt", "0", "--weightb", "--subme", "4"]),
}


def fade_case_frames(tag):
    (w, h), n, depth, rate, _, _ = FADE_CASES[tag]
    return wp_fade_frames(w, h, n, depth, rate)


def wp_case_frames(tag):
    (w, h), n, depth, (kind, arg), _, _ = WP_CASES[tag]
    if kind == "ft":
        return encoder_ft_clip(w, h, n, depth, dy0=2, dy_inc=2, dx_step=4)
    return encoder_api_clip(tag, w, h, n, depth)


# --b-adapt 1 (fast): tag -> ((w, h), frames, depth, clip, x265amd_param fields, the reference's options on top of B1_CLI)
B1_CLI = [o if o != "2" or BA_CLI[i - 1] != "--b-adapt" else "1" for i, o in enumerate(BA_CLI)]
B1_BASE = dict(BA_BASE, bFrameAdaptive=1)
B1_CASES = {
    "ba1_drift/": ((320, 192), 20, 8, ("api", None), dict(B1_BASE, bframes=4, lookaheadDepth=10), ["--bframes", "4", "--rc-lookahead", "10"]),
    "ba1_cut/": ((320, 192), 18, 8, ("scene", [9]), dict(B1_BASE, bframes=3, lookaheadDepth=8), ["--bframes", "3", "--rc-lookahead", "8"]),
    "ba1_ft_hbd/": ((256, 192), 14, 10, ("ft", None), dict(B1_BASE, bframes=4, lookaheadDepth=6), ["--bframes", "4", "--rc-lookahead", "6"]),
    # with everything else of the preset: B pyramid, open GOPs, the lookahead in slices (every estimate of --b-adapt 1 is made when asked for, i.e. in slices), weighted prediction
    "ba1_medium/": ((1280, 720), 12, 8, ("ft", None), dict(WP_BASE, bFrameAdaptive=1, bframes=4, lookaheadDepth=20, lookaheadSlices=8), ["--b-adapt", "1"]),
}


def b1_case_frames(tag):
    (w, h), n, depth, (kind, arg), _, _ = B1_CASES[tag]
    if kind == "scene":
        return scene_clip(w, h, n, arg, depth)
    if kind == "ft":
        return encoder_ft_clip(w, h, n, depth, dy0=2, dy_inc=2, dx_step=4)
    return encoder_api_clip(tag, w, h, n, depth)


def ba_case_frames(tag):
    (w, h), n, depth, (kind, arg), _, _ = BA_CASES[tag]
    if kind == "scene":
        return scene_clip(w, h, n, arg, depth)
    if kind == "ft":
        return encoder_ft_clip(w, h, n, depth, dy0=2, dy_inc=2, dx_step=4)
    return encoder_api_clip(tag, w, h, n, depth)


def scene_case_frames(tag):
    (w, h), n, depth, cuts, _, _ = SC_CASES[tag]
    return scene_clip(w, h, n, cuts, depth)


# ---- lookahead lowres pipeline (x265amd_lowres_init / x265amd_lowres_intra_costs vs Lowres::init / LookaheadTLD::lowresIntraEstimate) ----
LOWRES_LAMBDA = {8: 1, 10: 16}      # (int)x265_lambda_tab[X265_LOOKAHEAD_QP], X265_LOOKAHEAD_QP = 12 + 6 * (X265_DEPTH - 8) (common/constants.cpp, common/common.h:213)


def lowres_case(depth, seed, crop=(0, 0)):
    """padded full-resolution luma plane of inter_scene and the lowres geometry (half size, same margins)"""
    pics, stride, cstride, org = inter_scene(depth, seed, npics=1)
    W, H = MC_W - crop[0], MC_H - crop[1]
    luma = pics[0][:(MC_H + 2 * MC_MY) * stride].reshape(-1, stride).copy()
    if crop != (0, 0):      # a smaller picture inside the same buffer: re-extend its borders
        core = luma[MC_MY:MC_MY + H, MC_MX:MC_MX + W]
        luma = np.pad(core, ((MC_MY, MC_MY + crop[1]), (MC_MX, MC_MX + crop[0])), mode="edge")
    lw, lh = W // 2, H // 2
    lstride = lw + 2 * MC_MX
    return dict(depth=depth, luma=np.ascontiguousarray(luma), stride=stride, W=W, H=H, lw=lw, lh=lh, lstride=lstride, rows=lh + 2 * MC_MY,
                wcu=(lw + 7) >> 3, hcu=(lh + 7) >> 3)


def lowres_run_ref(R, c):
    dt = c["luma"].dtype
    planes = [np.zeros((c["rows"], c["lstride"]), dt) for _ in range(4)]
    o = MC_MY * c["lstride"] + MC_MX
    isz = dt.itemsize
    src0 = c["luma"].ctypes.data + (MC_MY * c["stride"] + MC_MX) * isz
    R.lib.ref_lowres_init.restype = None
    R.lib.ref_lowres_init(C.c_void_p(src0), C.c_int64(c["stride"]), c["lw"], c["lh"], *[C.c_void_p(p.ctypes.data + o * isz) for p in planes], C.c_int64(c["lstride"]),
                          MC_MX, MC_MY)
    ncu = c["wcu"] * c["hcu"]
    cost = np.zeros(ncu, np.int32); mode = np.zeros(ncu, np.uint8); rows = np.zeros(c["hcu"], np.int32); lc = np.zeros(ncu, np.uint16); sums = np.zeros(2, np.int64)
    R.lib.ref_lowres_intra.restype = None
    R.lib.ref_lowres_intra(C.c_void_p(planes[0].ctypes.data + o * isz), C.c_int64(c["lstride"]), c["wcu"], c["hcu"], _ptr(cost), _ptr(mode), _ptr(rows), _ptr(lc), _ptr(sums))
    return planes, cost, mode, rows, lc, sums


def lowres_frame_sums(c, cost):
    """the caller's reduction of lowresIntraEstimate without AQ (slicetype.cpp:797-823): lowresCosts, rowSatds, costEst"""
    wcu, hcu = c["wcu"], c["hcu"]
    cc = cost.reshape(hcu, wcu).astype(np.int64)
    inner = np.zeros((hcu, wcu), bool)
    inner[1:hcu - 1, 1:wcu - 1] = True
    if wcu <= 2 or hcu <= 2:
        inner[:] = True
    return np.minimum(cost, 0x3FFF).astype(np.uint16), cc.sum(1).astype(np.int32), int(cc[inner].sum())


def lowres_run_hip(L, c):
    import torch
    dt = c["luma"].dtype
    isz = dt.itemsize
    d_src = torch.from_numpy(c["luma"].view(np.uint8)).cuda()
    d_planes = [torch.zeros(c["rows"] * c["lstride"] * isz, dtype=torch.uint8, device="cuda") for _ in range(4)]
    o = (MC_MY * c["lstride"] + MC_MX) * isz
    ptrs = (C.c_void_p * 4)(*[p.data_ptr() + o for p in d_planes])
    rc = L.lib.x265amd_lowres_init(None, C.c_void_p(d_src.data_ptr() + (MC_MY * c["stride"] + MC_MX) * isz), C.c_int64(c["stride"]), c["lw"], c["lh"], ptrs,
                                   C.c_int64(c["lstride"]), MC_MX, MC_MY)
    assert rc == 0
    ncu = c["wcu"] * c["hcu"]
    d_cost = torch.zeros(ncu, dtype=torch.int32, device="cuda"); d_mode = torch.zeros(ncu, dtype=torch.uint8, device="cuda")
    rc = L.lib.x265amd_lowres_intra_costs(None, C.c_void_p(d_planes[0].data_ptr() + o), C.c_int64(c["lstride"]), c["wcu"], c["hcu"], LOWRES_LAMBDA[c["depth"]],
                                          C.c_void_p(d_cost.data_ptr()), C.c_void_p(d_mode.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    planes = [p.cpu().numpy().view(dt).reshape(c["rows"], c["lstride"]) for p in d_planes]
    return planes, d_cost.cpu().numpy(), d_mode.cpu().numpy()


# ---- lookahead frame cost (x265amd_lowres_frame_cost vs CostEstimateGroup::estimateFrameCost) ----
def lowres_cost_case(depth, seed, crop=(0, 0)):
    """three frames (display order) of a scene with global drift plus blocks that move on their own, as padded luma planes"""
    pics, stride, cstride, org = inter_scene(depth, seed, npics=3)
    rng = np.random.default_rng(seed + 4711)
    W, H = MC_W - crop[0], MC_H - crop[1]
    rows = MC_H + 2 * MC_MY
    lumas = []
    base = pics[0][:rows * stride].reshape(rows, stride)
    for k in range(3):
        l = pics[k][:rows * stride].reshape(rows, stride).copy()
        for _ in range(25):
            bs = int(rng.choice([16, 16, 32, 48]))
            bx, by = int(rng.integers(0, (W - bs) // 2)) * 2, int(rng.integers(0, (H - bs) // 2)) * 2
            dx, dy = int(rng.integers(-12, 13)), int(rng.integers(-10, 11))
            l[MC_MY + by:MC_MY + by + bs, MC_MX + bx:MC_MX + bx + bs] = base[MC_MY + by + dy:MC_MY + by + dy + bs, MC_MX + bx + dx:MC_MX + bx + dx + bs]
        core = l[MC_MY:MC_MY + H, MC_MX:MC_MX + W]
        lumas.append(np.ascontiguousarray(np.pad(core, ((MC_MY, MC_MY + crop[1]), (MC_MX, MC_MX + crop[0])), mode="edge")))
    return dict(depth=depth, lumas=lumas, stride=stride, W=W, H=H, wcu=(W // 2 + 7) >> 3, hcu=(H // 2 + 7) >> 3)


def lowres_cost_run_ref(R, c, p0, b, p1):
    isz = c["lumas"][0].itemsize
    ptrs = (C.c_void_p * 3)(*[l.ctypes.data + (MC_MY * c["stride"] + MC_MX) * isz for l in c["lumas"]])
    ncu = c["wcu"] * c["hcu"]
    lc = np.zeros(ncu, np.uint16); mvs = np.zeros((2, ncu, 2), np.int16); mvc = np.zeros((2, ncu), np.int32); ic = np.zeros(ncu, np.int32)
    rows = np.zeros(c["hcu"], np.int32); sums = np.zeros(3, np.int64)
    R.lib.ref_lowres_frame_cost.restype = C.c_int
    n = R.lib.ref_lowres_frame_cost(ptrs, C.c_int64(c["stride"]), c["W"], c["H"], MC_MX, MC_MY, p0, b, p1, 2, _ptr(lc), _ptr(mvs), _ptr(mvc), _ptr(ic), _ptr(rows), _ptr(sums))
    assert n == ncu, (n, ncu)
    return dict(lowres_costs=lc, mvs=mvs, mv_costs=mvc, intra_cost=ic, row_satds=rows, sums=sums)


def lowres_cost_sums(c, lowres_costs, bcost, bidir):
    """the caller's reduction (estimateCUCost tail + estimateFrameCost, slicetype.cpp:4220-4248, :4062-4067): score, intra block count, row sums"""
    wcu, hcu = c["wcu"], c["hcu"]
    bc = bcost.reshape(hcu, wcu).astype(np.int64)
    inner = np.zeros((hcu, wcu), bool)
    inner[1:hcu - 1, 1:wcu - 1] = True
    if wcu <= 2 or hcu <= 2:
        inner[:] = True
    est = int(bc[inner].sum())
    intra_mbs = 0 if bidir else int((((lowres_costs.reshape(hcu, wcu) >> 14) == 0) & inner).sum())
    score = est * 100 // 130 if bidir else est
    return score, est, intra_mbs, bc.sum(1).astype(np.int32)


def lowres_cost_run_hip(L, me, c, p0, b, p1):
    """Lowres::init of the three frames, intra costs, then ONE frame cost of b against p0 (and p1 when p1 > b) through x265amd_lowres_frame_cost, unsliced and unweighted, with
    every list searched (do_search0 = 1, do_search1 = bidir): what estimateFrameCost does on fresh Lowres objects.  No field is reused here; the reuse, sliced and weighted
    forms are LowresPathsDev's (below)"""
    import torch
    depth = c["depth"]
    dt = c["lumas"][0].dtype
    isz = dt.itemsize
    lw, lh = c["wcu"] * 8, c["hcu"] * 8                 # Lowres::create rounds the lowres size up to whole blocks
    lstride = (c["W"] // 2) + 2 * MC_MX
    lstride += (32 - (lstride & 31)) & 31
    rows = lh + 2 * MC_MY
    o = (MC_MY * lstride + MC_MX) * isz
    planes, intra = [], []
    ncu = c["wcu"] * c["hcu"]
    for k in range(3):
        d_src = torch.from_numpy(c["lumas"][k].view(np.uint8)).cuda()
        d_pl = [torch.zeros(rows * lstride * isz, dtype=torch.uint8, device="cuda") for _ in range(4)]
        ptrs = (C.c_void_p * 4)(*[p.data_ptr() + o for p in d_pl])
        assert L.lib.x265amd_lowres_init(None, C.c_void_p(d_src.data_ptr() + (MC_MY * c["stride"] + MC_MX) * isz), C.c_int64(c["stride"]), lw, lh, ptrs, C.c_int64(lstride),
                                         MC_MX, MC_MY) == 0
        d_cost = torch.zeros(ncu, dtype=torch.int32, device="cuda"); d_mode = torch.zeros(ncu, dtype=torch.uint8, device="cuda")
        assert L.lib.x265amd_lowres_intra_costs(None, C.c_void_p(d_pl[0].data_ptr() + o), C.c_int64(lstride), c["wcu"], c["hcu"], LOWRES_LAMBDA[depth],
                                                C.c_void_p(d_cost.data_ptr()), C.c_void_p(d_mode.data_ptr())) == 0
        planes.append(d_pl); intra.append(d_cost)
    torch.cuda.synchronize()
    bidir = p1 > b
    d_mvs = [torch.zeros(ncu * 2, dtype=torch.int16, device="cuda") for _ in range(2)]
    d_mvc = [torch.zeros(ncu, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_lc = torch.zeros(ncu, dtype=torch.int16, device="cuda"); d_bc = torch.zeros(ncu, dtype=torch.int32, device="cuda"); d_prog = torch.zeros(c["hcu"], dtype=torch.int32, device="cuda")
    ref0 = (C.c_void_p * 4)(*[p.data_ptr() + o for p in planes[p0]])
    ref1 = (C.c_void_p * 4)(*[p.data_ptr() + o for p in planes[p1]]) if bidir else None
    rc = L.lib.x265amd_lowres_frame_cost(None, me.ctx, C.c_void_p(planes[b][0].data_ptr() + o), ref0, ref1, C.c_int64(lstride), c["wcu"], c["hcu"], 1, int(bidir),
                                         C.c_void_p(intra[b].data_ptr()), C.c_void_p(d_mvs[0].data_ptr()), C.c_void_p(d_mvc[0].data_ptr()),
                                         C.c_void_p(d_mvs[1].data_ptr()) if bidir else None, C.c_void_p(d_mvc[1].data_ptr()) if bidir else None,
                                         C.c_void_p(d_lc.data_ptr()), C.c_void_p(d_bc.data_ptr()), C.c_void_p(d_prog.data_ptr()))
    assert rc == 0, L.lib.x265amd_last_error()
    torch.cuda.synchronize()
    lc = d_lc.cpu().numpy().view(np.uint16); bc = d_bc.cpu().numpy()
    mvs = np.stack([d_mvs[l].cpu().numpy().reshape(ncu, 2) for l in range(2)]); mvc = np.stack([d_mvc[l].cpu().numpy() for l in range(2)])
    score, est, intra_mbs, rows_ = lowres_cost_sums(c, lc, bc, bidir)
    return dict(lowres_costs=lc, mvs=mvs, mv_costs=mvc, intra_cost=intra[b].cpu().numpy(), row_satds=rows_, sums=np.array([score, est, intra_mbs], np.int64))


# ---- lookahead frame cost, the paths beside the plain one: cooperative slices, weighted search planes, reused motion fields (tests/test_lookahead_paths.py) ----
# golden: tests/golden/lowres_paths_golden.npz, made by tests/golden/make_lowres_paths_golden.py from the reference's own estimateCUCost (oracle/refprims.cpp:
# ref_lowres_frame_cost_paths)
PATHS_GOLD = os.path.join(GOLDEN_DIR, "lowres_paths_golden.npz")
PATHS_WEIGHT = (90, 7, 10)          # (scale, log2 denom, offset at 8 bits): 90 / 128 = 0.70, the fade of lowres_fade_case
# scene -> (bit depth, seed, crop, fade).  s8 / s10 are scenes of tests/test_lowres.py's COST_CASES, so their unsliced entries must repeat lowres_cost_golden.npz
PATHS_SCENES = {"s8": (8, 22, (0, 0), False), "c8": (8, 23, (24, 40), False), "f8": (8, 26, (0, 0), True),
                "s10": (10, 24, (0, 0), False), "c10": (10, 25, (24, 40), False), "f10": (10, 27, (0, 0), True)}
# slice layouts the reference can form (numSlices = hcu / rowsPerSlice), per block-row count; the last one is "one slice" = no slices
PATHS_LAYOUTS = {12: [(4, 3), (5, 2), (6, 2), (12, 1)], 10: [(5, 2), (3, 3), (10, 1)]}
PATHS_KINDS = {"P": (0, 1, 1), "B": (0, 1, 2)}
LOWRES_JOB_DT = np.dtype([("d_fenc", "<u8"), ("d_ref0", "<u8", 4), ("d_ref1", "<u8", 4), ("d_intra_cost", "<u8"), ("d_mvs0", "<u8"), ("d_mv_costs0", "<u8"), ("d_mvs1", "<u8"),
                          ("d_mv_costs1", "<u8"), ("d_lowres_costs", "<u8"), ("d_bcost", "<u8"), ("do_search0", "<i4"), ("do_search1", "<i4"), ("rows_per_slice", "<i4"),
                          ("num_slices", "<i4"), ("d_ref0w", "<u8", 4)])         # x265amd_lowres_cost_job (include/x265amd.h)


def lowres_fade_case(depth, seed, crop=(0, 0)):
    """lowres_cost_case under a fade: frame 1 is its own content (frame 0's plus the scene's motion) at 179 / 256 = 0.70 of the brightness plus 10, frame 2 at 102 / 256 = 0.40
    plus 20 -- so the weight (90, 7, 10) on frame 0 predicts frame 1 far better than no weight, and the plain average of frames 0 and 2 predicts it as well (0.70, +10)"""
    c = lowres_cost_case(depth, seed, crop)
    sh = depth - 8
    for k, (num, off) in ((1, (179, 10)), (2, (102, 20))):
        l = c["lumas"][k]
        c["lumas"][k] = np.ascontiguousarray((((l.astype(np.int64) * num + 128) >> 8) + (off << sh)).astype(l.dtype))
    return c


def lowres_paths_scene(scene):
    depth, seed, crop, fade = PATHS_SCENES[scene]
    return (lowres_fade_case if fade else lowres_cost_case)(depth, seed, crop)


def lowres_paths_specs():
    """every entry of the golden, in the order in which the reference computed them: name -> dict(scene, kind, slices (rowsPerSlice, numSlices) or (0, 0), search (list 0,
    list 1), weight or None, src: the entry whose fields the lists that are not searched read)"""
    specs = {}

    def add(name, scene, kind, slices=(0, 0), search=None, weight=None, src=None):
        specs[name] = dict(scene=scene, kind=kind, slices=slices, search=search or (1, int(kind == "B")), weight=weight, src=src)

    for depth in (8, 10):
        s, cr, f = "s%d" % depth, "c%d" % depth, "f%d" % depth
        for scene, hcu in ((s, 12), (cr, 10)):
            for kind in ("P", "B"):
                add("%s/%s/u" % (scene, kind), scene, kind)
                for (rps, ns) in PATHS_LAYOUTS[hcu]:
                    add("%s/%s/%dx%d" % (scene, kind, rps, ns), scene, kind, (rps, ns))
        lay = (4, 3) if depth == 8 else (5, 2)
        add(f + "/P/u", f, "P")
        for kind in ("P", "B"):
            add("%s/%s/w" % (f, kind), f, kind, weight=PATHS_WEIGHT)
            add("%s/%s/w%dx%d" % (f, kind, lay[0], lay[1]), f, kind, lay, weight=PATHS_WEIGHT)
        # reuse: the searched P estimate's list-0 field read by a B estimate that searches list 1 only, then that B estimate measured again with both fields read
        add(s + "/B/mixed", s, "B", search=(0, 1), src=s + "/P/u")
        add(s + "/B/measure", s, "B", search=(0, 0), src=s + "/B/mixed")
        add("%s/B/mixed%dx%d" % (s, lay[0], lay[1]), s, "B", lay, search=(0, 1), src="%s/P/%dx%d" % (s, lay[0], lay[1]))
        # and as the reference runs a fade: the P estimate searched list 0 on the weighted planes; the B estimate that reads that field has no weight (estimateFrameCost
        # clears isWeighted and analyses weights only when it searches list 0, slicetype.cpp:3997-3999).  A search of list 0 here would find other vectors
        add(f + "/B/reuse", f, "B", search=(0, 1), src=f + "/P/w")
    return specs


def lowres_paths_run_ref(R, c, spec, src=None):
    """one entry from the reference (CPU, oracle/_ref): src = the result whose fields are read"""
    p0, b, p1 = PATHS_KINDS[spec["kind"]]
    isz = c["lumas"][0].itemsize
    ptrs = (C.c_void_p * 3)(*[l.ctypes.data + (MC_MY * c["stride"] + MC_MX) * isz for l in c["lumas"]])
    ncu = c["wcu"] * c["hcu"]
    rps, ns = spec["slices"]
    lc = np.zeros(ncu, np.uint16); ic = np.zeros(ncu, np.int32); rows = np.zeros(c["hcu"], np.int32); ssum = np.zeros((max(ns, 1), 2), np.int64)
    mvs = src["mvs"].copy() if src is not None else np.zeros((2, ncu, 2), np.int16)
    mvc = src["mv_costs"].copy() if src is not None else np.zeros((2, ncu), np.int32)
    search = np.array(spec["search"], np.int32)
    weight = np.array((1,) + tuple(spec["weight"]) if spec["weight"] else (0, 0, 0, 0), np.int32)
    R.lib.ref_lowres_frame_cost_paths.restype = C.c_int
    n = R.lib.ref_lowres_frame_cost_paths(ptrs, C.c_int64(c["stride"]), c["W"], c["H"], MC_MX, MC_MY, p0, b, p1, 2, ns, rps, _ptr(search), _ptr(weight),
                                          _ptr(lc), _ptr(mvs), _ptr(mvc), _ptr(ic), _ptr(rows), _ptr(ssum))
    assert n == ncu, (n, ncu)
    return dict(lowres_costs=lc, mvs=mvs, mv_costs=mvc, intra_cost=ic, row_satds=rows, slice_sums=ssum)


def lowres_paths_golden_entry(g, name):
    return {k: g["%s/%s" % (name, k)] for k in ("lowres_costs", "mvs", "mv_costs", "row_satds", "slice_sums")}


def lowres_slice_rows(hcu, slices):
    """block rows [first, last] of every slice (processTasks, slicetype.cpp:3957-3958); no slices: the picture"""
    rps, ns = slices
    if ns <= 1:
        return [(0, hcu - 1)]
    return [(rps * i, hcu - 1 if i == ns - 1 else rps * (i + 1) - 1) for i in range(ns)]


def lowres_slice_sums(c, lowres_costs, bcost, bidir, slices):
    """lowres_cost_sums per slice: estimateCUCost's tail (slicetype.cpp:4220-4245) adds a block that is not on the PICTURE's edge to its slice's costEst / intraMbs"""
    wcu, hcu = c["wcu"], c["hcu"]
    bc = bcost.reshape(hcu, wcu).astype(np.int64)
    inner = np.zeros((hcu, wcu), bool)
    inner[1:hcu - 1, 1:wcu - 1] = True
    if wcu <= 2 or hcu <= 2:
        inner[:] = True
    intra = ((lowres_costs.reshape(hcu, wcu) >> 14) == 0) & inner
    out = []
    for (y0, y1) in lowres_slice_rows(hcu, slices):
        out.append((int(bc[y0:y1 + 1][inner[y0:y1 + 1]].sum()), 0 if bidir else int(intra[y0:y1 + 1].sum())))
    return np.array(out, np.int64)


class LowresPathsDev:
    """the device side of a lowres_cost_case: per frame ONE buffer of the four padded lowres planes (as Lowres::create lays them out) and the intra costs; estimates in any of
    the forms of x265amd_lowres_cost_job go through x265amd_lowres_frame_cost_batch, any number per launch"""

    def __init__(self, L, me, c):
        import torch
        self.torch, self.L, self.me, self.c = torch, L, me, c
        depth = c["depth"]
        self.dt = c["lumas"][0].dtype
        isz = self.isz = self.dt.itemsize
        lw, lh = c["wcu"] * 8, c["hcu"] * 8
        lstride = (c["W"] // 2) + 2 * MC_MX
        lstride += (32 - (lstride & 31)) & 31
        self.lstride, self.rows = lstride, lh + 2 * MC_MY
        self.planesize = self.rows * lstride                     # samples
        self.o = (MC_MY * lstride + MC_MX) * isz
        self.ncu = c["wcu"] * c["hcu"]
        self.buf, self.intra = [], []
        for k in range(3):
            d_src = torch.from_numpy(c["lumas"][k].view(np.uint8)).cuda()
            d_buf = torch.zeros(4 * self.planesize * isz, dtype=torch.uint8, device="cuda")
            ptrs = (C.c_void_p * 4)(*self.plane_ptrs(d_buf))
            assert L.lib.x265amd_lowres_init(None, C.c_void_p(d_src.data_ptr() + (MC_MY * c["stride"] + MC_MX) * isz), C.c_int64(c["stride"]), lw, lh, ptrs, C.c_int64(lstride),
                                             MC_MX, MC_MY) == 0
            d_cost = torch.zeros(self.ncu, dtype=torch.int32, device="cuda"); d_mode = torch.zeros(self.ncu, dtype=torch.uint8, device="cuda")
            assert L.lib.x265amd_lowres_intra_costs(None, C.c_void_p(d_buf.data_ptr() + self.o), C.c_int64(lstride), c["wcu"], c["hcu"], LOWRES_LAMBDA[depth],
                                                    C.c_void_p(d_cost.data_ptr()), C.c_void_p(d_mode.data_ptr())) == 0
            self.buf.append(d_buf); self.intra.append(d_cost)
        torch.cuda.synchronize()
        self.wbuf = {}

    def plane_ptrs(self, d_buf):
        """sample (0, 0) of the four planes of a buffer"""
        return [d_buf.data_ptr() + k * self.planesize * self.isz + self.o for k in range(4)]

    def weighted(self, k, weight):
        """LookaheadTLD::weightsAnalyse's weighted copies of frame k's four planes: x265amd_weight_buffer over the whole buffer, margins included"""
        key = (k,) + tuple(weight)
        if key not in self.wbuf:
            scale, denom, off = weight
            corr = 14 - self.c["depth"]
            d = self.torch.zeros_like(self.buf[k])
            assert self.L.lib.x265amd_weight_buffer(None, C.c_void_p(self.buf[k].data_ptr()), C.c_void_p(d.data_ptr()), C.c_size_t(4 * self.planesize), scale,
                                                    (1 << (denom - 1) if denom else 0) << corr, denom + corr, off << (self.c["depth"] - 8)) == 0, self.L.lib.x265amd_last_error()
            self.torch.cuda.synchronize()
            self.wbuf[key] = d
        return self.wbuf[key]

    def host_planes(self, d_buf):
        return d_buf.cpu().numpy().view(self.dt).reshape(4 * self.rows, self.lstride)

    def run(self, jobs):
        """jobs: dicts(kind, slices, search, weight, src = the result whose fields the lists that are not searched read) -> results in one launch.  Every output buffer starts
        filled with a pattern that no result has; the fields that are only read are returned as they are AFTER the launch (mvs / mv_costs of that list)"""
        torch = self.torch
        ncu = self.ncu
        rec = np.zeros(len(jobs), LOWRES_JOB_DT); keep = []
        for i, j in enumerate(jobs):
            p0, b, p1 = PATHS_KINDS[j["kind"]]
            bidir = p1 > b
            mv, mc = [], []
            for l in range(2):
                if not j["search"][l] and (l == 0 or bidir):
                    mv.append(torch.from_numpy(j["src"]["mvs"][l].reshape(-1).copy()).cuda()); mc.append(torch.from_numpy(j["src"]["mv_costs"][l].copy()).cuda())
                else:
                    mv.append(torch.full((ncu * 2,), 0x5A5A, dtype=torch.int16, device="cuda")); mc.append(torch.full((ncu,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"))
            lc = torch.full((ncu,), 0x5A5A, dtype=torch.int16, device="cuda"); bc = torch.full((ncu,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            keep.append((mv, mc, lc, bc))
            r = rec[i]
            d = j.get("dev") or self                # (the pictures of another scene of the same size)
            r["d_fenc"] = d.buf[b].data_ptr() + self.o
            r["d_ref0"] = self.plane_ptrs(d.buf[p0])
            if bidir:
                r["d_ref1"] = self.plane_ptrs(d.buf[p1])
                r["d_mvs1"], r["d_mv_costs1"], r["do_search1"] = mv[1].data_ptr(), mc[1].data_ptr(), int(j["search"][1])
            r["d_intra_cost"] = d.intra[b].data_ptr()
            r["d_mvs0"], r["d_mv_costs0"], r["do_search0"] = mv[0].data_ptr(), mc[0].data_ptr(), int(j["search"][0])
            r["d_lowres_costs"], r["d_bcost"] = lc.data_ptr(), bc.data_ptr()
            r["rows_per_slice"], r["num_slices"] = j["slices"]
            if j.get("weight"):
                r["d_ref0w"] = self.plane_ptrs(d.weighted(p0, j["weight"]))
        torch.cuda.synchronize()
        assert self.L.lib.x265amd_lowres_frame_cost_batch(None, self.me.ctx, rec.ctypes.data_as(C.c_void_p), len(jobs), C.c_int64(self.lstride), self.c["wcu"], self.c["hcu"]) == 0, \
            self.L.lib.x265amd_last_error()
        torch.cuda.synchronize()
        sums = np.zeros(2 * len(jobs), np.int64)
        assert self.L.lib.x265amd_lowres_cost_sums(None, rec.ctypes.data_as(C.c_void_p), len(jobs), self.c["wcu"], self.c["hcu"], sums.ctypes.data_as(C.c_void_p)) == 0
        out = []
        for i, (mv, mc, lc, bc) in enumerate(keep):
            out.append(dict(lowres_costs=lc.cpu().numpy().view(np.uint16), bcost=bc.cpu().numpy(), mvs=np.stack([m.cpu().numpy().reshape(ncu, 2) for m in mv]),
                            mv_costs=np.stack([m.cpu().numpy() for m in mc]), device_sums=(int(sums[2 * i]), int(sums[2 * i + 1]))))
        return out


def lowres_paths_assert(c, job, got, want, tag=""):
    """one estimate of LowresPathsDev.run against its golden entry, bit for bit: lowresCosts, the row sums of the unclipped costs, the fields and MV costs of the lists the
    estimate has, the per-slice sums (m_slice[i].costEst / intraMbs) and, over all slices, the device's own reduction"""
    bidir = job["kind"] == "B"
    assert np.array_equal(got["lowres_costs"], want["lowres_costs"]), (tag, "lowres_costs", np.argwhere(got["lowres_costs"] != want["lowres_costs"])[:6].ravel().tolist())
    rows = got["bcost"].reshape(c["hcu"], c["wcu"]).astype(np.int64).sum(1)
    assert np.array_equal(rows, want["row_satds"]), (tag, "row sums", rows.tolist(), want["row_satds"].tolist())
    for l in range(1 + bidir):
        assert np.array_equal(got["mvs"][l], want["mvs"][l]), (tag, "mvs", l, np.argwhere(got["mvs"][l] != want["mvs"][l])[:6].tolist())
        assert np.array_equal(got["mv_costs"][l], want["mv_costs"][l]), (tag, "mv_costs", l, np.argwhere(got["mv_costs"][l] != want["mv_costs"][l])[:6].ravel().tolist())
    ss = lowres_slice_sums(c, got["lowres_costs"], got["bcost"], bidir, job["slices"])
    assert np.array_equal(ss, want["slice_sums"]), (tag, "slice sums", ss.tolist(), want["slice_sums"].tolist())
    assert got["device_sums"] == (int(ss[:, 0].sum()), int(ss[:, 1].sum())), (tag, got["device_sums"], ss.tolist())


# ---- weightCost with motion vectors, restated from the reference with the oracle's pieces (tests/test_lookahead_paths.py f, g) ----
def weight_cand(depth, scale, denom, off):
    """x265amd_weight_cand as weightCost passes weight_pp's arguments (weightPrediction.cpp:182-189)"""
    corr = 14 - depth
    return (1, scale, (1 << (denom - 1) if denom else 0) << corr, denom + corr, off << (depth - 8))


WEIGHT_MARGIN = 32      # samples around the planes of the weight-cost fixtures: a clipped vector reaches 8 + 8 samples beyond the picture, an interpolation two more


def weight_cost_planes(depth, seed, width, height, nplanes):
    """source plane and nplanes reference planes (unrelated enough that reading the wrong one shows), each with WEIGHT_MARGIN samples around width x height"""
    rng = np.random.default_rng(seed)
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    hh, ww = height + 2 * WEIGHT_MARGIN + 8, width + 2 * WEIGHT_MARGIN
    ww += (32 - (ww & 31)) & 31
    base = np.kron(rng.integers(0, pmax + 1, ((hh + 7) // 8, (ww + 7) // 8)), np.ones((8, 8), np.int64))[:hh, :ww]
    refs = [np.clip(np.roll(base, (k, 2 * k), (0, 1)) + rng.integers(-24, 25, (hh, ww)) * (1 << (depth - 8)), 0, pmax).astype(dt) for k in range(nplanes)]
    fenc = np.clip(base * 0.7 + (12 << (depth - 8)) + rng.integers(-6, 7, (hh, ww)) * (1 << (depth - 8)), 0, pmax).astype(dt)
    return fenc, refs, ww


def weight_cost_luma_mvs(seed, width, height):
    """a field for mcLuma: every quarter-sample phase, vectors far outside the picture in the four directions, a zero vector"""
    rng = np.random.default_rng(seed)
    bw, bh = width >> 3, (height + 7) >> 3
    mv = np.zeros((bh * bw, 2), np.int16)
    for i in range(bh * bw):
        ph = (i * 7) & 15
        mv[i] = (4 * int(rng.integers(-5, 6)) + (ph & 3), 4 * int(rng.integers(-5, 6)) + (ph >> 2))
        if (i + i // bw) % 3 == 1:
            far = ((-3000, 5), (3000, -7), (6, -3000), (-9, 3000), (-2500, -2500), (2500, 2500))[(i // 3) % 6]
            mv[i] = far
    mv[0] = (0, 0)
    return mv


def mv_clip_luma(mv, x, y, width, height):
    """mcLuma's clip to the picture + 8 samples (weightPrediction.cpp:72-73, :79-84)"""
    return (min(max(int(mv[0]), (-x - 8) * 4), (width - x - 1 + 8) * 4), min(max(int(mv[1]), (-y - 8) * 4), (height - y - 1 + 8) * 4))


def weight_cost_luma_expected(O, depth, fenc, refs, stride, width, height, mvs, intra, cand):
    """weightAnalyse's luma measurement in the reference's order: mcLuma (weightPrediction.cpp:58-90: per 8x8 block the vector clipped, ReferencePlanes::lowresMC, lowres.h:71-96
    -- the half-sample plane (y & 2) | ((x & 2) >> 1) at the full-sample offset, averaged by pixelavg_pp with the plane of the vector rounded up when it has a quarter part), then
    weightCost (:169-218): weight_pp of the compensated plane, per block min(satd_8x8(reference, source), intra cost), summed in uint32 (intra None: the SATD alone, cache.intraCost
    being what the caller hands in)"""
    M = WEIGHT_MARGIN
    tot = 0
    cu = 0
    for y in range(0, height, 8):
        for x in range(0, width, 8):
            def blk(plane, dx, dy):
                return plane[M + y + dy:M + y + dy + 8, M + x + dx:M + x + dx + 8]
            if mvs is None:
                r = blk(refs[0], 0, 0).copy()
            else:
                qx, qy = mv_clip_luma(mvs[cu], x, y, width, height)
                a = blk(refs[(qy & 2) | ((qx & 2) >> 1)], qx >> 2, qy >> 2).copy()
                if (qx | qy) & 1:
                    qx2, qy2 = qx + (qx & 1), qy + (qy & 1)
                    b = blk(refs[(qy2 & 2) | ((qx2 & 2) >> 1)], qx2 >> 2, qy2 >> 2).copy()
                    r = np.zeros((8, 8), a.dtype)
                    O.lib.orc_pixelavg_pp(1, _ptr(r), C.c_int64(8), _ptr(a), C.c_int64(8), _ptr(b), C.c_int64(8))
                else:
                    r = a
            if cand[0]:
                w = np.zeros((8, 8), r.dtype)
                O.lib.orc_weight_pp(_ptr(r), _ptr(w), C.c_int64(8), 8, 8, cand[1], cand[2], cand[3], cand[4])
                r = w
            v = O.call("satd", 1, r, 8, blk(fenc, 0, 0).copy(), 8)
            tot += min(v, int(intra[cu])) if intra is not None else v
            cu += 1
    return tot & 0xFFFFFFFF


def lowres_paths_compute_ref():
    """every entry of lowres_paths_specs() from the reference (oracle/_ref), in the table's order: the arrays of lowres_paths_golden.npz"""
    out, res, scenes = {}, {}, {}
    for name, spec in lowres_paths_specs().items():
        scene = spec["scene"]
        if scene not in scenes:
            scenes[scene] = lowres_paths_scene(scene)
        c = scenes[scene]
        r = lowres_paths_run_ref(load_ref_with(c["depth"], "lowres_frame_cost_paths"), c, spec, res[spec["src"]] if spec["src"] else None)
        res[name] = r
        for k in ("lowres_costs", "mvs", "mv_costs", "row_satds", "slice_sums"):
            out["%s/%s" % (name, k)] = r[k]
        if scene + "/intra_cost" not in out:
            out[scene + "/intra_cost"] = r["intra_cost"]
        assert np.array_equal(out[scene + "/intra_cost"], r["intra_cost"]), name
    return out


def chroma_weight_inside(x, y, low_cu_w, low_cu_h):
    """mcChroma's condition (weightPrediction.cpp:121): the block's SAMPLE position against the lowres picture's size in blocks"""
    return x < low_cu_w and y < low_cu_h


def chroma_weight_mvs(seed, width, height, low_cu_w):
    """a field as mcChroma indexes it (weightPrediction.cpp:114, :119, :123: mvs[y * lowresWidthInCU + block column], y the block's first sample row): every (x & 7, y & 7)
    fraction class -- none, horizontal, vertical, both --, far vectors, a zero vector"""
    rng = np.random.default_rng(seed)
    n = height * low_cu_w + (width >> 3)
    mv = np.stack([rng.integers(-40, 41, n), rng.integers(-40, 41, n)], 1).astype(np.int16)
    mv[::5] = (mv[::5] >> 3) << 3                  # no fraction
    mv[1::5, 1] = (mv[1::5, 1] >> 3) << 3          # horizontal only
    mv[2::5, 0] = (mv[2::5, 0] >> 3) << 3          # vertical only
    far = np.array([(-3000, 3), (3000, -5), (2, -3000), (-1, 3000)], np.int16)
    for k in range(3, n, 7):
        mv[k] = far[(k // 7) % 4]
    mv[5] = (0, 0)
    return mv


def chroma_weight_cost_expected(O, depth, fenc, ref, stride, width, height, mvs, low_cu_w, low_cu_h, cand):
    """weightAnalyse's chroma measurement (4:2:0) in the reference's order: mcChroma (weightPrediction.cpp:93-159) per 8x8 chroma block -- inside the lowres grid (:121) the vector
    mvs[y * lowresWidthInCU + column] (<< 1, >> the chroma shifts: unchanged), clipped with the CHROMA plane's size (:116-117, :129-131), full-sample offset (mv >> 2), fraction
    (mv & 7) through copy / filter_hpp / filter_vpp / filter_hps + filter_vsp; outside a copy --, then weightCost's chroma branch (:179-191, :213-215): weight_pp, satd_8x8"""
    M = WEIGHT_MARGIN
    dt = fenc.dtype
    tot = 0
    part = PU_SIZES.index((16, 16))             # chroma[csp].pu[LUMA_16x16]: 8x8 chroma samples at 4:2:0
    for y in range(0, height, 8):
        for bx, x in enumerate(range(0, width, 8)):
            if mvs is not None and chroma_weight_inside(x, y, low_cu_w, low_cu_h):
                mx, my = int(mvs[y * low_cu_w + bx][0]), int(mvs[y * low_cu_w + bx][1])
                mx = min(max(mx, (-x - 8) * 4), (width - x - 1 + 8) * 4)
                my = min(max(my, (-y - 8) * 4), (height - y - 1 + 8) * 4)
                ty, tx = M + y + (my >> 2), M + x + (mx >> 2)
                xf, yf = mx & 7, my & 7
                p0 = C.c_void_p(ref.ctypes.data + (ty * stride + tx) * ref.itemsize)
                r = np.zeros((8, 8), dt)
                if not (xf | yf):
                    r = ref[ty:ty + 8, tx:tx + 8].copy()
                elif not yf:
                    O.lib.orc_chroma_hpp(CSP_I420, part, p0, C.c_int64(stride), _ptr(r), C.c_int64(8), xf)
                elif not xf:
                    O.lib.orc_chroma_vpp(CSP_I420, part, p0, C.c_int64(stride), _ptr(r), C.c_int64(8), yf)
                else:
                    immed = np.zeros((8 + 3, 8), np.int16)
                    O.lib.orc_chroma_hps(CSP_I420, part, p0, C.c_int64(stride), _ptr(immed), C.c_int64(8), xf, 1)
                    O.lib.orc_chroma_vsp(CSP_I420, part, C.c_void_p(immed.ctypes.data + 8 * 2), C.c_int64(8), _ptr(r), C.c_int64(8), yf)
            else:
                r = ref[M + y:M + y + 8, M + x:M + x + 8].copy()
            if cand[0]:
                w = np.zeros((8, 8), dt)
                O.lib.orc_weight_pp(_ptr(r), _ptr(w), C.c_int64(8), 8, 8, cand[1], cand[2], cand[3], cand[4])
                r = w
            tot += O.call("satd", 1, r, 8, fenc[M + y:M + y + 8, M + x:M + x + 8].copy(), 8)
    return tot & 0xFFFFFFFF


# ---- adaptive quantisation block energies (x265amd_aq_energy vs LookaheadTLD::acEnergyCu) ----
def aq_case(depth, seed):
    pics, stride, cstride, org = inter_scene(depth, seed, npics=1)
    return dict(depth=depth, pic=pics[0], stride=stride, cstride=cstride, org=org)


def aq_run_ref(R, c, W, H, qg):
    isz = c["pic"].itemsize
    n = ((W + qg - 1) // qg) * ((H + qg - 1) // qg)
    energy = np.zeros(n, np.uint32); wp = np.zeros(6, np.uint64)
    base = c["pic"].ctypes.data
    R.lib.ref_aq_energy.restype = C.c_int
    got = R.lib.ref_aq_energy(*[C.c_void_p(base + c["org"][k] * isz) for k in range(3)], C.c_int64(c["stride"]), C.c_int64(c["cstride"]), W, H, qg, _ptr(energy), _ptr(wp))
    assert got == n
    return energy, wp


def aq_run_hip(L, c, W, H, qg):
    import torch
    isz = c["pic"].itemsize
    d = torch.from_numpy(c["pic"].view(np.uint8)).cuda()
    planes = np.array([d.data_ptr() + c["org"][k] * isz for k in range(3)], np.uint64)
    n = ((W + qg - 1) // qg) * ((H + qg - 1) // qg)
    d_e = torch.zeros(n, dtype=torch.int32, device="cuda"); d_wp = torch.zeros(6, dtype=torch.int64, device="cuda")
    assert L.lib.x265amd_aq_energy(None, _ptr(planes), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), W, H, qg, C.c_void_p(d_e.data_ptr()), C.c_void_p(d_wp.data_ptr())) == 0
    torch.cuda.synchronize()
    return d_e.cpu().numpy().view(np.uint32), d_wp.cpu().numpy().view(np.uint64)


def aq_offsets_ref(R, c, W, H, mode, strength, bias, qg):
    isz = c["pic"].itemsize
    wcu, hcu = ((W // 2) + 7) >> 3, ((H // 2) + 7) >> 3
    n = wcu * hcu * (4 if qg == 8 else 1)
    a = np.zeros(n, np.float64); t = np.zeros(n, np.float64); f = np.zeros(n, np.int32)
    base = c["pic"].ctypes.data
    R.lib.ref_aq_frame.restype = C.c_int
    got = R.lib.ref_aq_frame(*[C.c_void_p(base + c["org"][k] * isz) for k in range(3)], C.c_int64(c["stride"]), C.c_int64(c["cstride"]), W, H, MC_MX, MC_MY, mode,
                             C.c_double(strength), C.c_double(bias), qg, _ptr(a), _ptr(t), _ptr(f))
    assert got == n, (got, n)
    return a, t, f


def aq_offsets_prod(L, energy, avg_count, mode, strength, bias, qg):
    n = len(energy)
    a = np.zeros(n, np.float64); t = np.zeros(n, np.float64); f = np.zeros(n, np.int32)
    rc = L.lib.x265amd_aq_offsets(_ptr(np.ascontiguousarray(energy)), n, avg_count, mode, C.c_double(strength), C.c_double(bias), qg, _ptr(a), _ptr(t), _ptr(f))
    assert rc == 0
    return a, t, f


# ---- x265amd_intra_pu: scan + candidate list + candidate chains of one prediction unit as one launch ----
INTRA_PU_JOB_DT = np.dtype([("tmpl", INTRA_TU_JOB_DT), ("lambda", "<u8"), ("rbits", "<u4"), ("mpm_base", "<u4"), ("slot_pixels", "<u4"), ("slot_coeffs", "<u4"),
                            ("preds", "u1", 3), ("max_cand", "u1"), ("reserved", "u1", 4)])
INTRA_PU_OUT_DT = np.dtype([("sa8d", "<i4", 35), ("num_cand", "<u4"), ("modes", "u1", 16)])
assert INTRA_PU_JOB_DT.itemsize == 128 and INTRA_PU_OUT_DT.itemsize == 160


def intra_pu_candidates(sa8d, preds, rbits, mpm_base, lam, max_cand):
    """Search::estIntraPredQT's candidate list (search.cpp:1615-1650 with updateCandList :3953-3972) on given SA8D costs: the modes in list order"""
    kmax = (1 << 64) - 1
    cost = []
    for m in range(35):
        b = rbits
        for i in range(3):
            if preds[i] == m:
                b = mpm_base + (1 if m == preds[0] else 2)
                break
        cost.append(int(sa8d[m]) + ((b * lam + 128) >> 8))
    bcost = min(cost)
    padded = bcost + (bcost >> 2)
    lst, modes = [kmax] * max_cand, [0] * max_cand
    for m in range(35):
        if cost[m] < padded or m == preds[0]:
            mi, mv = 0, 0
            for i in range(max_cand):
                if mv < lst[i]:
                    mv, mi = lst[i], i
            if cost[m] < mv:
                lst[mi], modes[mi] = cost[m], m
    n = 0
    while n < max_cand and lst[n] != kmax:
        n += 1
    return modes[:n]


def intra_pu_run_hip(L, c, preds, rbits, mpm_base, lam, max_cand):
    """x265amd_intra_pu on one luma block of intra_tu_cases (ttype 0): returns (sa8d[35], modes, [(stats, pred, recon, coeff, resi)] per candidate)"""
    import torch
    dt = c["plane"].dtype
    isz = dt.itemsize
    N = 1 << c["log2"]
    d_plane = torch.from_numpy(c["plane"].view(np.uint8).copy()).cuda()
    d_fenc = torch.from_numpy(np.ascontiguousarray(c["fenc"]).ravel().view(np.uint8).copy()).cuda()
    slot_pixels, slot_coeffs = 2048, 1024
    d_cand = torch.zeros(16 * slot_pixels * isz, dtype=torch.uint8, device="cuda")          # per candidate: recon at 0, pred at 1024 samples (stride N), as the intra RD lays them out
    d_coeff = torch.zeros(16 * slot_coeffs * 2, dtype=torch.uint8, device="cuda")
    d_resi = torch.zeros(16 * slot_coeffs * 2, dtype=torch.uint8, device="cuda")
    job = np.zeros(1, INTRA_PU_JOB_DT)
    mask = 0
    for u, f in enumerate(c["flags"]):
        mask |= int(f) << u
    job[0]["tmpl"]["tu"] = (d_fenc.data_ptr(), d_cand.data_ptr() + 1024 * isz, d_coeff.data_ptr(), d_resi.data_ptr(), d_cand.data_ptr(), N, N, N, N,
                            c["log2"], 0, 1, 0, c["slice"], c["qp"], c["signhide"], 0)
    job[0]["tmpl"]["nb"] = d_plane.data_ptr() + c["off"] * isz
    job[0]["tmpl"]["avail"], job[0]["tmpl"]["nb_stride"], job[0]["tmpl"]["strong"] = mask, c["stride"], c["strong"]
    job[0]["lambda"], job[0]["rbits"], job[0]["mpm_base"], job[0]["slot_pixels"], job[0]["slot_coeffs"] = lam, rbits, mpm_base, slot_pixels, slot_coeffs
    job[0]["preds"], job[0]["max_cand"] = preds, max_cand
    d_job = torch.from_numpy(job.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(INTRA_PU_OUT_DT.itemsize, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(16 * TU_RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    assert L.lib.x265amd_intra_pu(None, C.c_void_p(d_job.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_void_p(d_res.data_ptr())) == 0
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(INTRA_PU_OUT_DT)[0]
    res = d_res.cpu().numpy().view(TU_RESULT_DT)
    cand, coeff, resi = d_cand.cpu().numpy().view(dt), d_coeff.cpu().numpy().view(np.int16), d_resi.cpu().numpy().view(np.int16)
    per = []
    for i in range(int(out["num_cand"])):
        recon = cand[i * slot_pixels:i * slot_pixels + N * N].reshape(N, N).copy()
        pred = cand[i * slot_pixels + 1024:i * slot_pixels + 1024 + N * N].reshape(N, N).copy()
        st = (int(res[i]["num_sig"]), int(res[i]["zero_dist"]), int(res[i]["zero_energy"]), int(res[i]["nz_dist"]), int(res[i]["nz_energy"]))
        per.append((st, pred, recon, coeff[i * slot_coeffs:i * slot_coeffs + N * N].copy(), resi[i * slot_coeffs:i * slot_coeffs + N * N].reshape(N, N).copy()))
    return out["sa8d"].copy(), [int(m) for m in out["modes"][:int(out["num_cand"])]], per


# ---- x265amd_intra_nxn: an 8x8 NxN CU (four 4x4 luma units with their decisions, the luma measurements, the chroma decision) as one launch ----
INTRA_NXN_JOB_DT = np.dtype([("tmpl", INTRA_TU_JOB_DT, 4), ("pred_dst", "<u8", 4), ("layer_dst", "<u8", 4), ("lambda", "<u8"), ("lambda2", "<u8"), ("psy_scale", "<u8"),
                             ("frac_start", "<u8", 4), ("scan_frac", "<u4"), ("slot_pixels", "<u4"), ("slot_coeffs", "<u4"), ("left_mode", "u1", 2), ("above_mode", "u1", 2),
                             ("ctx", "u1", 160), ("max_cand", "u1"), ("do_chroma", "u1"), ("reserved", "u1", 2), ("pad", "u1", 4), ("ctmpl", INTRA_TU_JOB_DT, 2), ("crecon_dst", "<u8", 2), ("recon_dst", "<u8", 4), ("levels_dst", "<u8"), ("clevels_dst", "<u8"),
                             ("chain", "<u8"), ("peer", "<u8"), ("cu_out", "<u8"), ("peer_recon", "<u8", 3), ("win_dst", "<u8", 3), ("chain_token", "<u8"), ("chain_role", "u1"),
                             ("chain_first", "u1"), ("mode_src", "u1", 4), ("chain_index", "u1"), ("reserved2", "u1"),
                             ("rdoq_lambda2", "<i8", 3), ("rdoq_lambda", "<i4", 3), ("psy_rdoq_scale", "<i4"), ("rdoq_level", "u1"), ("rdoq_tu_depth", "u1"), ("rdoq_general", "u1"), ("reserved3", "u1", 5)])
INTRA_CHAIN_DT = np.dtype([("seq", "<u8"), ("frac", "<u8"), ("ctx", "u1", 160), ("mode", "u1", (4, 4))])
INTRA_CU8_RESULT_DT = np.dtype([("rd_cost", "<u8"), ("frac_bits", "<u8"), ("other_cost", "<u8"), ("total_bits", "<u4"), ("mv_bits", "<u4"), ("coeff_bits", "<u4"), ("psy_energy", "<u4"),
                                ("res_energy", "<u4"), ("luma_dist", "<u4"), ("chroma_dist", "<u4"), ("status", "<u4"), ("part_size", "u1"), ("chroma_dir", "u1"), ("cbf_u", "u1"),
                                ("cbf_v", "u1"), ("luma_dir", "u1", 4), ("cbf_y", "u1", 4), ("reserved", "u1", 4), ("ctx", "u1", 160), ("levels", "<i2", 96)])
INTRA_NXN_OUT_DT = np.dtype([("mode", "u1", 4), ("num_cand", "u1", 4), ("res", TU_RESULT_DT, 4), ("levels", "<i2", (4, 16)), ("psy_energy", "<u4"), ("res_energy", "<u4"),
                             ("chroma_best", "<u4"), ("chroma_reserved", "<u4"), ("cres", TU_RESULT_DT, 2), ("clevels", "<i2", (2, 16))])
assert INTRA_NXN_JOB_DT.itemsize == 1080 and INTRA_NXN_OUT_DT.itemsize == 408 and INTRA_CU8_RESULT_DT.itemsize == 424 and INTRA_CHAIN_DT.itemsize == 192


def entropy_bit_tables():
    """(bits[128], lpsNext[64]) of the CABAC estimator, read from the product's own header (the tables are the standard's: H.265 9.3.4.3, entropy.cpp:2627-2700)"""
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "x265-amod_amd", "csrc", "entropy_dev.h")).read()
    def table(name):
        body = src[src.index(name):]
        body = body[body.index("{") + 1:body.index("};")]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", body)]
    return table("en_bits[128]"), table("en_lpsNext[64]")


def cabac_next_state(state, bin_, lps_next):
    p, mps = state >> 1, state & 1
    if p == 63:
        return state
    if bin_ == mps:
        return ((p + 1 if p < 62 else 62) << 1) | mps
    if p == 0:
        return 1 - mps
    return (lps_next[p] << 1) | mps


def luma_mpm(left, above):
    """getIntraDirLumaPredictor (cudata.cpp:910-953) on the two neighbour modes"""
    if left == above:
        return [left, ((left - 2 + 31) & 31) + 2, ((left - 2 + 1) & 31) + 2] if left >= 2 else [0, 1, 26]
    return [left, above, 0 if (left and above) else (26 if left + above < 2 else 1)]


# ---- the rate control's own options around the preset (tests/test_encoder_api.py): small clips (cut CTUs right and below, the clip's scene change at 24), the reference's
# command line = --preset medium + the options + PRESET_CLI ----
RC_CASES = {
    "rc_crf20/": ((416, 240), 30, 8, 2, dict(PRESET_BASE, rfConstant=20.0), ["--preset", "medium", "--crf", "20"]),
    "rc_crf36/": ((416, 240), 30, 8, 2, dict(PRESET_BASE, rfConstant=36.0), ["--preset", "medium", "--crf", "36"]),
    "rc_no_cutree/": ((416, 240), 30, 8, 2, dict(PRESET_BASE, cuTree=0), ["--preset", "medium", "--no-cutree"]),                 # the blurred-complexity branch: QPs follow the estimates
    "rc_no_cutree_qcomp/": ((448, 256), 30, 8, 2, dict(PRESET_BASE, cuTree=0, qCompress=0.8, bframes=2), ["--preset", "medium", "--no-cutree", "--qcomp", "0.8", "--bframes", "2"]),
    "rc_aq1/": ((416, 240), 26, 8, 2, dict(PRESET_BASE, aqMode=1), ["--preset", "medium", "--aq-mode", "1"]),
    "rc_aq3_strength/": ((416, 240), 26, 8, 2, dict(PRESET_BASE, aqMode=3, aqStrength=1.5), ["--preset", "medium", "--aq-mode", "3", "--aq-strength", "1.5"]),
    "rc_qg64/": ((448, 256), 26, 8, 2, dict(PRESET_BASE, qgSize=64), ["--preset", "medium", "--qg-size", "64"]),
    "rc_qcomp_strength/": ((416, 240), 26, 8, 2, dict(PRESET_BASE, qCompress=0.8), ["--preset", "medium", "--qcomp", "0.8"]),   # cuTree's strength 5 (1 - qcomp)
    "rc_no_bframes/": ((416, 240), 26, 8, 2, dict(PRESET_BASE, bframes=0), ["--preset", "medium", "--bframes", "0"]),
    "rc_no_pyramid_keyint/": ((416, 240), 30, 8, 2, dict(PRESET_BASE, bBPyramid=0, keyframeMax=12, keyframeMin=12), ["--preset", "medium", "--no-b-pyramid", "--keyint", "12", "--min-keyint", "12"]),
    "rc_closed_gop/": ((416, 240), 30, 8, 2, dict(PRESET_BASE, bOpenGOP=0, keyframeMax=10, keyframeMin=5), ["--preset", "medium", "--no-open-gop", "--keyint", "10", "--min-keyint", "5"]),
    "rc_slow_hbd/": ((416, 240), 20, 10, 4, dict(PRESET_BASE, **SLOW_TOOLS), ["--preset", "slow"]),
    "rc_rd5/": ((416, 240), 14, 8, 2, dict(PRESET_BASE, rdLevel=5), ["--preset", "medium", "--rd", "5"]),                      # compressInterCU_rd5_6 with delta QP
    "rc_rd2/": ((416, 240), 14, 8, 2, dict(PRESET_BASE, rdLevel=2), ["--preset", "medium", "--rd", "2"]),
    # QPs above 51: the B pictures' rate-control QP passes 51 and the block offsets push CUs further -- the lambdas follow the QP asked for (up to 69), the quantiser
    # and the coded QP stop at 51 (Search::setLambdaFromQP, search.cpp:177-187)
    "rc_crf46/": ((416, 240), 30, 8, 2, dict(PRESET_BASE, rfConstant=46.0), ["--preset", "medium", "--crf", "46"]),
    "rc_crf51_aq3/": ((448, 256), 26, 8, 2, dict(PRESET_BASE, rfConstant=51.0, aqMode=3, aqStrength=2.0), ["--preset", "medium", "--crf", "51", "--aq-mode", "3", "--aq-strength", "2.0"]),
    "rc_crf44_hbd_slow/": ((416, 240), 20, 10, 4, dict(PRESET_BASE, rfConstant=44.0, **SLOW_TOOLS), ["--preset", "slow", "--crf", "44"]),
    # cuTree WITHOUT adaptive quantisation (Encoder::configure keeps aq-mode on at strength 0: zero offsets, delta QP from cuTree alone, encoder.cpp:3730-3734; slicetype.cpp:483-505):
    # --tune psnr (aq-strength 0, no psy-rd), --aq-mode 0; and neither: plain constant rate factor, no delta QP at all
    "rc_tune_psnr/": ((416, 240), 26, 8, 2, dict(PRESET_BASE, aqStrength=0.0, psyRd=0.0), ["--preset", "medium", "--tune", "psnr"]),
    "rc_aq0_cutree/": ((416, 240), 26, 8, 2, dict(PRESET_BASE, aqMode=0), ["--preset", "medium", "--aq-mode", "0"]),
    "rc_plain_crf/": ((448, 256), 26, 8, 2, dict(PRESET_BASE, aqMode=0, cuTree=0), ["--preset", "medium", "--aq-mode", "0", "--no-cutree"]),
    # the other tunes whose members the encoder reads (param.cpp:586-649)
    "rc_tune_ssim/": ((416, 240), 26, 8, 2, dict(PRESET_BASE, psyRd=0.0), ["--preset", "medium", "--tune", "ssim"]),
    "rc_tune_fastdecode/": ((416, 240), 26, 8, 2, dict(PRESET_BASE, bEnableLoopFilter=0, bEnableSAO=0, bEnableWeightedPred=0, bIntraInBFrames=0), ["--preset", "medium", "--tune", "fastdecode"]),
    "rc_ft1/": ((416, 240), 26, 8, 2, dict(PRESET_BASE, frameNumThreads=1), ["--preset", "medium", "--frame-threads", "1"]),       # one frame thread WITH wavefronts: SAO's switch-off by the picture before (sao.cpp:264)
    "rc_tune_zerolatency/": ((416, 240), 26, 8, 2, dict(PRESET_BASE, bFrameAdaptive=0, bframes=0, lookaheadDepth=0, scenecutThreshold=0, cuTree=0, frameNumThreads=1),
                             ["--preset", "medium", "--tune", "zerolatency"]),
}


# ---- the in-loop filters by columns: schedules for x265amd_filter_plan (host/filter_plan.cpp) and one combined picture per geometry ----
FILTER_STEP_DT = np.dtype([(n, "<i4") for n in ("kind", "row", "col_begin", "col_end", "y4_begin", "y4_end", "rec_y4_end", "rec_x4_begin", "rec_x4_end")])
FILTER_FINISH_DT = np.dtype([(n, "<i4") for n in ("row", "x_begin", "x_end", "y_begin", "y_end")])
FILTER_TOP, FILTER_FULL = 0, 1
FILTER_SCHEDULES = ("wavefront", "raster", "all", "single")
FILTER_MARGIN = (96, 80)            # the encoder's luma margins (chroma: half)
SAO_CARRY_BYTES = 160 + 8           # X265AMD_CTX_STRIDE + 8 (include/x265amd.h: x265amd_sao_rdo_cols)


def filter_schedule(kind, seed, ctuW, ctuH, max_step=None):
    """a seeded sequence of snapshots of a picture's analysis (analysedCols[r] per CTU row, monotone, the last one complete):
    wavefront -- row r is never ahead of analysedCols[r - 1] - 1 unless the row above is complete, random increments of up to max_step CTUs (2 * ctuW unless
                 given) per snapshot (what the encoder's rows do);
    raster    -- a row completes before the next begins, random increments;
    all       -- everything analysed before the filter first looks;
    single    -- one CTU per snapshot, in wavefront order."""
    rng = np.random.default_rng(seed)
    a = [0] * ctuH
    out = []

    def eligible():
        return [r for r in range(ctuH) if a[r] < ctuW and (r == 0 or a[r - 1] == ctuW or a[r] + 1 <= a[r - 1] - 1)]

    if kind == "all":
        return [[ctuW] * ctuH]
    if kind == "raster":
        for r in range(ctuH):
            while a[r] < ctuW:
                a[r] = min(ctuW, a[r] + int(rng.integers(1, ctuW + 1)))
                out.append(list(a))
        return out
    if kind == "single":
        while any(v < ctuW for v in a):
            for r in eligible():            # one pass down the wavefront, a snapshot per CTU
                a[r] += 1
                out.append(list(a))
        return out
    assert kind == "wavefront", kind
    while any(v < ctuW for v in a):
        for _ in range(int(rng.integers(1, (max_step or 2 * ctuW) + 1))):
            el = eligible()
            if not el:
                break
            a[el[int(rng.integers(0, len(el)))]] += 1
        out.append(list(a))
    return out


def filter_min_chunks(m, ctuW):
    """(min_chunk, min_chunk_last) of filterRowsCols for three values of the chunk minimum: 1 (the planner's smallest; the encoder does not use it), 2 (P pictures: 1 in the last three
    rows), 'w' (B pictures: whole rows)"""
    return {1: (1, 1), 2: (2, 1), "w": (ctuW, ctuW)}[m]


def filter_sweeps(L, width, height, schedule, min_chunk, min_chunk_last, early_top):
    """the sweeps the filter thread of a picture takes for a sequence of snapshots: x265amd_filter_plan after every snapshot for as long as it returns steps
    (x265amd_filter_ready must say the same).  Each sweep: dict(steps, finish, pub_x (after the sweep), analysed)."""
    ctuW, ctuH = (width + 63) // 64, (height + 63) // 64
    done_top, done_full, pub_x = (np.zeros(ctuH, np.int32) for _ in range(3))
    steps = np.zeros(2 * ctuH, FILTER_STEP_DT); finish = np.zeros(ctuH, FILTER_FINISH_DT)
    ns, nf = C.c_int(0), C.c_int(0)
    out = []
    for snap in schedule:
        an = np.array(snap, np.int32)
        while True:
            all_done = bool((done_full == ctuW).all())
            ready = L.lib.x265amd_filter_ready(width, height, _ptr(an), _ptr(done_top), _ptr(done_full), min_chunk, min_chunk_last, early_top)
            rc = L.lib.x265amd_filter_plan(width, height, _ptr(an), _ptr(done_top), _ptr(done_full), _ptr(pub_x), min_chunk, min_chunk_last, early_top,
                                           _ptr(steps), C.byref(ns), _ptr(finish), C.byref(nf))
            assert rc == 0, rc
            assert ready == int(ns.value > 0 or all_done), (ready, ns.value, all_done, snap)
            if ns.value == 0:
                assert nf.value == 0
                break
            out.append(dict(steps=steps[:ns.value].copy(), finish=finish[:nf.value].copy(), pub_x=pub_x.copy(), analysed=list(snap)))
    assert (done_top == ctuW).all() and (done_full == ctuW).all() and (pub_x == width).all(), (done_top, done_full, pub_x)
    return out


def filter_case(depth, seed, width, height, slice_b=True, bypass=False):
    """one picture for the column forms of the in-loop filters: deblock_case's coding tree, records and blocky planes re-laid into planes with the encoder's margins
    (the margins poisoned with a valid sample value: nothing may read them), a source picture derived from the unfiltered picture (as sao_case derives fenc from
    rec) so that the SAO decision really switches offsets on, and cabac_case's si / units for the decision."""
    c = deblock_case(depth, seed, width, height, slice_b=slice_b, bypass=bypass)
    rng = np.random.default_rng(seed + 7777)
    pmax = (1 << depth) - 1
    dt = c["planes"][0].dtype
    poison = 0xA5 if depth == 8 else 0x2A5
    mx, my = FILTER_MARGIN
    stride, cstride = width + 2 * mx, width // 2 + mx
    rec, fenc = [], []
    for k, (w, h, st, ax, ay, om) in enumerate(((width, height, stride, mx, my, 16), (width // 2, height // 2, cstride, mx // 2, my // 2, 8), (width // 2, height // 2, cstride, mx // 2, my // 2, 8))):
        pic = c["planes"][k][om:om + h, om:om + w].astype(np.int64)
        full = np.full((h + 2 * ay, st), poison, dt)
        full[ay:ay + h, ax:ax + w] = pic
        src = np.zeros((h + 2 * ay, st), dt)
        # the source: the unfiltered picture pulled halfway towards its local mean (local extremes are what the edge offsets correct) plus small noise
        e = np.pad(pic, 1, mode="edge")
        mean = (e[:-2, 1:-1] + e[2:, 1:-1] + e[1:-1, :-2] + e[1:-1, 2:] + 2) >> 2
        src[ay:ay + h, ax:ax + w] = np.clip(pic + ((mean - pic) >> 1) + rng.integers(-2, 3, pic.shape) * (1 << (depth - 8)), 0, pmax)
        rec.append(full); fenc.append(src)
    cab = cabac_case(seed, width, height, 0 if slice_b else 1)
    return dict(c, rec=rec, fenc=fenc, stride=stride, cstride=cstride, org=(my * stride + mx, (my // 2) * cstride + mx // 2), margin=(mx, my), poison=poison,
                si=np.array([cab["si"]], SLICE_INFO_DT), cu_units=np.ascontiguousarray(cab["units"].reshape(-1)), referenced=int(not slice_b),
                ctuW=(width + 63) // 64, ctuH=(height + 63) // 64, nctu=((width + 63) // 64) * ((height + 63) // 64))


def filter_case_expected(O, P, c):
    """the picture through the picture-wide forms on the CPU: the oracle's deblocking, statistics, offsets and borders; the product's host decision (x265amd_sao_rdo with
    two frame threads) in between.  Returns dict(D, count, org, params, F)."""
    w, h = c["width"], c["height"]
    D = [p.copy() for p in c["rec"]]
    O.lib.orc_deblock_picture(_ptr(_plane_ptrs(D, c["org"])), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), w, h, _ptr(c["units"]),
                              c["beta"], c["tc"], c["cb"], c["cr"], c["bypass"], 3)
    n = c["nctu"] * 3 * 5 * 32
    cnt = np.zeros(n, np.int32); org = np.zeros(n, np.int32)
    O.lib.orc_sao_stats_picture(_ptr(_plane_ptrs(D, c["org"])), _ptr(_plane_ptrs(c["fenc"], c["org"])), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), w, h, _ptr(cnt), _ptr(org))
    params = np.zeros(c["nctu"], SAO_CTU_DT); flags = np.zeros(2, np.int32); rate = np.zeros(8, np.float64)
    P.lib.x265amd_sao_rdo.argtypes = None
    assert P.lib.x265amd_sao_rdo(_ptr(c["si"]), c["referenced"], 2, 0, 69, _ptr(c["cu_units"].copy()), _ptr(cnt), _ptr(org), _ptr(rate), _ptr(params), _ptr(flags)) == 0
    F = [np.full_like(p, c["poison"]) for p in c["rec"]]
    O.lib.orc_sao_apply_picture(_ptr(_plane_ptrs(D, c["org"])), _ptr(_plane_ptrs(F, c["org"])), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), w, h, _ptr(params))
    mx, my = c["margin"]
    for k, f in enumerate(F):
        sh = 1 if k else 0
        O.lib.orc_extend_pic_border(off(f.reshape(-1), c["org"][1 if k else 0]), C.c_int64(c["cstride"] if k else c["stride"]), w >> sh, h >> sh, mx >> sh, my >> sh)
    return dict(D=D, count=cnt, org=org, params=params, F=F)


# ---- the in-loop filter kernels at partial CTUs and parameter extremes (tests/test_filter_edges.py) ----
# every partial extent from 8 to 56 in both directions on 2x2 CTUs, three CTU columns with a 24-sample tail, pictures smaller than a CTU
EDGE_GEOMETRIES_2X2 = ((72, 120), (80, 112), (88, 104), (96, 96), (104, 88), (112, 80), (120, 72))
EDGE_GEOMETRIES = EDGE_GEOMETRIES_2X2 + ((152, 24),) + ((8, 8), (16, 8), (8, 16), (24, 40), (40, 24), (56, 56), (64, 8), (8, 64))
DB_TC_TABLE = (0,) * 18 + (1,) * 9 + (2,) * 4 + (3,) * 4 + (4,) * 3 + (5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24)       # H.265 table 8-12
assert len(DB_TC_TABLE) == 54


def edge_poison(depth):
    return 0xA5 if depth == 8 else 0x2A5


def edge_frame(depth, width, height, pics):
    """three picture-sized arrays (Y, U, V) laid into planes with the encoder's margins, the margins poisoned with a valid sample value: (planes, stride, cstride, org)"""
    dt = np.uint8 if depth == 8 else np.uint16
    mx, my = FILTER_MARGIN
    stride, cstride = width + 2 * mx, width // 2 + mx
    planes = []
    for k, pic in enumerate(pics):
        sh = 1 if k else 0
        assert pic.shape == (height >> sh, width >> sh) and pic.min() >= 0 and pic.max() < (1 << depth)
        full = np.full(((height >> sh) + 2 * (my >> sh), cstride if k else stride), edge_poison(depth), dt)
        full[my >> sh:(my + height) >> sh, mx >> sh:(mx + width) >> sh] = pic
        planes.append(full)
    return planes, stride, cstride, (my * stride + mx, (my // 2) * cstride + mx // 2)


def edge_picture(planes, width, height, k):
    """the picture area of padded plane k"""
    mx, my = FILTER_MARGIN
    sh = 1 if k else 0
    return planes[k][my >> sh:(my + height) >> sh, mx >> sh:(mx + width) >> sh]


def edge_margins_intact(depth, planes, width, height, what):
    """nothing outside the picture was written: the margins still hold the poison"""
    for k, p in enumerate(planes):
        m = p != edge_poison(depth)
        edge_picture([m] * 3, width, height, k)[:] = False
        if m.any():
            ys, xs = np.nonzero(m)
            raise AssertionError("%s: plane %d: %d margin samples written, first at x %d y %d: %d" % (
                what, k, len(ys), xs[0] - (FILTER_MARGIN[0] >> (1 if k else 0)), ys[0] - (FILTER_MARGIN[1] >> (1 if k else 0)), p[ys[0], xs[0]]))


def edge_first_diff(got, want, k):
    """for an assertion message: where two padded planes first differ, in picture coordinates"""
    ys, xs = np.nonzero(got != want)
    sh = 1 if k else 0
    return "plane %d: first of %d at x %d y %d: %d, want %d" % (k, len(ys), xs[0] - (FILTER_MARGIN[0] >> sh), ys[0] - (FILTER_MARGIN[1] >> sh), got[ys[0], xs[0]], want[ys[0], xs[0]])


def edge_content(depth, rng, width, height, mode, qp_range=(18, 46), tc_offset=0):
    """three picture-sized int64 arrays:
    blocky    -- deblock_case's: 8x8 blocks in the middle third of the range with small noise;
    saturated -- 8x8 blocks at levels from {0 .. 3} or {pmax - 3 .. pmax} (the range end chosen per 24x24 area, so most edges lie between nearly equal levels at one
                 end), noise of +-1 << (depth - 8): filter results and offset sums reach and would pass 0 and pmax;
    saturated_rough -- the same with noise of every integer up to +-3 << (depth - 8).  With +-1 at 8 bits the normal and chroma filters' sums only reach the ends of the
                 range: a sample at pmax moves up only if the second sample behind the edge lies three (chroma: four) below the second before it, and the sample next
                 to it then cannot be at pmax as well when a block spans two levels;
    stepped   -- level = a walk along x plus a walk along y over the 8x8 grid, so every edge of a grid column (row) sees the same step: tc, 5 tc / 2, 10 tc or 27 tc (+-1) for
                 the tc of a QP drawn from qp_range.  For flat sides the normal filter's delta is (6 step + 8) >> 4: the strong / normal decision turns at a step of
                 5 tc / 2, the clip of delta at 8 tc / 3, the cut abs(delta) < 10 tc at 80 tc / 3.  Noise of every integer up to an amplitude drawn per block from
                 1 .. 6 << (depth - 8): the second differences then reach 4 to 24 << (depth - 8) a line, so the activity of an edge falls on both sides of beta, beta / 4,
                 beta / 8 and 3 beta / 16 at every QP up to beta's last entry, and at 10 bits not only on multiples of four;
    noise     -- smoothed uniform noise (sao_case's);
    flat      -- one level per plane;
    checker   -- a one-sample checkerboard between two levels: local minima and maxima only."""
    pmax, scale = (1 << depth) - 1, 1 << (depth - 8)
    out = []
    for k in range(3):
        w, h = (width >> 1, height >> 1) if k else (width, height)
        bw, bh = (w + 7) // 8, (h + 7) // 8
        up = lambda lv, n=8: np.kron(lv, np.ones((n, n), np.int64))
        if mode == "blocky":
            p = up(rng.integers(0, pmax + 1, (bh, bw)))[:h, :w] // 3 + pmax // 3 + rng.integers(-2, 3, (h, w)) * scale
        elif mode in ("saturated", "saturated_rough"):
            high = up(rng.integers(0, 2, ((bh + 2) // 3, (bw + 2) // 3)), 3)[:bh, :bw]
            lv = rng.integers(0, 4, (bh, bw))
            noise = rng.integers(-1, 2, (h, w)) * scale if mode == "saturated" else rng.integers(-3 * scale, 3 * scale + 1, (h, w))
            p = up(np.where(high == 1, pmax - lv, lv))[:h, :w] + noise
        elif mode == "stepped":
            def walk(n):
                v, pos = np.zeros(n, np.int64), 0
                for i in range(1, n):
                    tc = DB_TC_TABLE[min(53, max(0, int(rng.integers(*qp_range)) + tc_offset))] * scale
                    sign = 1 if rng.integers(0, 2) else -1
                    for mult in rng.permutation(4):
                        step = (tc, (5 * tc) // 2, 10 * tc, 27 * tc)[mult] + int(rng.integers(-1, 2)) * scale
                        for s in (sign, -sign):
                            if abs(pos + s * step) <= pmax // 4:
                                break
                        else:
                            continue
                        pos += s * step
                        break
                    v[i] = pos
                return v
            amp = up(rng.integers(1, 7, (bh, bw)))[:h, :w] * scale
            p = pmax // 2 + up(walk(bw)[None, :] + walk(bh)[:, None])[:h, :w] + rng.integers(-amp, amp + 1)
        elif mode == "noise":
            full = rng.integers(0, pmax + 1, (h, w))
            p = (full + np.roll(full, 1, 0) + np.roll(full, 1, 1) + np.roll(full, -1, 0)) // 4
            if rng.integers(0, 2):
                p = (p // 8) * 8 + rng.integers(0, 3, p.shape)
        elif mode == "flat":
            p = np.full((h, w), int(rng.integers(0, pmax + 1)), np.int64)
        elif mode == "checker":
            lo = int(rng.integers(0, pmax))
            hi = int(rng.integers(lo + 1, pmax + 1))
            yy, xx = np.mgrid[0:h, 0:w]
            p = np.where((xx + yy) & 1, hi, lo)
        else:
            raise ValueError(mode)
        out.append(np.clip(p, 0, pmax).astype(np.int64))
    return out


def deblock_edge_case(depth, seed, width, height, slice_b=True, bypass=False, qp_range=(18, 46), content="blocky", offsets=None):
    """deblock_case's coding tree and records (QP per CU from qp_range) under planes with the encoder's margins, poisoned; the picture's content by edge_content from a
    generator of its own; offsets: (beta / 2, tc / 2, Cb, Cr) of the PPS instead of deblock_case's draw from the narrow ranges"""
    c = deblock_case(depth, seed, width, height, slice_b=slice_b, bypass=bypass, qp_range=qp_range)
    if offsets is not None:
        c["beta"], c["tc"], c["cb"], c["cr"] = offsets
    rng = np.random.default_rng(seed + 424242)
    planes, stride, cstride, org = edge_frame(depth, width, height, edge_content(depth, rng, width, height, content, qp_range, 2 * c["tc"]))
    return dict(c, planes=planes, stride=stride, cstride=cstride, org=org, content=content, depth=depth)


def deblock_index_clips(c):
    """how often the table indices of the edges between an intra unit and its left or upper neighbour (strength 2 whatever the motion) leave their ranges, from QP + offset:
    dict(beta_lo, beta_hi, tc_lo, tc_hi: luma; cqp_hi: the min(qp - 6, 51) of the chroma QP mapping fired, ctc_lo, ctc_hi: the chroma tc index)"""
    w4, h4 = c["width"] // 4, c["height"] // 4
    u = c["units"].reshape(h4, w4)
    n = dict(beta_lo=0, beta_hi=0, tc_lo=0, tc_hi=0, cqp_hi=0, ctc_lo=0, ctc_hi=0)
    for d, (tu, dy, dx) in enumerate(((DB_TU_LEFT, 0, 1), (DB_TU_TOP, 1, 0))):
        for y4 in range(2 * dy, h4, 1 + dy):
            for x4 in range(2 * dx, w4, 1 + dx):
                q, p = u[y4, x4], u[y4 - dy, x4 - dx]
                if not (q["flags"] & tu) or not ((q["flags"] | p["flags"]) & DB_INTRA) or (c["bypass"] and (q["flags"] & p["flags"] & DB_BYPASS)):
                    continue
                qp = (int(p["qp"]) + int(q["qp"]) + 1) >> 1
                b, t = qp + 2 * c["beta"], qp + 2 + 2 * c["tc"]
                n["beta_lo"] += b < 0; n["beta_hi"] += b > 51; n["tc_lo"] += t < 0; n["tc_hi"] += t > 53
                across, along = (x4, y4) if d == 0 else (y4, x4)
                if across & 3 or along & 1:
                    continue
                for o in (c["cb"], c["cr"]):
                    cq = qp + o
                    n["cqp_hi"] += cq - 6 > 51
                    cq = cq if cq < 30 else ((29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37)[cq - 30] if cq < 44 else min(cq - 6, 51))
                    n["ctc_lo"] += cq + 2 + 2 * c["tc"] < 0; n["ctc_hi"] += cq + 2 + 2 * c["tc"] > 53
    return n


def deblock_strength_rows():
    """the boundary-strength table of H.265 8.7.2.4 as (what, edge kind, unit P, unit Q, strength): 'tu' -- P and Q are 8x8 CUs without further split, the edge between
    them a transform edge; 'pu' -- the two prediction units of one 16x16 CU with a single transform unit.  Picture identities per list, vectors in quarter samples."""
    A, B, Z = (8, -4), (-5, 9), (0, 0)
    U = lambda ref=(0, 1), mv=(A, B), intra=0, cbf=0: dict(ref=ref, mv=mv, intra=intra, cbf=cbf)
    add = lambda v, d: (v[0] + d[0], v[1] + d[1])
    rows = []
    for lst in (0, 1):
        for axis in (0, 1):
            for dist, bs in ((3, 0), (4, 1)):
                d = (dist, 0) if axis == 0 else (0, -dist)
                rows.append(("same pictures in the same order, list %d differs by %d in %s" % (lst, dist, "xy"[axis]), "tu", U(), U(mv=(add(A, d), B) if lst == 0 else (A, add(B, d))), bs))
    one = lambda mv: U(ref=(2, 2), mv=mv)
    rows += [
        ("swapped lists, crosswise 3 apart, straight far", "tu", U(), U(ref=(1, 0), mv=(add(B, (3, 0)), add(A, (0, -3)))), 0),
        ("swapped lists, crosswise 4 apart in y on one list", "tu", U(), U(ref=(1, 0), mv=(add(B, (0, 4)), A)), 1),
        ("swapped lists, crosswise far, straight 3 apart", "tu", U(), U(ref=(1, 0), mv=(add(A, (3, 0)), add(B, (0, 3)))), 1),
        ("one picture on both lists, straight near, crosswise near", "tu", one(((8, -4), (9, -3))), one(((10, -3), (8, -2))), 0),
        ("one picture on both lists, straight near, crosswise far", "tu", one((A, B)), one((add(A, (3, 0)), add(B, (0, -3)))), 0),
        ("one picture on both lists, straight far, crosswise near", "tu", one((A, B)), one((add(B, (3, 0)), add(A, (0, 3)))), 0),
        ("one picture on both lists, straight far (4 on list 0), crosswise far", "tu", one((A, B)), one((add(A, (4, 0)), B)), 1),
        ("uni-predicted P, bi-predicted Q, list 0 equal", "tu", U(ref=(0, -1), mv=(A, Z)), U(), 1),
        ("bi-predicted P, uni-predicted Q, list 1 equal", "tu", U(), U(ref=(-1, 1), mv=(Z, B)), 1),
        ("different pictures, equal vectors", "tu", U(ref=(0, -1), mv=(A, Z)), U(ref=(1, -1), mv=(A, Z)), 1),
        ("list 0 alone, same picture, 3 apart", "tu", U(ref=(0, -1), mv=(A, Z)), U(ref=(0, -1), mv=(add(A, (-3, 3)), Z)), 0),
        ("list 0 alone, same picture, 4 apart", "tu", U(ref=(0, -1), mv=(A, Z)), U(ref=(0, -1), mv=(add(A, (-4, 0)), Z)), 1),
        ("one picture, list 0 in P and list 1 in Q, 3 apart", "tu", U(ref=(0, -1), mv=(A, Z)), U(ref=(-1, 0), mv=(Z, add(A, (0, 3)))), 0),
        ("one picture, list 0 in P and list 1 in Q, 4 apart", "tu", U(ref=(0, -1), mv=(A, Z)), U(ref=(-1, 0), mv=(Z, add(A, (0, 4)))), 1),
        ("intra P", "tu", U(ref=(-1, -1), mv=(Z, Z), intra=1), U(), 2),
        ("intra Q", "tu", U(), U(ref=(-1, -1), mv=(Z, Z), intra=1), 2),
        ("coded residual in P, transform edge, equal motion", "tu", U(cbf=1), U(), 1),
        ("coded residual in Q, transform edge, equal motion", "tu", U(), U(cbf=1), 1),
        ("no residual, transform edge, equal motion", "tu", U(), U(), 0),
        ("coded residual, prediction edge alone, equal motion", "pu", U(cbf=1), U(cbf=1), 0),
        ("coded residual, prediction edge alone, 4 apart", "pu", U(cbf=1), U(cbf=1, mv=(A, add(B, (4, 0)))), 1),
        ("no residual, prediction edge alone, different pictures", "pu", U(), U(ref=(0, 2)), 1),
    ]
    return rows


def deblock_strength_case(depth):
    """every row of deblock_strength_rows once on a vertical and once on a horizontal edge: one 16x16 slot per (row, direction) in a 128-wide B picture, QP 40, no offsets.
    Flat 8x8 blocks whose level alternates by six (<< depth - 8): an edge of strength 1 or 2 changes the two samples next to it (beta 42, tc 6 or 7: d = 0, the strong
    filter moves a step of six), an edge of strength 0 nothing.  Returns deblock_case's dict plus `edges`: (what, direction, x, y of the slot, strength)."""
    rows = deblock_strength_rows()
    width = 128
    height = (2 * len(rows) + 7) // 8 * 16
    w4, h4 = width // 4, height // 4
    ru = np.zeros((h4, w4), REF_DB_UNIT_DT)
    du = np.zeros((h4, w4), DB_UNIT_DT)
    ru["qp"] = 40; du["qp"] = 40

    def put_cu(x, y, size, part, pus):
        ys, xs = slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4)
        ru["log2CU"][ys, xs] = int(np.log2(size)); ru["partSize"][ys, xs] = part; ru["intra"][ys, xs] = pus[0]["intra"]; ru["cbf"][ys, xs] = pus[0]["cbf"]
        du["flags"][ys, xs] |= pus[0]["intra"] * DB_INTRA + pus[0]["cbf"] * DB_CBF
        du["flags"][ys, x // 4] |= DB_TU_LEFT
        du["flags"][y // 4, xs] |= DB_TU_TOP
        q = size // 4
        for u, (px, py, pw, ph) in zip(pus, _PU_RECTS[part]):
            pys, pxs = slice((y + py * q) // 4, (y + (py + ph) * q) // 4), slice((x + px * q) // 4, (x + (px + pw) * q) // 4)
            for arr in (ru, du):
                arr["ref"][pys, pxs] = u["ref"]; arr["mv"][pys, pxs] = u["mv"]
            if px:
                du["flags"][pys, (x + px * q) // 4] |= DB_PU_LEFT
            if py:
                du["flags"][(y + py * q) // 4, pxs] |= DB_PU_TOP

    edges = []
    filler = dict(ref=(0, 1), mv=((8, -4), (-5, 9)), intra=0, cbf=0)
    for slot in range((width // 16) * (height // 16)):
        x, y = slot % (width // 16) * 16, slot // (width // 16) * 16
        if slot >= 2 * len(rows):
            for k in range(4):
                put_cu(x + (k & 1) * 8, y + (k >> 1) * 8, 8, 0, [filler])
            continue
        what, kind, P, Q, bs = rows[slot // 2]
        d = slot & 1
        if kind == "pu":
            put_cu(x, y, 16, 1 if d else 2, [P, Q])
        else:
            for k in range(4):
                put_cu(x + (k & 1) * 8, y + (k >> 1) * 8, 8, 0, [Q if (k >> 1 if d else k & 1) else P])
        edges.append((what, d, x, y, bs))
    yy, xx = np.mgrid[0:height // 8, 0:width // 8]
    step = 6 << (depth - 8)
    luma = np.kron((1 << (depth - 1)) + step * ((xx + yy) & 1), np.ones((8, 8), np.int64))
    yy, xx = np.mgrid[0:height // 16, 0:width // 16]
    chroma = np.kron((1 << (depth - 1)) + step * ((xx + yy) & 1), np.ones((8, 8), np.int64))
    planes, stride, cstride, org = edge_frame(depth, width, height, [luma, chroma, chroma.copy()])
    return dict(planes=planes, stride=stride, cstride=cstride, org=org, width=width, height=height, ref_units=np.ascontiguousarray(ru.ravel()),
                units=np.ascontiguousarray(du.ravel()), beta=0, tc=0, cb=0, cr=0, bypass=0, slice_p=0, edges=edges, depth=depth)


def deblock_strength_changed(c, before, after):
    """per entry of c['edges']: did the two luma samples next to the slot's inner edge change, on the lines that edges of the other direction never touch (3 and 4 of an
    8x8 block)"""
    a, b = edge_picture(before, c["width"], c["height"], 0), edge_picture(after, c["width"], c["height"], 0)
    out = []
    for (what, d, x, y, bs) in c["edges"]:
        lines = [y + 3, y + 4, y + 11, y + 12] if d == 0 else [x + 3, x + 4, x + 11, x + 12]
        if d == 0:
            ch = [bool((a[l, x + 7:x + 9] != b[l, x + 7:x + 9]).all()) for l in lines]
        else:
            ch = [bool((a[y + 7:y + 9, l] != b[y + 7:y + 9, l]).all()) for l in lines]
        same = [bool((a[l, x + 5:x + 11] == b[l, x + 5:x + 11]).all()) if d == 0 else bool((a[y + 5:y + 11, l] == b[y + 5:y + 11, l]).all()) for l in lines]
        assert all(ch) or all(same), (what, d, ch, same)
        out.append(all(ch))
    return out


def _dev_planes(planes, org, shift=0):
    """the padded planes on the device, `shift` samples into buffers one sample longer (poison in front); the table of the picture origins' addresses"""
    import torch
    isz = planes[0].itemsize
    bufs = []
    for p in planes:
        flat = np.concatenate([p.ravel()[:1]] * shift + [p.ravel()])
        bufs.append(torch.from_numpy(flat.view(np.uint8).copy()).cuda())
    tab = np.array([b.data_ptr() + (o + shift) * isz for b, o in zip(bufs, (org[0], org[1], org[1]))], np.uint64)
    return bufs, tab


def _host_planes(bufs, planes, shift=0):
    return [b.cpu().numpy().view(p.dtype)[shift:].reshape(p.shape) for b, p in zip(bufs, planes)]


def deblock_run_hip_forms(L, c, passes=3):
    """the picture through x265amd_deblock_picture, through x265amd_deblock_rows CTU row by CTU row, and through x265amd_deblock_rows_cols CTU row by CTU row and column
    by column in order: dict(picture, rows, cols) of padded planes.  passes 1 or 2: that pass alone in every form."""
    import torch
    w, h = c["width"], c["height"]
    d_units = torch.from_numpy(c["units"].view(np.uint8).copy()).cuda()
    tail = (C.c_void_p(d_units.data_ptr()), c["beta"], c["tc"], c["cb"], c["cr"], c["bypass"], passes)
    out = {}
    for form in ("picture", "rows", "cols"):
        bufs, tab = _dev_planes(c["planes"], c["org"])
        head = (None, C.c_void_p(int(tab[0])), C.c_void_p(int(tab[1])), C.c_void_p(int(tab[2])), C.c_int64(c["stride"]), C.c_int64(c["cstride"]), w, h)
        if form == "picture":
            assert L.lib.x265amd_deblock_picture(*head, *tail) == 0
        else:
            for y4 in range(0, h // 4, 16):
                y4e = min(h // 4, y4 + 16)
                if form == "rows":
                    assert L.lib.x265amd_deblock_rows(*head, *tail, y4, y4e) == 0
                else:
                    for col in range((w + 63) // 64):
                        assert L.lib.x265amd_deblock_rows_cols(*head, *tail, y4, y4e, col, col + 1) == 0
        torch.cuda.synchronize()
        out[form] = _host_planes(bufs, c["planes"])
    return out


def sao_edge_case(depth, seed, width, height, content="noise", source="near", force_band=None, index=0):
    """sao_case's record under planes with the encoder's margins, poisoned (source picture included).  content: edge_content's mode of the deblocked picture; source:
    'near' -- the picture plus noise of +-6, 'opposite' -- the other end of the range (pmax - sample: the largest differences the sums can hold).  Parameters: offsets from
    the whole range (+-7 at 8 bits, +-31 at 10) with both ends put into every CTU's luma record, the types of CTU j cycling through -1 .. 4 from `index` on, luma and chroma
    at different rates; force_band: the band positions of CTU j's three planes become force_band[(j + plane) % len]"""
    rng = np.random.default_rng(seed)
    pmax = (1 << depth) - 1
    rec = edge_content(depth, rng, width, height, content)
    if source == "near":
        fenc = [np.clip(r + rng.integers(-6, 7, r.shape), 0, pmax) for r in rec]
    else:
        fenc = [pmax - r for r in rec]
    planes, stride, cstride, org = edge_frame(depth, width, height, rec)
    fplanes = edge_frame(depth, width, height, fenc)[0]
    nctu = ((width + 63) // 64) * ((height + 63) // 64)
    top = 7 if depth == 8 else 31
    params = np.zeros(nctu, SAO_CTU_DT)
    params["bandPos"] = rng.integers(0, 32, (nctu, 3))
    params["offset"] = rng.integers(-top, top + 1, (nctu, 3, 4))
    for j in range(nctu):
        n = 4 * index + j
        params["type"][j] = (n % 6 - 1, (n + n // 6 + 2) % 6 - 1)
        for plane in range(3):
            params["offset"][j, plane, (j + plane) % 4] = top if (j + plane) & 1 else -top
            if force_band:
                params["bandPos"][j, plane] = force_band[(j + plane) % len(force_band)]
    return dict(rec=planes, fenc=fplanes, stride=stride, cstride=cstride, org=org, width=width, height=height, params=params, nctu=nctu, depth=depth, content=content)


def sao_apply_coverage(c):
    """from the deblocked picture and the parameters: dict(clip_lo, clip_hi: samples whose offset sum leaves the range, wrapped: samples of a band pos + k > 31 with a
    non-zero offset) -- the edge offsets' sums computed with the table of H.265 8.7.3"""
    w, h = c["width"], c["height"]
    pmax = (1 << c["depth"]) - 1
    ctuW = (w + 63) // 64
    n = dict(clip_lo=0, clip_hi=0, wrapped=0)
    for k in range(3):
        sh = 1 if k else 0
        v = edge_picture(c["rec"], w, h, k).astype(np.int64)
        ph, pw = v.shape
        yy, xx = np.mgrid[0:ph, 0:pw]
        ctu = ((yy << sh) >> 6) * ctuW + ((xx << sh) >> 6)
        typ = c["params"]["type"][:, 1 if k else 0].astype(np.int64)[ctu]
        offs = c["params"]["offset"][:, k, :].astype(np.int64)[ctu]                      # [y][x][4]
        pos = c["params"]["bandPos"][:, k].astype(np.int64)[ctu]
        out = v.copy()
        band = ((v >> (c["depth"] - 5)) - pos) & 31
        isb = (typ == 4) & (band < 4)
        boff = np.take_along_axis(offs, np.minimum(band, 3)[..., None], 2)[..., 0]
        out[isb] += boff[isb]
        n["wrapped"] += int((isb & (pos + band > 31) & (boff != 0)).sum())
        e = np.pad(v, 1, mode="edge")
        for t, (dx, dy) in enumerate(((-1, 0), (0, -1), (-1, -1), (1, -1))):
            a, b = e[1 + dy:1 + dy + ph, 1 + dx:1 + dx + pw], e[1 - dy:1 - dy + ph, 1 - dx:1 - dx + pw]
            cls = np.array([1, 2, 0, 3, 4])[np.sign(v - a) + np.sign(v - b) + 2]
            inside = np.ones_like(v, bool)
            if dx:
                inside[:, 0] = inside[:, -1] = False
            if dy:
                inside[0, :] = inside[-1, :] = False
            m = (typ == t) & inside & (cls > 0)
            eoff = np.take_along_axis(offs, np.maximum(cls - 1, 0)[..., None], 2)[..., 0]
            out[m] += eoff[m]
        n["clip_lo"] += int((out < 0).sum()); n["clip_hi"] += int((out > pmax).sum())
    return n


def sao_run_hip_forms(L, c):
    """dict: picture -- (count, offsetOrg, offset planes) through x265amd_sao_stats / x265amd_sao_apply; cols -- the same through x265amd_sao_stats_rows_cols CTU by CTU
    and x265amd_sao_apply_rows_cols CTU row by CTU row and 64-sample column range by range, in order; odd -- (count, offsetOrg) through x265amd_sao_stats with every
    plane's origin one sample further into its buffer"""
    import torch
    w, h = c["width"], c["height"]
    ctuW, ctuH = (w + 63) // 64, (h + 63) // 64
    n = c["nctu"] * 3 * 5 * 32
    geom = (C.c_int64(c["stride"]), C.c_int64(c["cstride"]), w, h)
    d_par = torch.from_numpy(c["params"].view(np.uint8).copy()).cuda()
    out = {}
    for form in ("picture", "cols", "odd"):
        shift = 1 if form == "odd" else 0
        rec, rtab = _dev_planes(c["rec"], c["org"], shift)
        fenc, ftab = _dev_planes(c["fenc"], c["org"], shift)
        dst, dtab = _dev_planes(c["rec"], c["org"], shift)
        d_cnt = torch.full((n,), -1515870811, dtype=torch.int32, device="cuda"); d_org = torch.full((n,), -1515870811, dtype=torch.int32, device="cuda")
        stats = (None, _ptr(rtab), _ptr(ftab), *geom, C.c_void_p(d_cnt.data_ptr()), C.c_void_p(d_org.data_ptr()))
        apply = (None, _ptr(rtab), _ptr(dtab), *geom, C.c_void_p(d_par.data_ptr()))
        if form == "cols":
            for r in range(ctuH):
                for col in range(ctuW):
                    assert L.lib.x265amd_sao_stats_rows_cols(*stats, r, r + 1, col, col + 1) == 0
                for col in range(ctuW):
                    assert L.lib.x265amd_sao_apply_rows_cols(*apply, r, r + 1, 64 * col, min(w, 64 * col + 64)) == 0
        else:
            assert L.lib.x265amd_sao_stats(*stats) == 0
            if form == "picture":
                assert L.lib.x265amd_sao_apply(*apply) == 0
        torch.cuda.synchronize()
        out[form] = (d_cnt.cpu().numpy(), d_org.cpu().numpy(), _host_planes(dst, c["rec"], shift), _host_planes(rec, c["rec"], shift))
    return out


# ----------------------------------------------------------------------------------------------------------
# layer 2 as documented (include/x265amd.h): batched job lists through x265amd_run_jobs -- tests/test_job_lists.py.
# The per-slot shims (csrc/slot_shims.hip) repack every operand and launch one job; here the operands of a whole batch
# lie in two arenas that exist twice, byte for byte: on the host, where the oracle runs on them, and on the device,
# where the kernels do.  Job addresses are the device base plus the host offset and strides are the host's, so the whole
# output arena can be compared at the end: every block right, nothing written outside one, nothing left unwritten.
# ----------------------------------------------------------------------------------------------------------
JOB_DT = np.dtype([("op", "<i4"), ("size", "<i4"), ("p", "<i4", (6,)), ("a", "<u8"), ("b", "<u8"), ("c", "<u8"), ("d", "<u8"), ("e", "<u8", (2,)),
                   ("sa", "<i4"), ("sb", "<i4"), ("sc", "<i4"), ("sd", "<i4")])      # x265amd_job
# enum x265amd_op; family = op // 32 (tests/test_job_lists.py checks the values against the header's text)
JOB_OPS = dict(SAD=0, SAD_X3=1, SAD_X4=2, SATD=3, SA8D=4, SSE_PP=5, SSE_SS=6, SSD_S=7, PSY_COST_PP=8, VAR=9, CHROMA_SATD=10, CHROMA_SA8D=11,
               SUB_PS=32, ADD_PS=33, PIXELAVG_PP=34, ADDAVG=35, WEIGHT_PP=36, WEIGHT_SP=37, SCALE2D_64TO32=38, SCALE1D_128TO64=39, TRANSPOSE=40,
               CPY2DTO1D_SHL=41, CPY2DTO1D_SHR=42, CPY1DTO2D_SHL=43, CPY1DTO2D_SHR=44, COPY_CNT=45, COUNT_NONZERO=46,
               DCT=64, IDCT=65, DST4=66, IDST4=67, QUANT=68, NQUANT=69, DEQUANT_NORMAL=70, DEQUANT_SCALING=71,
               INTRA_PRED=96, INTRA_FILTER=97, INTRA_ALLANGS=98,
               IP_HPP=128, IP_HPS=129, IP_VPP=130, IP_VPS=131, IP_VSP=132, IP_VSS=133, IP_HVPP=134, IP_P2S=135)
JOB_OP_NAME = {v: k for k, v in JOB_OPS.items()}
JOB_FAMILIES = 5
# how many distinct (size index, filter phase ...) keys every op has to appear with over a family's batches:
#   PU ops 25 partitions, CU ops 5 sizes (TU ops 4); chroma_satd the 18 partitions whose 4:2:0 half is a multiple of 4x4, chroma_sa8d cu 1..4;
#   addAvg luma + 4:2:0; weight_pp widths 16..64 in steps of 16, weight_sp those less one; quantisation 16 / 64 / 256 / 1024 coefficients;
#   intra_pred 4 sizes x 35 modes x bFilter, allangs 4 sizes x bLuma;
#   interpolation: luma 25 partitions x coeffIdx 0..3, 4:2:0 chroma 24 partitions (none for part 0) x coeffIdx 0..7; hps twice that (isRowExt); hvpp 25 x the nine
#   (idxX, idxY) in 1..3 x 1..3; p2s 25 + 24
JOB_COVERAGE = dict(SAD=25, SAD_X3=25, SAD_X4=25, SATD=25, SA8D=5, SSE_PP=5, SSE_SS=5, SSD_S=5, PSY_COST_PP=5, VAR=5, CHROMA_SATD=18, CHROMA_SA8D=4,
                    SUB_PS=5, ADD_PS=5, PIXELAVG_PP=25, ADDAVG=50, WEIGHT_PP=4, WEIGHT_SP=4, SCALE2D_64TO32=1, SCALE1D_128TO64=1, TRANSPOSE=5,
                    CPY2DTO1D_SHL=4, CPY2DTO1D_SHR=4, CPY1DTO2D_SHL=4, CPY1DTO2D_SHR=4, COPY_CNT=4, COUNT_NONZERO=4,
                    DCT=4, IDCT=4, DST4=1, IDST4=1, QUANT=4, NQUANT=4, DEQUANT_NORMAL=4, DEQUANT_SCALING=4,
                    INTRA_PRED=280, INTRA_FILTER=4, INTRA_ALLANGS=8,
                    IP_HPP=25 * 4 + 24 * 8, IP_HPS=2 * (25 * 4 + 24 * 8), IP_VPP=25 * 4 + 24 * 8, IP_VPS=25 * 4 + 24 * 8, IP_VSP=25 * 4 + 24 * 8,
                    IP_VSS=25 * 4 + 24 * 8, IP_HVPP=25 * 9, IP_P2S=25 + 24)
JOB_PLANE = 8192            # elements per shared source plane: the largest reach is an 8-tap 64x64 block at stride 83, (63 + 7) * 83 + 64 + 7 elements
JOB_GUARD = 8               # poison bytes kept between two jobs' output regions, at least


class _JobHost:
    """pointers into the host copies of the two arenas, for the oracle side of a job"""

    def __init__(self, inb, outb):
        self.inb, self.outb = inb, outb

    def i(self, o):
        return C.c_void_p(self.inb.ctypes.data + o)

    def o(self, o):
        return C.c_void_p(self.outb.ctypes.data + o)

    def u64(self, o, v):
        """a scalar result as the kernels store it: the int (sign-extended) or uint64 return value in a 64-bit word"""
        self.outb[o:o + 8] = np.array([int(v) & 0xFFFFFFFFFFFFFFFF], np.uint64).view(np.uint8)


class JobSpec:
    """one job before the device addresses are known: ins / outs map the record's address fields (a b c d e0 e1) to byte offsets in the input / output arena"""
    __slots__ = ("op", "size", "p", "ins", "outs", "sa", "sb", "sc", "sd", "key", "oracle")

    def name(self):
        return "%s size %d key %s" % (JOB_OP_NAME[self.op], self.size, self.key)


class JobArena:
    """The memory of one family's jobs for one (depth, mode).  Input: a few shared source planes (pix_buf / s16_buf contents and ranges of the case_* functions above) that
    the jobs read at their own offsets, as the calls of a host loop read one picture.  Output: a disjoint region per job, handed out by a cursor while the jobs are built.
    The j_* methods are the builders, one per op; each follows the op's shim in csrc/slot_shims.hip field for field and returns the JobSpec whose `oracle` is the orc_* call
    with the same size index, pointers and strides on the host copies."""

    def __init__(self, L, rng, mode):
        self.L, self.rng, self.mode, self.px = L, rng, mode, np.dtype(L.pixel).itemsize
        opp = "random" if mode == "random" else ("max" if mode == "min" else "min")
        lim, n = L.pmax, JOB_PLANE
        self.rem = int(rng.integers(0, 6))          # qp % 6 of the quantisation tables in this arena
        smooth = np.clip(np.cumsum(rng.integers(-3, 4, n)) + L.pmax // 2, 0, L.pmax).astype(L.pixel) if mode == "random" else pix_buf(L, rng, n, mode)
        qc = np.full(n, QUANT_SCALES[self.rem], np.int32)
        dqc = np.full(n, INV_QUANT_SCALES[self.rem] * 16, np.int32)
        if mode == "random":                        # scaling-list style tables, as in case_quant
            qc = (qc.astype(np.int64) * 16 // rng.integers(8, 40, n)).astype(np.int32)
            dqc = (INV_QUANT_SCALES[self.rem] * rng.integers(8, 40, n)).astype(np.int32)
        planes = [("pix", pix_buf(L, rng, n, mode)), ("pix2", pix_buf(L, rng, n, opp)), ("smooth", smooth),
                  ("res", s16_buf(rng, n, -lim, lim, mode)), ("res2", s16_buf(rng, n, -lim, lim, opp)),
                  ("ifs", s16_buf(rng, n, -8192, 8191, mode)), ("coef", s16_buf(rng, n, -32768, 32767, mode)),
                  ("cpy", s16_buf(rng, n, -4096, 4095, mode)), ("lvl", s16_buf(rng, n, -3, 3, mode)), ("qc", qc), ("dqc", dqc)]
        self.planes, parts, at = {}, [], 0
        for kind, arr in planes:
            self.planes[kind] = (at, arr.itemsize)
            raw = arr.view(np.uint8)
            parts.append(raw)
            pad = -raw.size % 64
            parts.append(np.zeros(pad, np.uint8))
            at += raw.size + pad
        self.inb = np.concatenate(parts)
        self.cur = 0
        self.specs = []

    # ---- placement ----
    def stride(self, w):
        """the block width itself, the width plus a small even padding, or an odd stride"""
        return int(self.rng.choice([w, w + 2, w + 6, w + 16, 67, 83]))

    def pick(self, kind, before, after):
        """byte offset of an operand in the shared plane `kind`: an odd element offset that leaves `before` elements in front of it and `after` from it on"""
        at, elem = self.planes[kind]
        lo, hi = before, JOB_PLANE - after
        assert 0 <= lo < hi - 1, (kind, before, after)
        o = int(self.rng.integers(lo, hi)) | 1
        if o > hi:
            o -= 2
        assert lo <= o <= hi and o & 1
        return at + o * elem

    def _out(self, nbytes, skew):
        start = (self.cur + JOB_GUARD + 7) // 8 * 8 + skew
        self.cur = start + nbytes
        return start

    def out_rect(self, elem, w, h, stride):
        """an output block: element-aligned, at an odd element offset from an 8-byte boundary"""
        return self._out(((h - 1) * stride + w) * elem, elem * int(self.rng.choice([1, 3])))

    def out_flat(self, elem, n):
        return self.out_rect(elem, n, 1, n)

    def out_u64(self):
        return self._out(8, 0)                      # 64-bit scalar results: 8-byte aligned

    def out_i32(self, n):
        return self._out(4 * n, 4)                  # sad_x3 / sad_x4 results: 4-byte aligned and no more

    @property
    def out_size(self):
        return (self.cur + JOB_GUARD + 63) // 64 * 64

    def poison(self):
        return ((np.arange(self.out_size, dtype=np.uint32) * 37 + 11) & 0xFF).astype(np.uint8)

    def job(self, op, size, key, oracle, p=(), ins=None, outs=None, sa=0, sb=0, sc=0, sd=0):
        s = JobSpec()
        s.op, s.size, s.key, s.oracle = JOB_OPS[op], size, key, oracle
        s.p = tuple(p) + (0,) * (6 - len(p))
        s.ins, s.outs, s.sa, s.sb, s.sc, s.sd = ins or {}, outs or {}, sa, sb, sc, sd
        self.specs.append(s)
        return s

    # ---- family 0: distortion (dist_pp, sad_xn and the 16-bit forms of the shims) ----
    def _dist(self, op, name, size, w, h, kinds=("pix", "pix2"), csp=False):
        sa, sb = self.stride(w), self.stride(w)
        a, b, d = self.pick(kinds[0], 0, (h - 1) * sa + w), self.pick(kinds[1], 0, (h - 1) * sb + w), self.out_u64()
        args = (CSP_I420, size) if csp else (size,)
        return self.job(op, size, (size,), lambda O, M: M.u64(d, O.call(name, *args, M.i(a), sa, M.i(b), sb)), ins=dict(a=a, b=b), outs=dict(d=d), sa=sa, sb=sb)

    def _dist1(self, op, name, size, kind):
        n = 4 << size
        sa = self.stride(n)
        a, d = self.pick(kind, 0, (n - 1) * sa + n), self.out_u64()
        return self.job(op, size, (size,), lambda O, M: M.u64(d, O.call(name, size, M.i(a), sa)), ins=dict(a=a), outs=dict(d=d), sa=sa)

    def _sad_xn(self, op, name, part, nc):
        w, h = PU_SIZES[part]
        sb = self.stride(w)
        a = self.pick("pix", 0, (h - 1) * FENC_STRIDE + w)          # fenc: the reference's 64-element stride, no stride field
        r = [self.pick("pix2", 0, (h - 1) * sb + w) for _ in range(nc)]
        d = self.out_i32(nc)
        ins = dict(zip(("b", "c", "e0", "e1"), r), a=a)
        return self.job(op, part, (part,), lambda O, M: O.call(name, part, M.i(a), *[M.i(x) for x in r], sb, M.o(d)), ins=ins, outs=dict(d=d), sb=sb)

    def j_sad(self, part): return self._dist("SAD", "sad", part, *PU_SIZES[part])
    def j_sad_x3(self, part): return self._sad_xn("SAD_X3", "sad_x3", part, 3)
    def j_sad_x4(self, part): return self._sad_xn("SAD_X4", "sad_x4", part, 4)
    def j_satd(self, part): return self._dist("SATD", "satd", part, *PU_SIZES[part])
    def j_sa8d(self, cu): return self._dist("SA8D", "sa8d", cu, 4 << cu, 4 << cu)
    def j_sse_pp(self, cu): return self._dist("SSE_PP", "sse_pp", cu, 4 << cu, 4 << cu)
    def j_sse_ss(self, cu): return self._dist("SSE_SS", "sse_ss", cu, 4 << cu, 4 << cu, kinds=("res", "res2"))
    def j_ssd_s(self, cu): return self._dist1("SSD_S", "ssd_s", cu, "res")
    def j_psy_cost_pp(self, cu): return self._dist("PSY_COST_PP", "psy_cost_pp", cu, 4 << cu, 4 << cu)
    def j_var(self, cu): return self._dist1("VAR", "var", cu, "pix")
    def j_chroma_satd(self, part): return self._dist("CHROMA_SATD", "chroma_satd", part, PU_SIZES[part][0] // 2, PU_SIZES[part][1] // 2, csp=True)
    def j_chroma_sa8d(self, cu): return self._dist("CHROMA_SA8D", "chroma_sa8d", cu, 2 << cu, 2 << cu, csp=True)

    # ---- family 1: pixel / residual block ops ----
    def _rect3(self, op, size, key, w, h, ka, ea, kb, eb, ed, call, p=()):
        """two strided inputs, one strided output"""
        sa, sb, sd = self.stride(w), self.stride(w), self.stride(w)
        a, b, d = self.pick(ka, 0, (h - 1) * sa + w), self.pick(kb, 0, (h - 1) * sb + w), self.out_rect(ed, w, h, sd)
        return self.job(op, size, key, lambda O, M: call(O, M.i(a), sa, M.i(b), sb, M.o(d), sd), p=p, ins=dict(a=a, b=b), outs=dict(d=d), sa=sa, sb=sb, sd=sd)

    def j_sub_ps(self, cu):
        n = 4 << cu
        return self._rect3("SUB_PS", cu, (cu,), n, n, "pix", self.px, "pix2", self.px, 2, lambda O, a, sa, b, sb, d, sd: O.call("sub_ps", cu, d, sd, a, b, sa, sb))

    def j_add_ps(self, cu):
        n = 4 << cu
        return self._rect3("ADD_PS", cu, (cu,), n, n, "pix", self.px, "res", 2, self.px, lambda O, a, sa, b, sb, d, sd: O.call("add_ps", cu, d, sd, a, b, sa, sb))

    def j_pixelavg_pp(self, part):
        w, h = PU_SIZES[part]
        return self._rect3("PIXELAVG_PP", part, (part,), w, h, "pix", self.px, "pix", self.px, self.px, lambda O, a, sa, b, sb, d, sd: O.call("pixelavg_pp", part, d, sd, a, sa, b, sb))

    def j_addavg(self, part, chroma):
        w, h = PU_SIZES[part][0] >> chroma, PU_SIZES[part][1] >> chroma
        if chroma:
            call = lambda O, a, sa, b, sb, d, sd: O.call("chroma_addAvg", CSP_I420, part, a, b, d, sa, sb, sd)
        else:
            call = lambda O, a, sa, b, sb, d, sd: O.call("addAvg", part, a, b, d, sa, sb, sd)
        return self._rect3("ADDAVG", part, (part, chroma), w, h, "ifs", 2, "ifs", 2, self.px, call, p=(chroma,))

    def _weight_args(self):
        rng, corr = self.rng, 14 - self.L.depth
        shift = int(rng.integers(0, 7)) + corr
        rnd = ((1 << (shift - 1)) if shift else 0) & ~((1 << corr) - 1)
        return int(rng.integers(1, 17)), int(rng.integers(1, 128)), rnd, shift, int(rng.integers(-20, 21))

    def j_weight_pp(self, w):
        """w: a multiple of 16.  weightp_pp_t has ONE stride for source and destination: sa == sd"""
        h, w0, rnd, shift, offset = self._weight_args()
        st = self.stride(w)
        a, d = self.pick("pix", 0, (h - 1) * st + w), self.out_rect(self.px, w, h, st)
        return self.job("WEIGHT_PP", 0, (w,), lambda O, M: O.call("weight_pp", M.i(a), M.o(d), st, w, h, w0, rnd, shift, offset), p=(w, h, w0, rnd, shift, offset),
                        ins=dict(a=a), outs=dict(d=d), sa=st, sd=st)

    def j_weight_sp(self, w):
        h, w0, rnd, shift, offset = self._weight_args()
        sa, sd = self.stride(w), self.stride(w)
        a, d = self.pick("ifs", 0, (h - 1) * sa + w), self.out_rect(self.px, w, h, sd)
        return self.job("WEIGHT_SP", 0, (w,), lambda O, M: O.call("weight_sp", M.i(a), M.o(d), sa, sd, w, h, w0, rnd, shift, offset), p=(w, h, w0, rnd, shift, offset),
                        ins=dict(a=a), outs=dict(d=d), sa=sa, sd=sd)

    def j_scale2d_64to32(self):
        sa = self.stride(64)
        a, d = self.pick("pix", 0, 63 * sa + 64), self.out_flat(self.px, 32 * 32)
        return self.job("SCALE2D_64TO32", 0, (0,), lambda O, M: O.call("scale2D_64to32", M.o(d), M.i(a), sa), ins=dict(a=a), outs=dict(d=d), sa=sa)

    def j_scale1d_128to64(self):
        a, d = self.pick("pix", 0, 256), self.out_flat(self.px, 128)
        return self.job("SCALE1D_128TO64", 0, (0,), lambda O, M: O.call("scale1D_128to64", M.o(d), M.i(a)), ins=dict(a=a), outs=dict(d=d))

    def j_transpose(self, cu):
        n = 4 << cu
        sa = self.stride(n)
        a, d = self.pick("pix", 0, (n - 1) * sa + n), self.out_flat(self.px, n * n)
        return self.job("TRANSPOSE", cu, (cu,), lambda O, M: O.call("transpose", cu, M.o(d), M.i(a), sa), ins=dict(a=a), outs=dict(d=d), sa=sa)

    def _cpy(self, op, name, cu, to1d):
        n, shift = 4 << cu, int(self.rng.integers(1, 3))
        st = self.stride(n)
        if to1d:
            a, d = self.pick("cpy", 0, (n - 1) * st + n), self.out_flat(2, n * n)
            return self.job(op, cu, (cu,), lambda O, M: O.call(name, cu, M.o(d), M.i(a), st, shift), p=(shift,), ins=dict(a=a), outs=dict(d=d), sa=st)
        a, d = self.pick("cpy", 0, n * n), self.out_rect(2, n, n, st)           # the coefficient input is packed
        return self.job(op, cu, (cu,), lambda O, M: O.call(name, cu, M.o(d), M.i(a), st, shift), p=(shift,), ins=dict(a=a), outs=dict(d=d), sd=st)

    def j_cpy2dto1d_shl(self, cu): return self._cpy("CPY2DTO1D_SHL", "cpy2Dto1D_shl", cu, True)
    def j_cpy2dto1d_shr(self, cu): return self._cpy("CPY2DTO1D_SHR", "cpy2Dto1D_shr", cu, True)
    def j_cpy1dto2d_shl(self, cu): return self._cpy("CPY1DTO2D_SHL", "cpy1Dto2D_shl", cu, False)
    def j_cpy1dto2d_shr(self, cu): return self._cpy("CPY1DTO2D_SHR", "cpy1Dto2D_shr", cu, False)

    def j_copy_cnt(self, cu):
        n = 4 << cu
        sa = self.stride(n)
        a, d, e0 = self.pick("lvl" if self.rng.integers(0, 2) else "cpy", 0, (n - 1) * sa + n), self.out_flat(2, n * n), self.out_u64()
        return self.job("COPY_CNT", cu, (cu,), lambda O, M: M.u64(e0, O.call("copy_cnt", cu, M.o(d), M.i(a), sa)), ins=dict(a=a), outs=dict(d=d, e0=e0), sa=sa)

    def j_count_nonzero(self, cu):
        n = 4 << cu
        a, d = self.pick("lvl", 0, n * n), self.out_u64()                       # packed
        return self.job("COUNT_NONZERO", cu, (cu,), lambda O, M: M.u64(d, O.call("count_nonzero", cu, M.i(a))), ins=dict(a=a), outs=dict(d=d))

    # ---- family 2: transforms + quantisation ----
    def _fwd(self, op, name, cu, dst4):
        n = 4 << cu
        sa = self.stride(n)
        a, d = self.pick("res", 0, (n - 1) * sa + n), self.out_flat(2, n * n)
        call = (lambda O, M: O.call(name, M.i(a), M.o(d), sa)) if dst4 else (lambda O, M: O.call(name, cu, M.i(a), M.o(d), sa))
        return self.job(op, cu, (cu,), call, ins=dict(a=a), outs=dict(d=d), sa=sa)

    def _inv(self, op, name, cu, dst4):
        """coefficients packed; plausible (residual-range) or full-range values, as case_dct feeds both"""
        n = 4 << cu
        sd = self.stride(n)
        a, d = self.pick("coef" if self.rng.integers(0, 2) else "res", 0, n * n), self.out_rect(2, n, n, sd)
        call = (lambda O, M: O.call(name, M.i(a), M.o(d), sd)) if dst4 else (lambda O, M: O.call(name, cu, M.i(a), M.o(d), sd))
        return self.job(op, cu, (cu,), call, ins=dict(a=a), outs=dict(d=d), sd=sd)

    def j_dct(self, cu): return self._fwd("DCT", "dct", cu, False)
    def j_idct(self, cu): return self._inv("IDCT", "idct", cu, False)
    def j_dst4(self): return self._fwd("DST4", "dst4x4", 0, True)
    def j_idst4(self): return self._inv("IDST4", "idst4x4", 0, True)

    def _qparams(self, cu):
        """qBits / add / per / dequantisation shift of case_quant for a TU of size index cu, at a QP whose remainder is the arena's"""
        per = int(self.rng.integers(0, 9 if self.rem < 4 else 8))
        tshift = 15 - self.L.depth - (cu + 2)
        qbits = 14 + per + tshift
        return qbits, (171 if self.rng.integers(0, 2) else 85) << (qbits - 9), per, 20 - 14 - tshift

    def j_quant(self, cu):
        num = (4 << cu) ** 2
        qbits, add, _, _ = self._qparams(cu)
        a, b = self.pick("coef", 0, num), self.pick("qc", 0, num)
        d, e0, e1 = self.out_flat(2, num), self.out_flat(4, num), self.out_u64()
        return self.job("QUANT", 0, (num,), lambda O, M: M.u64(e1, O.call("quant", M.i(a), M.i(b), M.o(e0), M.o(d), qbits, add, num)), p=(qbits, add, num),
                        ins=dict(a=a, b=b), outs=dict(d=d, e0=e0, e1=e1))

    def j_nquant(self, cu):
        num = (4 << cu) ** 2
        qbits, add, _, _ = self._qparams(cu)
        a, b, d, e1 = self.pick("coef", 0, num), self.pick("qc", 0, num), self.out_flat(2, num), self.out_u64()
        return self.job("NQUANT", 0, (num,), lambda O, M: M.u64(e1, O.call("nquant", M.i(a), M.i(b), M.o(d), qbits, add, num)), p=(qbits, add, num),
                        ins=dict(a=a, b=b), outs=dict(d=d, e1=e1))

    def j_dequant_normal(self, cu):
        num = (4 << cu) ** 2
        _, _, per, shift = self._qparams(cu)
        scale = INV_QUANT_SCALES[self.rem] << per
        a, d = self.pick("coef", 0, num), self.out_flat(2, num)
        return self.job("DEQUANT_NORMAL", 0, (num,), lambda O, M: O.call("dequant_normal", M.i(a), M.o(d), num, scale, shift), p=(num, scale, shift), ins=dict(a=a), outs=dict(d=d))

    def j_dequant_scaling(self, cu):
        num = (4 << cu) ** 2
        _, _, per, shift = self._qparams(cu)
        a, b, d = self.pick("coef", 0, num), self.pick("dqc", 0, num), self.out_flat(2, num)
        return self.job("DEQUANT_SCALING", 0, (num,), lambda O, M: O.call("dequant_scaling", M.i(a), M.i(b), M.o(d), num, per, shift), p=(num, per, shift),
                        ins=dict(a=a, b=b), outs=dict(d=d))

    # ---- family 3: intra prediction (neighbour arrays packed: 4N + 1 samples) ----
    def j_intra_pred(self, cu, mode, bfilter):
        n = 4 << cu
        sd = self.stride(n)
        a, d = self.pick("smooth" if self.rng.integers(0, 2) else "pix", 0, 4 * n + 1), self.out_rect(self.px, n, n, sd)
        return self.job("INTRA_PRED", cu, (cu, mode, bfilter), lambda O, M: O.call("intra_pred", cu, mode, M.o(d), sd, M.i(a), bfilter), p=(mode, bfilter),
                        ins=dict(a=a), outs=dict(d=d), sd=sd)

    def j_intra_filter(self, cu):
        n = 4 << cu
        a, d = self.pick("smooth" if self.rng.integers(0, 2) else "pix", 0, 4 * n + 1), self.out_flat(self.px, 4 * n + 1)
        return self.job("INTRA_FILTER", cu, (cu,), lambda O, M: O.call("intra_filter", cu, M.i(a), M.o(d)), ins=dict(a=a), outs=dict(d=d))

    def j_intra_allangs(self, cu, bluma):
        n = 4 << cu
        a, b, d = self.pick("pix", 0, 4 * n + 1), self.pick("smooth", 0, 4 * n + 1), self.out_flat(self.px, 33 * n * n)
        return self.job("INTRA_ALLANGS", cu, (cu, bluma), lambda O, M: O.call("intra_allangs", cu, M.o(d), M.i(a), M.i(b), bluma), p=(bluma,), ins=dict(a=a, b=b), outs=dict(d=d))

    # ---- family 4: interpolation.  The margins are those of the shim's interp(): taps / 2 - 1 samples left and above, taps - 1 - (taps / 2 - 1) right and below ----
    def _ip(self, op, name, part, chroma, idx, aux, horiz, vert, src16, dst16, ext_rows=0, extra=None):
        taps = 4 if chroma else 8
        w, h = PU_SIZES[part][0] >> chroma, PU_SIZES[part][1] >> chroma
        half = taps // 2 - 1
        mx, mxr = (half, taps - 1 - half) if horiz else (0, 0)
        mt, mb = (half, taps - 1 - half) if vert else (0, 0)
        sa, sd = self.stride(w), self.stride(w)
        a = self.pick("ifs" if src16 else "pix", mt * sa + mx, (h - 1 + mb) * sa + w + mxr)
        d = self.out_rect(2 if dst16 else self.px, w, h + ext_rows, sd)
        args = ((CSP_I420, part) if chroma else (part,))
        tail = () if extra is None else extra
        return self.job(op, 0, (part, chroma) + tuple(tail), lambda O, M: O.call(("chroma_" if chroma else "luma_") + name, *args, M.i(a), sa, M.o(d), sd, *tail),
                        p=(taps, w, h, idx, aux), ins=dict(a=a), outs=dict(d=d), sa=sa, sd=sd)

    def j_ip_hpp(self, part, chroma, idx): return self._ip("IP_HPP", "hpp", part, chroma, idx, 0, True, False, False, False, extra=(idx,))
    def j_ip_hps(self, part, chroma, idx, ext):
        return self._ip("IP_HPS", "hps", part, chroma, idx, ext, True, ext != 0, False, True, ext_rows=((3 if chroma else 7) if ext else 0), extra=(idx, ext))
    def j_ip_vpp(self, part, chroma, idx): return self._ip("IP_VPP", "vpp", part, chroma, idx, 0, False, True, False, False, extra=(idx,))
    def j_ip_vps(self, part, chroma, idx): return self._ip("IP_VPS", "vps", part, chroma, idx, 0, False, True, False, True, extra=(idx,))
    def j_ip_vsp(self, part, chroma, idx): return self._ip("IP_VSP", "vsp", part, chroma, idx, 0, False, True, True, False, extra=(idx,))
    def j_ip_vss(self, part, chroma, idx): return self._ip("IP_VSS", "vss", part, chroma, idx, 0, False, True, True, True, extra=(idx,))
    def j_ip_hvpp(self, part, ix, iy): return self._ip("IP_HVPP", "hvpp", part, 0, ix, iy, True, True, False, False, extra=(ix, iy))
    def j_ip_p2s(self, part, chroma): return self._ip("IP_P2S", "p2s", part, chroma, 0, 0, False, False, False, True)


def chroma_satd_defined(part):
    """the 4:2:0 half of the partition is a multiple of 4x4 (reference: pixel.cpp:1205-1229; NULL slots otherwise)"""
    return ((PU_SIZES[part][0] >> 1) | (PU_SIZES[part][1] >> 1)) & 3 == 0


def job_family_specs(L, family, mode, seed):
    """JobArena with every (op, size index, filter phase) of the family built, families 0..3 several times over with fresh strides and offsets; arena.specs shuffled"""
    rng = np.random.default_rng(case_seed("jobs%d" % family, L.depth, mode, seed))
    A = JobArena(L, rng, mode)
    parts, cus, tus = range(25), range(5), range(4)
    if family == 0:
        for _ in range(3):
            for part in parts:
                A.j_sad(part); A.j_sad_x3(part); A.j_sad_x4(part); A.j_satd(part)
                if chroma_satd_defined(part):
                    A.j_chroma_satd(part)
            for cu in cus:
                A.j_sa8d(cu); A.j_sse_pp(cu); A.j_sse_ss(cu); A.j_ssd_s(cu); A.j_psy_cost_pp(cu); A.j_var(cu)
                if cu >= 1:
                    A.j_chroma_sa8d(cu)
    elif family == 1:
        for _ in range(3):
            for part in parts:
                A.j_pixelavg_pp(part); A.j_addavg(part, 0); A.j_addavg(part, 1)
            for cu in cus:
                A.j_sub_ps(cu); A.j_add_ps(cu); A.j_transpose(cu)
            for cu in tus:
                A.j_cpy2dto1d_shl(cu); A.j_cpy2dto1d_shr(cu); A.j_cpy1dto2d_shl(cu); A.j_cpy1dto2d_shr(cu); A.j_copy_cnt(cu); A.j_count_nonzero(cu)
            for w in (16, 32, 48, 64):
                A.j_weight_pp(w); A.j_weight_sp(w - 1)
            A.j_scale2d_64to32(); A.j_scale1d_128to64()
    elif family == 2:
        for _ in range(8):
            for cu in tus:
                A.j_quant(cu); A.j_nquant(cu); A.j_dequant_normal(cu); A.j_dequant_scaling(cu)
                for _ in range(3):      # the transforms are the ops with per-wave LDS: most blocks of the shuffled batch should hold several of them
                    A.j_dct(cu); A.j_idct(cu)
            A.j_dst4(); A.j_idst4(); A.j_dst4(); A.j_idst4()
    elif family == 3:
        for cu in tus:
            for m in range(35):
                for bf in (0, 1):
                    A.j_intra_pred(cu, m, bf)
            for _ in range(3):
                A.j_intra_filter(cu); A.j_intra_allangs(cu, 0); A.j_intra_allangs(cu, 1)
    elif family == 4:
        for part in parts:
            for chroma in ((0, 1) if part else (0,)):       # no 2x2 chroma filters (reference: ipfilter.cpp:418-466)
                for idx in range(8 if chroma else 4):
                    A.j_ip_hpp(part, chroma, idx); A.j_ip_hps(part, chroma, idx, 0); A.j_ip_hps(part, chroma, idx, 1)
                    A.j_ip_vpp(part, chroma, idx); A.j_ip_vps(part, chroma, idx); A.j_ip_vsp(part, chroma, idx); A.j_ip_vss(part, chroma, idx)
                A.j_ip_p2s(part, chroma)
            for ix in (1, 2, 3):
                for iy in (1, 2, 3):
                    A.j_ip_hvpp(part, ix, iy)
    else:
        raise ValueError(family)
    order = rng.permutation(len(A.specs))
    A.specs = [A.specs[i] for i in order]
    return A


def job_coverage(specs):
    """{op name: number of distinct keys}"""
    seen = {}
    for s in specs:
        seen.setdefault(JOB_OP_NAME[s.op], set()).add(s.key)
    return {k: len(v) for k, v in seen.items()}


def job_mixed_head(specs, n):
    """n jobs of as many different ops as the list offers, in list order but the ops with per-wave LDS (the transforms) first: the small batches, so that the
    waves of the one or two blocks hold different ops and, in family 2, more than one LDS region is in use"""
    lds = {JOB_OPS[k] for k in ("DCT", "IDCT", "DST4", "IDST4")}
    specs = sorted(specs, key=lambda s: s.op not in lds)
    head, ops = [], set()
    for s in specs:
        if s.op not in ops:
            head.append(s); ops.add(s.op)
        if len(head) == n:
            return head
    return head + [s for s in specs if s not in head][:n - len(head)]


def job_records(specs, in_base, out_base):
    recs = np.zeros(len(specs), JOB_DT)
    for r, s in zip(recs, specs):
        r["op"], r["size"], r["p"], r["sa"], r["sb"], r["sc"], r["sd"] = s.op, s.size, s.p, s.sa, s.sb, s.sc, s.sd
        for base, fields in ((in_base, s.ins), (out_base, s.outs)):
            for f, o in fields.items():
                if f in ("e0", "e1"):
                    r["e"][int(f[1])] = base + o
                else:
                    r[f] = base + o
    return recs


def job_touch(r, depth):
    """Every address range the kernels of csrc/prim_kernels.hip can touch for the record r, from the record alone: [(first byte, one past the last, is a write)].
    The interpolation ranges are those of the shim's interp(): taps / 2 - 1 samples left and above, taps - 1 - (taps / 2 - 1) right and below, the taps - 1 extra
    rows of hps with isRowExt; sad_x3 / sad_x4 read fenc at the reference's 64-element stride."""
    px = 1 if depth == 8 else 2
    op, size, p = JOB_OP_NAME[int(r["op"])], int(r["size"]), [int(v) for v in r["p"]]
    a, b, c, d, e0, e1 = [int(r[f]) for f in "abcd"] + [int(r["e"][0]), int(r["e"][1])]
    sa, sb, sd = int(r["sa"]), int(r["sb"]), int(r["sd"])
    out = []

    def rect(addr, elem, w, h, stride, write=False, block_w=None):
        block_w = w if block_w is None else block_w
        assert stride >= block_w or h == 1, (op, stride, block_w)       # the contract: strides no smaller than the block width
        out.append((addr, addr + ((h - 1) * stride + w) * elem, write))

    def flat(addr, nbytes, write=False):
        out.append((addr, addr + nbytes, write))

    if op in ("SAD", "SAD_X3", "SAD_X4", "SATD", "CHROMA_SATD", "PIXELAVG_PP", "ADDAVG"):
        assert 0 <= size < 25       # the kernels look the partition up in a table of 25
    else:
        assert 0 <= size < 5
    W, H = PU_SIZES[size]
    N = 4 << size
    if op in ("SAD", "SATD", "CHROMA_SATD"):
        w, h = (W // 2, H // 2) if op == "CHROMA_SATD" else (W, H)
        rect(a, px, w, h, sa); rect(b, px, w, h, sb); flat(d, 8, True)
    elif op in ("SAD_X3", "SAD_X4"):
        rect(a, px, W, H, FENC_STRIDE)
        for cand in (b, c, e0, e1)[:3 if op == "SAD_X3" else 4]:
            rect(cand, px, W, H, sb)
        flat(d, 4 * (3 if op == "SAD_X3" else 4), True)
    elif op in ("SA8D", "SSE_PP", "PSY_COST_PP", "CHROMA_SA8D"):
        n = N // 2 if op == "CHROMA_SA8D" else N
        rect(a, px, n, n, sa); rect(b, px, n, n, sb); flat(d, 8, True)
    elif op == "SSE_SS":
        rect(a, 2, N, N, sa); rect(b, 2, N, N, sb); flat(d, 8, True)
    elif op == "SSD_S":
        rect(a, 2, N, N, sa); flat(d, 8, True)
    elif op == "VAR":
        rect(a, px, N, N, sa); flat(d, 8, True)
    elif op == "SUB_PS":
        rect(a, px, N, N, sa); rect(b, px, N, N, sb); rect(d, 2, N, N, sd, True)
    elif op == "ADD_PS":
        rect(a, px, N, N, sa); rect(b, 2, N, N, sb); rect(d, px, N, N, sd, True)
    elif op == "PIXELAVG_PP":
        rect(a, px, W, H, sa); rect(b, px, W, H, sb); rect(d, px, W, H, sd, True)
    elif op == "ADDAVG":
        w, h = W >> p[0], H >> p[0]
        rect(a, 2, w, h, sa); rect(b, 2, w, h, sb); rect(d, px, w, h, sd, True)
    elif op in ("WEIGHT_PP", "WEIGHT_SP"):
        rect(a, px if op == "WEIGHT_PP" else 2, p[0], p[1], sa); rect(d, px, p[0], p[1], sd, True)
    elif op == "SCALE2D_64TO32":
        rect(a, px, 64, 64, sa); flat(d, 32 * 32 * px, True)
    elif op == "SCALE1D_128TO64":
        flat(a, 256 * px); flat(d, 128 * px, True)
    elif op == "TRANSPOSE":
        rect(a, px, N, N, sa); flat(d, N * N * px, True)
    elif op in ("CPY2DTO1D_SHL", "CPY2DTO1D_SHR"):
        rect(a, 2, N, N, sa); flat(d, N * N * 2, True)
    elif op in ("CPY1DTO2D_SHL", "CPY1DTO2D_SHR"):
        flat(a, N * N * 2); rect(d, 2, N, N, sd, True)
    elif op == "COPY_CNT":
        rect(a, 2, N, N, sa); flat(d, N * N * 2, True); flat(e0, 8, True)
    elif op == "COUNT_NONZERO":
        flat(a, N * N * 2); flat(d, 8, True)
    elif op in ("DCT", "DST4"):
        n = 4 if op == "DST4" else N
        rect(a, 2, n, n, sa); flat(d, n * n * 2, True)
    elif op in ("IDCT", "IDST4"):
        n = 4 if op == "IDST4" else N
        flat(a, n * n * 2); rect(d, 2, n, n, sd, True)
    elif op in ("QUANT", "NQUANT"):
        num = p[2]
        flat(a, 2 * num); flat(b, 4 * num); flat(d, 2 * num, True); flat(e1, 8, True)
        if op == "QUANT":
            flat(e0, 4 * num, True)
    elif op in ("DEQUANT_NORMAL", "DEQUANT_SCALING"):
        num = p[0]
        flat(a, 2 * num); flat(d, 2 * num, True)
        if op == "DEQUANT_SCALING":
            flat(b, 4 * num)
    elif op in ("INTRA_PRED", "INTRA_FILTER", "INTRA_ALLANGS"):
        assert 0 <= size < 4        # the kernel's LDS neighbour rows hold 4 * 32 + 1 samples
        flat(a, (4 * N + 1) * px)
        if op == "INTRA_PRED":
            assert 0 <= p[0] < 35
            rect(d, px, N, N, sd, True)
        elif op == "INTRA_FILTER":
            flat(d, (4 * N + 1) * px, True)
        else:
            flat(b, (4 * N + 1) * px); flat(d, 33 * N * N * px, True)
    elif op.startswith("IP_"):
        taps, w, h, idx, aux = p[:5]
        assert taps in (4, 8) and 0 <= idx < (4 if taps == 8 else 8) and w > 0 and h > 0
        half, rest = taps // 2 - 1, taps - 1 - (taps // 2 - 1)
        horiz = op in ("IP_HPP", "IP_HPS", "IP_HVPP")
        vert = op in ("IP_VPP", "IP_VPS", "IP_VSP", "IP_VSS", "IP_HVPP") or (op == "IP_HPS" and aux != 0)
        if op == "IP_HVPP":
            assert 0 <= aux < 4
        se, de = (2 if op in ("IP_VSP", "IP_VSS") else px), (2 if op in ("IP_HPS", "IP_VPS", "IP_VSS", "IP_P2S") else px)
        mx, mxr, mt, mb = (half if horiz else 0), (rest if horiz else 0), (half if vert else 0), (rest if vert else 0)
        rect(a - (mt * sa + mx) * se, se, w + mx + mxr, h + mt + mb, sa, block_w=w)
        rect(d, de, w, h + (taps - 1 if op == "IP_HPS" and aux else 0), sd, True)
    else:
        raise AssertionError("unknown op %r" % op)
    return out


def job_result_field(op):
    """(field, alignment) of the op's scalar result, as the layer-2 comment of include/x265amd.h states it: a 64-bit word in d, or in e[0] / e[1] where the op has
    other use for d; sad_x3 / sad_x4: int32 values in d.  (None, 0): the op has blocks only"""
    if op in ("SAD_X3", "SAD_X4"):
        return "d", 4
    if JOB_OPS[op] // 32 == 0 or op == "COUNT_NONZERO":
        return "d", 8
    if op == "COPY_CNT":
        return "e0", 8
    if op in ("QUANT", "NQUANT"):
        return "e1", 8
    return None, 0


def job_assert_inside(recs, specs, depth, in_base, in_size, out_base, out_size):
    """no record may make a kernel read outside the input arena or write outside its own output region: checked on the host before anything is launched"""
    for i, (r, s) in enumerate(zip(recs, specs)):
        assert int(r["op"]) // 32 == int(recs[0]["op"]) // 32, "job %d: one family per launch" % i
        for lo, hi, write in job_touch(r, depth):
            base, size = (out_base, out_size) if write else (in_base, in_size)
            assert base <= lo < hi <= base + size, "job %d (%s): %s range [%d, %d) outside its arena [0, %d)" % (i, s.name(), "write" if write else "read", lo - base, hi - base, size)
        field, align = job_result_field(JOB_OP_NAME[s.op])
        if field:
            addr = int(r["e"][int(field[1])]) if field in ("e0", "e1") else int(r[field])
            assert addr % align == 0, "job %d (%s): result %s not %d-byte aligned" % (i, s.name(), field, align)
    writes = sorted((lo, hi, i) for i, r in enumerate(recs) for lo, hi, write in job_touch(r, depth) if write)
    for (lo0, hi0, i0), (lo1, hi1, i1) in zip(writes, writes[1:]):
        assert hi0 <= lo1, "jobs %d and %d write overlapping ranges" % (i0, i1)


def job_expected(O, arena, specs):
    """the output arena after the oracle has run the given jobs on the host copies: poison everywhere else"""
    want = arena.poison()
    M = _JobHost(arena.inb, want)
    for s in specs:
        s.oracle(O, M)
    return want


def job_regions(arena, specs, depth):
    """[(first byte, one past the last, job index)] of the output arena, sorted: where each job of the batch writes"""
    recs = job_records(specs, 0, 0)
    reg = []
    for i, r in enumerate(recs):
        # input offsets are taken from base 0 as well, which is harmless here: only the writes are kept
        reg += [(lo, hi, i) for lo, hi, write in job_touch(r, depth) if write]
    return sorted(reg)


def job_compare(arena, specs, depth, got, want, what):
    """whole-arena comparison; a mismatch names the job, its op and size index and the first differing position"""
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    first = int(bad[0])
    reg = job_regions(arena, specs, depth)
    owner = [(lo, hi, i) for lo, hi, i in reg if lo <= first < hi]
    if owner:
        lo, hi, i = owner[0]
        where = "inside the output of job %d (%s), byte %d of its %d" % (i, specs[i].name(), first - lo, hi - lo)
    else:
        before = [(lo, hi, i) for lo, hi, i in reg if hi <= first]
        where = "OUTSIDE every job's output" + (", %d bytes behind that of job %d (%s)" % (first - before[-1][1], before[-1][2], specs[before[-1][2]].name()) if before else "")
    jobs = sorted({i for lo, hi, i in reg if np.any(got[lo:hi] != want[lo:hi])})
    raise AssertionError("%s: %d bytes of the output arena differ, the first at offset %d, %s: got 0x%02x want 0x%02x (poison 0x%02x); jobs with differences: %s"
                         % (what, bad.size, first, where, got[first], want[first], (first * 37 + 11) & 0xFF, jobs[:16]))


def job_run_device(L, arena, specs, family, stream=None):
    """uploads both arenas verbatim, checks every record's reach on the host, launches the batch (stream: None, or a torch.cuda.Stream) and returns the output arena
    as the device left it"""
    import torch
    d_in = torch.from_numpy(arena.inb).cuda()
    d_out = torch.from_numpy(arena.poison()).cuda()
    recs = job_records(specs, d_in.data_ptr(), d_out.data_ptr())
    job_assert_inside(recs, specs, L.depth, d_in.data_ptr(), arena.inb.size, d_out.data_ptr(), arena.out_size)
    d_jobs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    handle = None if stream is None else C.c_void_p(stream.cuda_stream)
    assert L.lib.x265amd_run_jobs(handle, C.c_void_p(d_jobs.data_ptr()), len(specs), family) == 0
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(d_in.cpu().numpy(), arena.inb), "the input arena changed"
    return got
