#!/usr/bin/env python3
"""What it costs to get a device-resident picture into Pic::dSrc, measured on the GPU and written as a table.

  ingest_rate.py [out.md]     default: profiles/ingest_rate.md

For 1920x1080 (coded 1920x1080) and 3840x2160, the time from a picture that lies in device memory to a complete padded source picture (margins 96 / 80):

  ingest      x265amd_ingest_picture, one launch: planar at the library's depth (both libraries), NV12 into the 8-bit library, P010 (16-bit words, bitDepth 16) into the
              10-bit and into the 8-bit library
  upload      the sequence x265amd_encoder::uploadPicture(onDevice) issues for a planar picture of the library's depth, call for call on the NULL stream: hipMemsetAsync of
              the whole buffer, per plane hipMemcpy2DAsync and x265amd_extend_pic_border (twice when the size is padded; neither of these sizes is).  Those calls are the
              same code in the commit before the ingest pass and in this one; run the script in a checkout of that commit (it then skips `ingest`) to measure it there.

HIP events around one picture's work, the median of 20 after 5 warm-up runs.  Next to each time: the bytes the work has to read (the source samples once) plus the bytes it
has to write (every element of the flat buffer once; the upload sequence writes the buffer twice over where it copies: the memset's bytes are counted too), and that figure
over the time as a fraction of the HBM peak (8 TB/s).  A picture fits the last-level cache, so the fraction says how far the work is from the memory system's best, not
where the bytes came from.  Needs a GPU; no threshold is set on anything here.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hevc_testlib as T

RUNS, WARMUP = 20, 5
HBM_PEAK = 8.0e12
MARGINS = (96, 80)
SIZES = ((1920, 1080), (3840, 2160))


class Surface(C.Structure):
    _fields_ = [("planes", C.c_void_p * 3), ("stride", C.c_int32 * 3), ("bitDepth", C.c_int32), ("layout", C.c_int32), ("clipMin", C.c_int32), ("clipMax", C.c_int32),
                ("reserved", C.c_int32)]


def hip_runtime():
    """the HIP runtime this process has loaded already (torch's, which the library binds to as well: tests/hevc_testlib.py load_hip)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            rt = C.CDLL(line.split()[-1])
            rt.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
            rt.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
            return rt
    raise RuntimeError("no HIP runtime is loaded")


def geometry(W, H, mx, my):
    stride, cstride = W + 2 * mx, W // 2 + mx
    ysz, csz = (H + 2 * my) * stride, (H // 2 + my) * cstride
    return dict(stride=stride, cstride=cstride, org=(my * stride + mx, ysz + (my // 2) * cstride + mx // 2, ysz + csz + (my // 2) * cstride + mx // 2), total=ysz + 2 * csz)


def timed(fn):
    import torch
    ms = []
    for it in range(WARMUP + RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def measure():
    import torch
    rows = []
    libs = {d: T.load_hip(d).lib for d in (8, 10)}
    rt = hip_runtime()
    for lib in libs.values():
        lib.x265amd_last_error.restype = C.c_char_p
        lib.x265amd_extend_pic_border.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
        if hasattr(lib, "x265amd_ingest_picture"):
            lib.x265amd_ingest_picture.argtypes = [C.c_void_p, C.POINTER(Surface), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    have_ingest = hasattr(libs[8], "x265amd_ingest_picture")
    rng = np.random.default_rng(1)
    mx, my = MARGINS
    for (w, h) in SIZES:
        g = geometry(w, h, mx, my)
        for lib_depth in (8, 10):
            lib, osz = libs[lib_depth], (2 if lib_depth > 8 else 1)
            dst = torch.zeros(g["total"] * osz, dtype=torch.uint8, device="cuda")
            written = g["total"] * osz

            def source(isz, top, semi):
                shapes = [(h, w), (h // 2, w)] if semi else [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
                host = [rng.integers(0, top, s).astype(np.uint16 if isz == 2 else np.uint8) for s in shapes]
                return [torch.from_numpy(p.view(np.uint8).reshape(p.shape[0], -1)).cuda() for p in host]

            cases = [("planar %d-bit" % lib_depth, lib_depth, 0)]
            cases += [("NV12", 8, 1)] if lib_depth == 8 else []
            cases += [("P010 (bitDepth 16)", 16, 1)]
            for name, depth, semi in cases if have_ingest else []:
                isz = 2 if depth > 8 else 1
                planes = source(isz, 1 << (depth if depth != 16 else 16), semi)
                s = Surface()
                for k, t in enumerate(planes):
                    s.planes[k] = t.data_ptr(); s.stride[k] = t.stride(0)
                s.bitDepth, s.layout, s.clipMin, s.clipMax = depth, semi, -1, -1
                torch.cuda.synchronize()

                def ingest():
                    assert lib.x265amd_ingest_picture(None, C.byref(s), w, h, dst.data_ptr(), w, h, mx, my) == 0, lib.x265amd_last_error()

                med, lo, hi = timed(ingest)
                nbytes = w * h * 3 // 2 * isz + written
                rows.append(dict(size="%dx%d" % (w, h), library=lib_depth, what="ingest: " + name, launches=1, ms_median=med, ms_min=lo, ms_max=hi, bytes=nbytes,
                                 fraction_of_hbm_peak=nbytes / (med * 1e-3) / HBM_PEAK))
            planes = source(osz, 1 << lib_depth, 0)
            torch.cuda.synchronize()

            def upload():
                assert rt.hipMemsetAsync(dst.data_ptr(), 0, written, None) == 0
                for k, t in enumerate(planes):
                    pw, ph, st = (w >> (k > 0)), (h >> (k > 0)), (g["cstride"] if k else g["stride"])
                    org = dst.data_ptr() + g["org"][k] * osz
                    assert rt.hipMemcpy2DAsync(org, st * osz, t.data_ptr(), t.stride(0), pw * osz, ph, 3, None) == 0          # hipMemcpyDeviceToDevice
                    assert lib.x265amd_extend_pic_border(None, org, st, pw, ph, mx >> (k > 0), my >> (k > 0)) == 0, lib.x265amd_last_error()

            med, lo, hi = timed(upload)
            nbytes = w * h * 3 // 2 * osz + written + written           # the samples read, the buffer zeroed, the buffer written
            rows.append(dict(size="%dx%d" % (w, h), library=lib_depth, what="upload sequence (memset, 3 x 2-D copy, 3 x border)", launches=7, ms_median=med, ms_min=lo, ms_max=hi,
                             bytes=nbytes, fraction_of_hbm_peak=nbytes / (med * 1e-3) / HBM_PEAK))
    return torch.cuda.get_device_name(0), have_ingest, rows


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ingest_rate.md")
    device, have_ingest, rows = measure()
    lines = ["# From a device-resident picture to a complete padded source picture", "",
             "Written by `dbg/ingest_rate.py` on %s: HIP events around one picture's work, the median of %d after %d warm-up runs, margins %d / %d." % (device, RUNS, WARMUP, MARGINS[0], MARGINS[1]),
             "Bytes: the source samples read once plus every element of the flat buffer written once (the upload sequence: plus the memset's bytes); the fraction is that",
             "figure over the time against an HBM peak of 8 TB/s.  A picture fits the last-level cache.  No threshold is set on any of this.", ""]
    if not have_ingest:
        lines += ["This build has no `x265amd_ingest_picture`: only the upload sequence was measured.", ""]
    lines += ["| size | library | work | calls | ms (median) | ms (min .. max) | MB | of the HBM peak |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d-bit | %s | %d | %.4f | %.4f .. %.4f | %.2f | %.1f %% |" % (r["size"], r["library"], r["what"], r["launches"], r["ms_median"], r["ms_min"], r["ms_max"],
                                                                                       r["bytes"] / 1e6, 100 * r["fraction_of_hbm_peak"]))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(dict(device=device, rows=rows)))


if __name__ == "__main__":
    main()
