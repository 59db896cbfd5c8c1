"""What the tests of the SAO options share (--sao-non-deblock, --limit-sao, --selective-sao): the plane sets, a restatement of the reference's two statistics functions
written from source/encoder/sao.cpp line by line (loops over Python lists, no vector tricks), the ctypes mirror of x265amd_param_ext and the calls into the library's
host model.  tests/test_sao_options.py (CPU), tests/test_hip_sao_options.py and tests/test_encoder_sao_options.py (GPU) and tests/golden/make_sao_options_golden.py
read it; nothing here needs a GPU."""
import ctypes as C

import numpy as np

import hevc_testlib as T

NON_DEBLOCK, EO01_ONLY = 1, 2           # X265AMD_SAO_* (include/x265amd.h; tests/native/abi_layout_sao_check.cpp pins the numbers)
WORDS = 5 * 32                          # per (CTU, plane): type 0..3 = EO_0..3 (classes 0..4), 4 = BO (32 bands)

# the smallest sizes at which the statistics can go wrong: one CTU that is at the right and bottom edge at once with nothing above or left; no partial CTU;
# a last column of 8 and a last row of 8; of 8 and 24
SHAPES = [(64, 64), (128, 128), (136, 72), (200, 152)]
CONTENTS = ["noise", "flat", "checker", "ramp_h", "ramp_v", "ramp_d135", "ramp_d45"]


class ParamExt(C.Structure):            # x265amd_param_ext (include/x265amd_encoder.h; tests/native/abi_layout_sao_check.cpp pins the layout)
    _fields_ = [("size", C.c_uint32), ("bSaoNonDeblocked", C.c_int32), ("bLimitSAO", C.c_int32), ("selectiveSAO", C.c_int32), ("reserved", C.c_int32 * 12)]


def nctu(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def _lcg(seed, n):
    """a 32-bit linear congruential generator (Numerical Recipes' constants), its top bits"""
    out, s = [0] * n, seed
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xffffffff
        out[i] = s >> 8
    return np.array(out, np.int64)


def _field(name, w, h, depth, seed):
    pmax = (1 << depth) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "noise":
        # 24 levels over the whole range: 24 bands, and neighbours tie often enough that the classes with one equal neighbour are not empty in a strip of a few hundred samples
        return (_lcg(seed, w * h).reshape(h, w) % 24) * ((pmax + 1) // 24)
    if name == "flat":
        return np.full((h, w), pmax // 2 + (seed % 3), np.int64)
    if name == "checker":
        return np.where((xx + yy + seed) & 1, pmax, 0).astype(np.int64)
    step = {"ramp_h": xx, "ramp_v": yy, "ramp_d135": xx + yy, "ramp_d45": xx - yy + h}[name]
    return ((step // 2 + seed) % (pmax + 1)).astype(np.int64)          # steps two samples wide: neighbours tie as often as they differ


def plane_set(content, w, h, depth):
    """(rec, fenc, pre): three lists of Y, U, V planes at their exact sizes.  rec = the deblocked picture, pre = the picture before deblocking -- for the noise set an
    INDEPENDENT field, so that a kernel reading the wrong one shows; for the others a shifted one --, fenc = the source: the largest differences for the checkerboard"""
    dt = np.uint8 if depth == 8 else np.uint16
    rec, fenc, pre = [], [], []
    for k, (pw, ph) in enumerate(((w, h), (w // 2, h // 2), (w // 2, h // 2))):
        r = _field(content, pw, ph, depth, 11 + k)
        p = _field(content, pw, ph, depth, 500 + k)         # (the checkerboard's other phase, another level of the flat plane, the ramps shifted)
        pmax = (1 << depth) - 1
        f = _field("noise", pw, ph, depth, 900 + k)
        if content == "checker":
            f = pmax - r                                    # every difference is +pmax or -pmax
        elif content != "noise":
            f = np.clip(r + (f % 13) - 6, 0, pmax)
        rec.append(np.ascontiguousarray(r.astype(dt))); fenc.append(np.ascontiguousarray(f.astype(dt))); pre.append(np.ascontiguousarray(p.astype(dt)))
    return rec, fenc, pre


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# source/encoder/sao.cpp restated.  s_eoTable (:65-72), signOf, the primitives saoCuStatsBO_c / E0_c .. E3_c (:1762-1925) and the two callers.  A plane is a list
# of rows; `at(p, x, y)` is rec0[y * stride + x] relative to the CTU's first sample.
EO_TABLE = [1, 2, 0, 3, 4]


def sign_of(v):
    return (v > 0) - (v < 0)


class _Rel:
    """a plane seen from a CTU's first sample: r[y][x] with negative and overhanging coordinates inside the picture"""
    def __init__(self, rows, lpelx, tpely):
        self.rows, self.x0, self.y0 = rows, lpelx, tpely

    def at(self, x, y):
        gx, gy = self.x0 + x, self.y0 + y
        assert 0 <= gy < len(self.rows) and 0 <= gx < len(self.rows[0]), "the reference would read outside the picture: (%d, %d)" % (gx, gy)
        return self.rows[gy][gx]


def _geometry(width, height, cx, cy, plane):
    sh = 1 if plane else 0
    pic_w, pic_h = width >> sh, height >> sh
    lpelx, tpely = (cx * 64) >> sh, (cy * 64) >> sh
    rpelx, bpely = min(lpelx + (64 >> sh), pic_w), min(tpely + (64 >> sh), pic_h)
    return pic_w, pic_h, lpelx, tpely, rpelx, bpely


def calc_sao_stats_ctu(rec_rows, fenc_rows, width, height, cx, cy, plane, non_deblock, limit_b_slice, depth):
    """SAO::calcSaoStatsCTU (:735-917) for one CTU and plane -> (count[5][32], offsetOrg[5][32]).  limit_b_slice: param.bLimitSAO in a B slice (:861)"""
    count = [[0] * 32 for _ in range(5)]; stats = [[0] * 32 for _ in range(5)]
    pic_w, pic_h, lpelx, tpely, rpelx, bpely = _geometry(width, height, cx, cy, plane)
    ctu_w, ctu_h = rpelx - lpelx, bpely - tpely
    above_unavail = 1 if not tpely else 0
    rec, fenc = _Rel(rec_rows, lpelx, tpely), _Rel(fenc_rows, lpelx, tpely)
    plane_offset = 2 if plane else 0
    skip_b, skip_r = 4, 5
    diff = [[fenc.at(x, y) - rec.at(x, y) for x in range(ctu_w)] for y in range(ctu_h)]
    bo_shift = depth - 5
    # SAO_BO
    if non_deblock:
        skip_b, skip_r = 3, 4
    end_x = ctu_w if rpelx == pic_w else ctu_w - skip_r + plane_offset
    end_y = ctu_h if bpely == pic_h else ctu_h - skip_b + plane_offset
    for y in range(end_y):
        for x in range(end_x):
            cl = rec.at(x, y) >> bo_shift
            stats[4][cl] += diff[y][x]; count[4][cl] += 1
    # SAO_EO_0
    if non_deblock:
        skip_b, skip_r = 3, 5
    start_x = 1 if not lpelx else 0
    end_x = ctu_w - 1 if rpelx == pic_w else ctu_w - skip_r + plane_offset
    tmp_s, tmp_c = [0] * 5, [0] * 5
    for y in range(ctu_h - skip_b + plane_offset):
        sign_left = sign_of(rec.at(start_x, y) - rec.at(start_x - 1, y))
        for x in range(end_x - start_x):
            sign_right = sign_of(rec.at(start_x + x, y) - rec.at(start_x + x + 1, y))
            edge = sign_right + sign_left + 2
            sign_left = -sign_right
            tmp_s[edge] += diff[y][start_x + x]; tmp_c[edge] += 1
    for e in range(5):
        stats[0][EO_TABLE[e]] += tmp_s[e]; count[0][EO_TABLE[e]] += tmp_c[e]
    # SAO_EO_1
    if non_deblock:
        skip_b, skip_r = 4, 4
    start_y = above_unavail
    end_x = ctu_w if rpelx == pic_w else ctu_w - skip_r + plane_offset
    end_y = ctu_h - 1 if bpely == pic_h else ctu_h - skip_b + plane_offset
    up = [sign_of(rec.at(x, start_y) - rec.at(x, start_y - 1)) for x in range(ctu_w)]
    tmp_s, tmp_c = [0] * 5, [0] * 5
    for y in range(end_y - start_y):
        for x in range(end_x):
            sign_down = sign_of(rec.at(x, start_y + y) - rec.at(x, start_y + y + 1))
            edge = sign_down + up[x] + 2
            up[x] = -sign_down
            tmp_s[edge] += diff[start_y + y][x]; tmp_c[edge] += 1
    for e in range(5):
        stats[1][EO_TABLE[e]] += tmp_s[e]; count[1][EO_TABLE[e]] += tmp_c[e]
    if not limit_b_slice:
        # SAO_EO_2
        if non_deblock:
            skip_b, skip_r = 4, 5
        start_x = 1 if not lpelx else 0
        end_x = ctu_w - 1 if rpelx == pic_w else ctu_w - skip_r + plane_offset
        start_y = above_unavail
        end_y = ctu_h - 1 if bpely == pic_h else ctu_h - skip_b + plane_offset
        up1 = [0] * (ctu_w + 2); upt = [0] * (ctu_w + 2)
        for i in range(end_x - start_x):
            up1[i] = sign_of(rec.at(start_x + i, start_y) - rec.at(start_x + i - 1, start_y - 1))
        tmp_s, tmp_c = [0] * 5, [0] * 5
        for y in range(end_y - start_y):
            upt[0] = sign_of(rec.at(start_x, start_y + y + 1) - rec.at(start_x - 1, start_y + y))
            for x in range(end_x - start_x):
                sign_down = sign_of(rec.at(start_x + x, start_y + y) - rec.at(start_x + x + 1, start_y + y + 1))
                edge = sign_down + up1[x] + 2
                upt[x + 1] = -sign_down
                tmp_s[edge] += diff[start_y + y][start_x + x]; tmp_c[edge] += 1
            up1, upt = upt, up1
        for e in range(5):
            stats[2][EO_TABLE[e]] += tmp_s[e]; count[2][EO_TABLE[e]] += tmp_c[e]
        # SAO_EO_3
        if non_deblock:
            skip_b, skip_r = 4, 5
        up_all = [0] * (ctu_w + 3)          # upBuff1 of the caller; the primitive is handed upBuff1 + 1
        for i in range(end_x - start_x + 1):
            up_all[i] = sign_of(rec.at(start_x - 1 + i, start_y) - rec.at(start_x - 1 + i + 1, start_y - 1))
        tmp_s, tmp_c = [0] * 5, [0] * 5
        n = end_x - start_x
        for y in range(end_y - start_y):
            for x in range(n):
                sign_down = sign_of(rec.at(start_x + x, start_y + y) - rec.at(start_x + x - 1, start_y + y + 1))
                edge = sign_down + up_all[1 + x] + 2
                up_all[1 + x - 1] = -sign_down
                tmp_s[edge] += diff[start_y + y][start_x + x]; tmp_c[edge] += 1
            up_all[1 + n - 1] = sign_of(rec.at(start_x + n - 1, start_y + y + 1) - rec.at(start_x + n, start_y + y))
        for e in range(5):
            stats[3][EO_TABLE[e]] += tmp_s[e]; count[3][EO_TABLE[e]] += tmp_c[e]
    return count, stats


def calc_sao_stats_cu_before_dblk(rec_rows, fenc_rows, width, height, cx, cy, plane, depth):
    """SAO::calcSaoStatsCu_BeforeDblk (:919-1197) for one CTU and plane (the function loops over the planes itself: plane_offset is 0 for luma, 2 for both chroma
    planes).  Buffers the reference leaves uninitialised are None here: a statistic made of one would raise"""
    count = [[0] * 32 for _ in range(5)]; stats = [[0] * 32 for _ in range(5)]
    pic_w, pic_h, lpelx, tpely, rpelx, bpely = _geometry(width, height, cx, cy, plane)
    ctu_w, ctu_h = rpelx - lpelx, bpely - tpely
    above_avail = 1 if not tpely else 0         # the reference's name for "above unavailable"
    rec, fenc = _Rel(rec_rows, lpelx, tpely), _Rel(fenc_rows, lpelx, tpely)
    plane_offset = 2 if plane else 0
    bo_shift = depth - 5
    # SAO_BO
    skip_b, skip_r = 3 - plane_offset, 4 - plane_offset
    start_x = ctu_w if rpelx == pic_w else ctu_w - skip_r
    start_y = ctu_h if bpely == pic_h else ctu_h - skip_b
    for y in range(ctu_h):
        for x in range(start_x if y < start_y else 0, ctu_w):
            cl = rec.at(x, y) >> bo_shift
            stats[4][cl] += fenc.at(x, y) - rec.at(x, y); count[4][cl] += 1
    # SAO_EO_0
    skip_b, skip_r = 3 - plane_offset, 5 - plane_offset
    start_x = ctu_w - 1 if rpelx == pic_w else ctu_w - skip_r
    start_y = ctu_h if bpely == pic_h else ctu_h - skip_b
    first_x = 1 if not lpelx else 0
    end_x = ctu_w - 1
    for y in range(ctu_h):
        x = start_x if y < start_y else first_x
        sign_left = sign_of(rec.at(x, y) - rec.at(x - 1, y))
        while x < end_x:
            sign_right = sign_of(rec.at(x, y) - rec.at(x + 1, y))
            edge = sign_right + sign_left + 2
            sign_left = -sign_right
            stats[0][EO_TABLE[edge]] += fenc.at(x, y) - rec.at(x, y); count[0][EO_TABLE[edge]] += 1
            x += 1
    # SAO_EO_1
    skip_b, skip_r = 4 - plane_offset, 4 - plane_offset
    start_x = ctu_w if rpelx == pic_w else ctu_w - skip_r
    start_y = ctu_h - 1 if bpely == pic_h else ctu_h - skip_b
    first_y = above_avail
    end_y = ctu_h - 1
    up1 = [None] * (ctu_w + 2)
    for x in range(start_x, ctu_w):
        up1[x] = sign_of(rec.at(x, first_y) - rec.at(x, first_y - 1))
    for y in range(first_y, end_y):
        for x in range(start_x if y < start_y - 1 else 0, ctu_w):
            sign_down = sign_of(rec.at(x, y) - rec.at(x, y + 1))
            up = up1[x]
            up1[x] = -sign_down
            if x < start_x and y < start_y:
                continue
            edge = sign_down + up + 2
            stats[1][EO_TABLE[edge]] += fenc.at(x, y) - rec.at(x, y); count[1][EO_TABLE[edge]] += 1
    # SAO_EO_2
    skip_b, skip_r = 4 - plane_offset, 5 - plane_offset
    start_x = ctu_w - 1 if rpelx == pic_w else ctu_w - skip_r
    start_y = ctu_h - 1 if bpely == pic_h else ctu_h - skip_b
    first_x = 1 if not lpelx else 0
    first_y = above_avail
    end_x, end_y = ctu_w - 1, ctu_h - 1
    up1 = [None] * (ctu_w + 2); upt = [None] * (ctu_w + 2)
    for x in range(start_x, end_x):
        up1[x] = sign_of(rec.at(x, first_y) - rec.at(x - 1, first_y - 1))
    for y in range(first_y, end_y):
        x = start_x if y < start_y - 1 else first_x
        upt[x] = sign_of(rec.at(x, y + 1) - rec.at(x - 1, y))
        while x < end_x:
            sign_down = sign_of(rec.at(x, y) - rec.at(x + 1, y + 1))
            up = up1[x]
            upt[x + 1] = -sign_down
            if not (x < start_x and y < start_y):
                edge = sign_down + up + 2
                stats[2][EO_TABLE[edge]] += fenc.at(x, y) - rec.at(x, y); count[2][EO_TABLE[edge]] += 1
            x += 1
        up1, upt = upt, up1
    # SAO_EO_3
    skip_b, skip_r = 4 - plane_offset, 5 - plane_offset
    start_x = ctu_w - 1 if rpelx == pic_w else ctu_w - skip_r
    start_y = ctu_h - 1 if bpely == pic_h else ctu_h - skip_b
    up1 = {}
    for x in range(start_x - 1, end_x):
        up1[x] = sign_of(rec.at(x, first_y) - rec.at(x + 1, first_y - 1))
    for y in range(first_y, end_y):
        for x in range(start_x if y < start_y - 1 else first_x, end_x):
            sign_down = sign_of(rec.at(x, y) - rec.at(x - 1, y + 1))
            up = up1.get(x)
            up1[x - 1] = -sign_down
            if x < start_x and y < start_y:
                continue
            edge = sign_down + up + 2
            stats[3][EO_TABLE[edge]] += fenc.at(x, y) - rec.at(x, y); count[3][EO_TABLE[edge]] += 1
        up1[end_x - 1] = sign_of(rec.at(end_x - 1, y + 1) - rec.at(end_x, y))
    return count, stats


def restated_picture(planes, fenc, width, height, depth, per_ctu):
    """per_ctu(rec rows, fenc rows, cx, cy, plane) -> (count, stats) for every CTU and plane, in the layout of d_count / d_offset_org"""
    ctu_w, ctu_h = (width + 63) // 64, (height + 63) // 64
    cnt = np.zeros((ctu_w * ctu_h, 3, 5, 32), np.int32); org = np.zeros_like(cnt)
    rows = [p.astype(np.int64).tolist() for p in planes]; frows = [p.astype(np.int64).tolist() for p in fenc]
    for cy in range(ctu_h):
        for cx in range(ctu_w):
            for plane in range(3):
                c, s = per_ctu(rows[plane], frows[plane], cx, cy, plane)
                cnt[cy * ctu_w + cx, plane] = c; org[cy * ctu_w + cx, plane] = s
    return cnt.reshape(-1), org.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _tab(planes):
    return (C.c_void_p * 3)(*[p.ctypes.data for p in planes])


def model(lib, rec, fenc, pre, w, h, flags, want_post=True, want_pre=False):
    """x265amd_sao_stats_model on exact-size planes -> dict(count, org, pre_count, pre_org)"""
    fn = lib.x265amd_sao_stats_model
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = nctu(w, h) * 3 * WORDS
    out = {k: np.full(n, -77, np.int32) for k in ("count", "org", "pre_count", "pre_org")}
    rc = fn(_tab(rec) if want_post else None, _tab(fenc), _tab(pre) if want_pre else None, w, w // 2, w, h, flags,
            out["pre_count"].ctypes.data if want_pre else None, out["pre_org"].ctypes.data if want_pre else None,
            out["count"].ctypes.data if want_post else None, out["org"].ctypes.data if want_post else None)
    assert rc == 0, rc
    return out


def classes_covered(count_words):
    """per (CTU, plane) record array [n, 3, 5, 32]: every class 0..4 of every edge type and at least eight bands non-zero in SOME record"""
    c = np.asarray(count_words).reshape(-1, 5, 32)
    edge = (c[:, :4, :5] > 0).any(axis=0).all()
    bands = int((c[:, 4, :] > 0).any(axis=0).sum())
    return bool(edge) and bands >= 8


def open_ext(lib, prm, ext):
    lib.x265amd_encoder_open_ext.restype = C.c_void_p
    lib.x265amd_encoder_open_ext.argtypes = [C.POINTER(T.EncParam), C.c_void_p]
    return lib.x265amd_encoder_open_ext(C.byref(prm), C.byref(ext) if ext is not None else None)


def encoder_run_ext(L, planes_per_frame, width, height, ext_fields, **overrides):
    """hevc_testlib.encoder_run through x265amd_encoder_open_ext: ext_fields = the members of x265amd_param_ext (None: a NULL record).  Returns the whole byte stream and
    the number of pictures coded"""
    lib = L.lib
    lib.x265amd_encoder_headers.argtypes = [C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32)]
    lib.x265amd_encoder_encode.argtypes = [C.c_void_p, C.POINTER(C.POINTER(T.EncNal)), C.POINTER(C.c_uint32), C.POINTER(T.EncPicture), C.POINTER(T.EncPicture)]
    lib.x265amd_encoder_close.argtypes = [C.c_void_p]
    lib.x265amd_param_default.argtypes = [C.POINTER(T.EncParam)]
    lib.x265amd_last_error.restype = C.c_char_p
    prm = T.EncParam()
    lib.x265amd_param_default(C.byref(prm))
    prm.sourceWidth, prm.sourceHeight = width, height
    for k, v in overrides.items():
        assert hasattr(prm, k), k
        setattr(prm, k, v)
    ext = None
    if ext_fields is not None:
        ext = ParamExt(size=C.sizeof(ParamExt), **ext_fields)
    enc = open_ext(lib, prm, ext)
    assert enc, lib.x265amd_last_error()
    stream, coded = bytearray(), 0
    nal = C.POINTER(T.EncNal)(); nnal = C.c_uint32(0)
    try:
        assert lib.x265amd_encoder_headers(enc, C.byref(nal), C.byref(nnal)) > 0
        for i in range(nnal.value):
            stream += bytes(nal[i].payload[:nal[i].sizeBytes])
        for planes in list(planes_per_frame) + [None]:
            while True:
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
                if planes is not None or not ret:           # one call per input picture; the flush until nothing comes
                    break
    finally:
        lib.x265amd_encoder_close(enc)
    return np.frombuffer(bytes(stream), np.uint8), coded
