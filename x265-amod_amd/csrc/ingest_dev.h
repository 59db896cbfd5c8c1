/* The sample conversion of the picture ingest pass (csrc/ingest_kernels.hip) and of its host model (host/ingest_model.cpp): the few lines the two share.
 * PicYuv::copyFromPicture chooses by the picture's depth b and the build's depth (source/common/picyuv.cpp:298-396):
 *   b == 8, 8-bit build      copy                                   (:327-352, memcpy)
 *   b == 8, deeper build     v << (DEPTH - 8), NO mask              (:300-320, planecopy_cp: pixel.cpp planecopy_cp_c)
 *   b > 8, b > DEPTH         (v >> (b - DEPTH)) & ((1 << DEPTH) - 1) (:366-370, :385-388, planecopy_sp)
 *   b > 8, b <= DEPTH        (v << (DEPTH - b)) & mask, b == DEPTH too (:371-375, :390-394, planecopy_sp_shl)
 * and the luma clip that follows (:413-424): min with the upper bound first, then max with the lower. */
#ifndef X265AMD_INGEST_DEV_H
#define X265AMD_INGEST_DEV_H
#include <stdint.h>
#include "../../include/x265amd.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XA_INGEST_HD __host__ __device__
#else
#define XA_INGEST_HD
#endif

/* v: the source sample as it was read (8 or 16 bits, every bit of the word); b: x265_picture.bitDepth, 8..16 */
XA_INGEST_HD inline uint32_t xa_ingest_conv(uint32_t v, int b)
{
    if (b == 8) return X265AMD_DEPTH > 8 ? v << (X265AMD_DEPTH - 8) : v;
    const uint32_t mask = (1u << X265AMD_DEPTH) - 1;
    return b > X265AMD_DEPTH ? (v >> (b - X265AMD_DEPTH)) & mask : (v << (X265AMD_DEPTH - b)) & mask;
}
/* lo / hi: the bounds in force (0 and the largest sample when one is not set) */
XA_INGEST_HD inline uint32_t xa_ingest_clip(uint32_t v, uint32_t lo, uint32_t hi)
{
    v = v < hi ? v : hi;
    return v > lo ? v : lo;
}

/* What x265amd_ingest_picture and x265amd_ingest_model refuse, by name, before anything is read or written: NULL when the arguments are in order.  (Argument checks only:
 * the two compute separately.) */
inline const char* xa_ingest_check(const x265amd_surface* s, int srcW, int srcH, int W, int H, int marginX, int marginY)
{
    if (!s) return "null surface";
    if (s->layout != 0 && s->layout != 1) return "layout: 0 (planar 4:2:0) or 1 (semi-planar 4:2:0)";
    if (s->bitDepth < 8 || s->bitDepth > 16) return "bitDepth outside 8..16";
    if (srcW <= 0 || srcH <= 0 || (srcW & 1) || (srcH & 1)) return "srcW / srcH must be positive and even (4:2:0)";
    if (W < srcW || H < srcH || (W & 1) || (H & 1) || marginX < 0 || marginY < 0) return "W / H below srcW / srcH or odd, or a negative margin";
    const int isz = s->bitDepth > 8 ? 2 : 1, nplanes = s->layout ? 2 : 3;
    for (int k = 0; k < nplanes; k++)
    {
        const int rowBytes = (k == 0 || s->layout ? srcW : srcW / 2) * isz;          /* (a semi-planar chroma row holds srcW / 2 pairs) */
        if (!s->planes[k]) return "null plane";
        if (s->stride[k] < rowBytes) return "stride below the row's bytes";
        if (isz == 2 && ((s->stride[k] & 1) || ((uintptr_t)s->planes[k] & 1))) return "16-bit samples at an odd stride or an odd address (alignment)";
    }
    const int pmax = (1 << X265AMD_DEPTH) - 1;
    if (s->clipMin < -1 || s->clipMax < -1 || s->clipMin > pmax || s->clipMax > pmax || (s->clipMin >= 0 && s->clipMax >= 0 && s->clipMin > s->clipMax))
        return "clipMin / clipMax outside the pixel range or crossed";
    return nullptr;
}
#endif
