/* Picture ingest (include/x265amd.h: x265amd_ingest_picture): a caller's surface -- any sample depth from 8 to 16 bits, three planes or luma +
 * interleaved chroma (NV12, P010 / P016) -- becomes the encoder's padded source picture in ONE launch.
 *
 * What it restates: PicYuv::copyFromPicture (source/common/picyuv.cpp:261-515: the plane copies with their shifts and masks :298-396, the luma clip :413-424, the pad up to
 * the coded size :479-514) and extendPicBorder (source/common/pixel.cpp:1044-1058) behind it.  Both replicate edge samples, so every sample of the padded area is
 *     dst(x, y) = conv(src(clamp(x, 0, sw - 1), clamp(y, 0, sh - 1)))
 * on its own: no second pass, no order between threads, no atomics, no LDS.
 *
 * Bandwidth work (a 1080p 8-bit picture: 3.1 MB read, 3.9 MB written).  A lane owns 16 bytes of one destination row -- 16 samples of the 8-bit library, 8 of the 10-bit --
 * and a wave 1 KiB of it.  The chunks of a row are anchored at the row's first 16-byte boundary: chunk 0 is the scalar head in front of it, the last chunk the scalar
 * tail, every chunk between is one 16-byte store.  A chunk that lies inside the source row reads its samples with vector loads when the source address allows it (8, 16
 * or 2 x 16 bytes); chunks that touch the pad or a margin, and sources at odd offsets, read sample by sample (the clamped re-reads of the first / last row and column hit
 * in L2).  Semi-planar chroma: one lane reads the U,V pairs of its chunk once (two loads) and stores the U and the V chunk (two 16-byte stores when the V row is
 * aligned like the U row, as it is for the encoder's geometry).  The kernel writes EVERY element of the flat buffer -- with odd margins the few chroma elements outside
 * the padded area as zeros -- so no memset runs in front of it. */
#include "x265amd_dev.h"
#include "x265amd_host.h"
#include "ingest_dev.h"
#include <string.h>

namespace {

constexpr int VPT = 16 / (int)sizeof(pixel);        /* samples per lane: 16 bytes of destination */

struct IngestArgs
{
    const uint8_t* src[3]; long srcStride[3];       /* bytes */
    pixel* dst;                                     /* the flat Y | U | V buffer */
    long stride, cstride, ysz, csz;                 /* elements */
    int sw, sh, W, H, mx, my;                       /* luma geometry; chroma: half of everything */
    int yRows, cRows;                               /* rows of the luma plane and of one chroma plane in the buffer */
    int bitDepth, clip;
    uint32_t lo, hi;
};

/* N consecutive samples of type S into words of their own: vector loads when the address is aligned to them */
template<typename S, int N> __device__ inline void load_run(const S* p, uint32_t* out)
{
    constexpr int BYTES = N * (int)sizeof(S), VB = BYTES >= 16 ? 16 : 8, PER = 4 / (int)sizeof(S), BITS = 8 * (int)sizeof(S);
    static_assert(BYTES % VB == 0, "a run is a whole number of vector loads");
    if (((uintptr_t)p & (VB - 1)) == 0)
    {
        uint32_t w[BYTES / 4];
#pragma unroll
        for (int k = 0; k < BYTES / VB; k++)
        {
            if (VB == 16) { const uint4 q = reinterpret_cast<const uint4*>(p)[k]; w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w; }
            else { const uint2 q = reinterpret_cast<const uint2*>(p)[k]; w[2 * k] = q.x; w[2 * k + 1] = q.y; }
        }
#pragma unroll
        for (int i = 0; i < N; i++) out[i] = (w[i / PER] >> (BITS * (i % PER))) & ((1u << BITS) - 1);
    }
    else
    {
#pragma unroll
        for (int i = 0; i < N; i++) out[i] = p[i];
    }
}

/* n <= VPT samples to a destination row: one 16-byte store for a whole, aligned chunk */
__device__ inline void store_run(pixel* p, const uint32_t* v, int n)
{
    if (n == VPT && ((uintptr_t)p & 15) == 0)
    {
        constexpr int PER = 4 / (int)sizeof(pixel), BITS = 8 * (int)sizeof(pixel);
        uint32_t w[4] = { 0, 0, 0, 0 };
#pragma unroll
        for (int i = 0; i < VPT; i++) w[i / PER] |= v[i] << (BITS * (i % PER));
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < VPT; i++)
        if (i < n) p[i] = (pixel)v[i];
}

/* S: the source sample type; SEMI: chroma comes as U,V pairs in src[1] (a chroma row of the grid then stands for the U row and the V row) */
template<typename S, bool SEMI> __global__ __launch_bounds__(256) void k_ingest(IngestArgs a)
{
    int r = (int)(blockIdx.y * blockDim.y + threadIdx.y), plane = 0;
    if (r >= a.yRows)
    {
        r -= a.yRows; plane = 1;
        if (!SEMI && r >= a.cRows) { r -= a.cRows; plane = 2; }
        if (r >= a.cRows) return;
    }
    const int s1 = plane ? 1 : 0;
    const int w = a.W >> s1, h = a.H >> s1, mx = a.mx >> s1, my = a.my >> s1, sw = a.sw >> s1, sh = a.sh >> s1;
    const int rowLen = (int)(plane ? a.cstride : a.stride);
    pixel* row = a.dst + (plane == 0 ? 0 : a.ysz + (plane == 2 ? a.csz : 0)) + (long)r * rowLen;
    const int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) / sizeof(pixel));
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int c0 = j == 0 ? 0 : head + (j - 1) * VPT;
    const int n = min(j == 0 ? head : VPT, rowLen - c0);
    if (n <= 0) return;
    const int y = r - my, x0 = c0 - mx;
    uint32_t v[VPT], v2[VPT];
#pragma unroll
    for (int i = 0; i < VPT; i++) v[i] = v2[i] = 0;
    if (y < h + my)             /* (with an odd marginY the buffer has one chroma row below the padded area: zeros) */
    {
        const bool pairs = SEMI && plane;
        const uint8_t* base = a.src[plane] + (long)min(max(y, 0), sh - 1) * a.srcStride[plane];
        const S* s = reinterpret_cast<const S*>(base);
        if (n == VPT && x0 >= 0 && x0 + VPT <= sw)
        {
            if (pairs)
            {
                uint32_t uv[2 * VPT];
                load_run<S, 2 * VPT>(s + 2 * x0, uv);
#pragma unroll
                for (int i = 0; i < VPT; i++) { v[i] = uv[2 * i]; v2[i] = uv[2 * i + 1]; }
            }
            else load_run<S, VPT>(s + x0, v);
        }
        else
        {
#pragma unroll
            for (int i = 0; i < VPT; i++)
            {
                const int x = x0 + i;
                if (i >= n || x >= w + mx) continue;        /* (an odd marginX: one chroma column right of the padded area) */
                const int cx = min(max(x, 0), sw - 1);
                if (pairs) { v[i] = s[2 * cx]; v2[i] = s[2 * cx + 1]; }
                else v[i] = s[cx];
            }
        }
#pragma unroll
        for (int i = 0; i < VPT; i++)
        {
            const bool inside = x0 + i < w + mx;
            uint32_t t = xa_ingest_conv(v[i], a.bitDepth);
            if (plane == 0 && a.clip) t = xa_ingest_clip(t, a.lo, a.hi);
            v[i] = inside ? t : 0;
            if (pairs) v2[i] = inside ? xa_ingest_conv(v2[i], a.bitDepth) : 0;
        }
    }
    store_run(row + c0, v, n);
    if (SEMI && plane) store_run(row + a.csz + c0, v2, n);
}

}

extern "C" int x265amd_ingest_picture(void* stream, const x265amd_surface* d_src, int srcW, int srcH, x265amd_pixel* d_pic, int W, int H, int marginX, int marginY)
{
    static thread_local char why[160];
    const char* bad = xa_ingest_check(d_src, srcW, srcH, W, H, marginX, marginY);
    if (!bad && (!d_pic || ((uintptr_t)d_pic & (sizeof(pixel) - 1)))) bad = "null destination, or one at an odd address (alignment)";
    if (bad)
    {
        snprintf(why, sizeof(why), "x265amd_ingest_picture: %s", bad);
        return xa_fail(X265AMD_EINVAL, why);
    }
    if (xa_is_queue(stream)) return xa_fail(X265AMD_EINVAL, "x265amd_ingest_picture: stream: a hipStream_t (or NULL), not a device job queue");
    IngestArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < (d_src->layout ? 2 : 3); k++) { a.src[k] = (const uint8_t*)d_src->planes[k]; a.srcStride[k] = d_src->stride[k]; }
    a.dst = (pixel*)d_pic;
    a.stride = W + 2 * marginX; a.cstride = W / 2 + marginX;
    a.yRows = H + 2 * marginY; a.cRows = H / 2 + marginY;
    a.ysz = (long)a.yRows * a.stride; a.csz = (long)a.cRows * a.cstride;
    a.sw = srcW; a.sh = srcH; a.W = W; a.H = H; a.mx = marginX; a.my = marginY;
    a.bitDepth = d_src->bitDepth;
    a.clip = d_src->clipMin >= 0 || d_src->clipMax >= 0;
    a.lo = d_src->clipMin >= 0 ? (uint32_t)d_src->clipMin : 0; a.hi = d_src->clipMax >= 0 ? (uint32_t)d_src->clipMax : (1u << X265AMD_DEPTH) - 1;
    /* a block: 64 chunks of 4 rows; chunk 0 of a row is its head, so a row has at most 1 + ceil(stride / VPT) chunks */
    const int chunks = 1 + (int)((a.stride + VPT - 1) / VPT), rows = a.yRows + (d_src->layout ? 1 : 2) * a.cRows;
    const dim3 block(64, 4), grid((chunks + 63) / 64, (rows + 3) / 4);
    const hipStream_t st = (hipStream_t)stream;
    const bool wide = d_src->bitDepth > 8;
    if (!d_src->layout) { if (wide) hipLaunchKernelGGL((k_ingest<uint16_t, false>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_ingest<uint8_t, false>), grid, block, 0, st, a); }
    else { if (wide) hipLaunchKernelGGL((k_ingest<uint16_t, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_ingest<uint8_t, true>), grid, block, 0, st, a); }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}
