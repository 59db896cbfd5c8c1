/* Quality metrics as picture-wide reductions (include/x265amd.h: x265amd_picture_ssd, x265amd_picture_ssim, x265amd_luma_level; the arithmetic and the geometry that
 * host and device share: quality_dev.h; the host models: host/quality_model.cpp).
 *
 * The reference measures these on the host, CTU row by CTU row, inside its frame filter (FrameFilter::processPostRow, source/encoder/framefilter.cpp:654-723;
 * PicYuv::copyFromPicture, source/common/picyuv.cpp:426-439).  Here the source and the reconstructed picture are both in device memory already, so each measurement is one
 * pass over the planes and a few words come back.  All three are HBM-bound: every sample is read once (the SSIM pass reads a block row twice, once per window row
 * it belongs to; the second read comes from L2).
 *
 *   k_picture_ssd    grid (chunks of kRedRows rows, 3 planes).  A lane takes runs of 4 samples along a row, one vector load per plane where the row is aligned; plain
 *                    integer arithmetic; a 32-bit partial per lane and row -- at most 64 samples (the entry point refuses rows beyond 16384 samples; 1023^2 * 4105
 *                    would pass 2^32) -- widened to 64 bits per lane across the chunk's rows, one 64-bit wave sum, the four waves' sums through LDS, then ONE 64-bit vector atomic per workgroup.
 *   k_luma_level     the same walk over one plane: sum and maximum.
 *   k_ssim_rows      grid (tiles of kSsimTile windows, window rows).  A lane forms the four sums of one 4x4 block in both block rows of the window row into LDS; one lane
 *                    per window adds four blocks' sums and forms the term (xa_ssim_end_1: every float operation rounded on its own, no fused multiply-add); one lane per group of four windows adds the
 *                    group's terms left to right (ssim_end_4) and stores the group sum.  kSsimTile is a multiple of four, so groups never straddle tiles.
 *   k_ssim_bands     grid (bands).  The band's group sums, staged through LDS in chunks, are added by ONE lane in the reference's order: the only serial part, about 7 500
 *                    additions for a band of a 4320p picture.  Float addition does not associate and the result has to be the reference's bits.
 * No atomics on floats, nothing depends on the order in which workgroups arrive. */
#include "x265amd_dev.h"
#include "x265amd_host.h"
#include "quality_dev.h"

constexpr int kRedRows = 8;             /* rows per workgroup of the two reductions */
constexpr int kRedMaxWidth = 16384;     /* 64 samples per lane and row: the bound of the 32-bit partials (1023^2 * 4105 would pass 2^32) */
constexpr int kSsimTile = 252;          /* windows per workgroup: 63 groups of four, 253 blocks per block row */
constexpr int kSsimChain = 2048;        /* group sums staged per step of the band's chain */

struct QualityPlanes { const pixel* src[3]; const pixel* rec[3]; };

/* four samples from an aligned address in one load */
XA_DEV void xa_load4(const pixel* p, int v[4])
{
#if XA_DEPTH > 8
    const uint2 w = *(const uint2*)p;
    v[0] = w.x & 0xffff; v[1] = w.x >> 16; v[2] = w.y & 0xffff; v[3] = w.y >> 16;
#else
    const uint32_t w = *(const uint32_t*)p;
    v[0] = w & 0xff; v[1] = (w >> 8) & 0xff; v[2] = (w >> 16) & 0xff; v[3] = w >> 24;
#endif
}
XA_DEV bool xa_aligned4(const pixel* p) { return ((uintptr_t)p & (4 * sizeof(pixel) - 1)) == 0; }

__global__ __launch_bounds__(256) void k_picture_ssd(QualityPlanes P, long stride, long cstride, int orgWidth, int height, unsigned long long* ssd)
{
    const int tid = threadIdx.x, plane = blockIdx.y;
    const int w = plane ? orgWidth >> 1 : orgWidth, h = plane ? height >> 1 : height;
    const long st = plane ? cstride : stride;
    const int row0 = blockIdx.x * kRedRows, row1 = min(row0 + kRedRows, h);
    if (row0 >= h) return;              /* (the whole workgroup: the grid's chunk count is the luma plane's) */
    uint64_t acc = 0;
    for (int r = row0; r < row1; r++)
    {
        const pixel* a = P.src[plane] + (long)r * st; const pixel* b = P.rec[plane] + (long)r * st;
        const bool vec = xa_aligned4(a) && xa_aligned4(b);
        uint32_t part = 0;
        for (int x = tid * 4; x < w; x += 256 * 4)
        {
            if (vec && x + 4 <= w)
            {
                int va[4], vb[4];
                xa_load4(a + x, va); xa_load4(b + x, vb);
                for (int i = 0; i < 4; i++) { const int d = va[i] - vb[i]; part += (uint32_t)(d * d); }
            }
            else
                for (int i = 0; i < 4 && x + i < w; i++) { const int d = (int)a[x + i] - (int)b[x + i]; part += (uint32_t)(d * d); }
        }
        acc += part;            /* (per lane: no cross-lane step between rows, so the next row's loads are in flight behind this row's arithmetic) */
    }
    /* one atomic per workgroup: every workgroup of a plane adds to ONE word, and the pass's time went with the number of atomics, not with the bytes */
    __shared__ uint64_t waveSum[4];
    acc = xa_wave_sum(acc);
    if ((tid & 63) == 0) waveSum[tid >> 6] = acc;
    __syncthreads();
    const uint64_t all = waveSum[0] + waveSum[1] + waveSum[2] + waveSum[3];
    if (tid == 0 && all) atomicAdd(&ssd[plane], (unsigned long long)all);
}

__global__ __launch_bounds__(256) void k_luma_level(const pixel* luma, long stride, int orgWidth, int orgHeight, x265amd_luma_level_record* level)
{
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * kRedRows, row1 = min(row0 + kRedRows, orgHeight);
    uint64_t acc = 0;
    int top = 0;
    for (int r = row0; r < row1; r++)
    {
        const pixel* a = luma + (long)r * stride;
        const bool vec = xa_aligned4(a);
        uint32_t part = 0;
        for (int x = tid * 4; x < orgWidth; x += 256 * 4)
        {
            if (vec && x + 4 <= orgWidth)
            {
                int va[4];
                xa_load4(a + x, va);
                for (int i = 0; i < 4; i++) { part += (uint32_t)va[i]; top = max(top, va[i]); }
            }
            else
                for (int i = 0; i < 4 && x + i < orgWidth; i++) { const int v = a[x + i]; part += (uint32_t)v; top = max(top, v); }
        }
        acc += part;
    }
    __shared__ uint64_t waveSum[4];
    __shared__ int waveTop[4];
    acc = xa_wave_sum(acc);
    for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
    if ((tid & 63) == 0) { waveSum[tid >> 6] = acc; waveTop[tid >> 6] = top; }
    __syncthreads();
    if (tid == 0)
    {
        const uint64_t all = waveSum[0] + waveSum[1] + waveSum[2] + waveSum[3];
        const int allTop = max(max(waveTop[0], waveTop[1]), max(waveTop[2], waveTop[3]));
        if (all) atomicAdd((unsigned long long*)&level->sum, (unsigned long long)all);
        if (allTop) atomicMax(&level->max, (uint32_t)allTop);
    }
}

__global__ __launch_bounds__(256) void k_ssim_rows(const pixel* src, const pixel* rec, long stride, int width, int height, float* groupSums, int32_t* blockSums)
{
    __shared__ int sums[2][kSsimTile + 1][4];
    __shared__ float terms[kSsimTile];
    const int tid = threadIdx.x, wy = blockIdx.y, wb = xa_ssim_wb(width), first = blockIdx.x * kSsimTile;
    const int bx = first + tid;
    if (tid <= kSsimTile && bx < wb)
        for (int k = 0; k < 2; k++)
        {
            /* ssim_4x4x2_core's sums of one block: pix1 is the reconstruction, pix2 the source (framefilter.cpp:694-709) */
            const long at = (long)(2 + 4 * (wy + k)) * stride + 2 + 4 * bx;
            uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
            for (int y = 0; y < 4; y++)
                for (int x = 0; x < 4; x++)
                {
                    const uint32_t a = rec[at + y * stride + x], b = src[at + y * stride + x];
                    s1 += a; s2 += b; ss += a * a; ss += b * b; s12 += a * b;
                }
            sums[k][tid][0] = (int)s1; sums[k][tid][1] = (int)s2; sums[k][tid][2] = (int)ss; sums[k][tid][3] = (int)s12;
            if (blockSums && (k == 0 || wy == xa_ssim_hb(height) - 2))
            {
                int32_t* out = blockSums + ((size_t)(wy + k) * wb + bx) * 4;
                out[0] = (int)s1; out[1] = (int)s2; out[2] = (int)ss; out[3] = (int)s12;
            }
        }
    __syncthreads();
    if (tid < kSsimTile && first + tid < wb - 1)
    {
        int s[4];
        for (int i = 0; i < 4; i++) s[i] = sums[1][tid][i] + sums[1][tid + 1][i] + sums[0][tid][i] + sums[0][tid + 1][i];
        terms[tid] = xa_ssim_end_1(s[0], s[1], s[2], s[3], XA_DEPTH);
    }
    __syncthreads();
    const int g0 = first + XA_SSIM_GROUP * tid;
    if (tid < kSsimTile / XA_SSIM_GROUP && g0 < wb - 1)
        groupSums[(size_t)wy * xa_ssim_groups(width) + blockIdx.x * (kSsimTile / XA_SSIM_GROUP) + tid] = xa_ssim_group_sum(&terms[XA_SSIM_GROUP * tid], min(XA_SSIM_GROUP, wb - 1 - g0));
}

__global__ __launch_bounds__(256) void k_ssim_bands(const float* groupSums, int width, int height, x265amd_ssim_band* bands)
{
    __shared__ float staged[kSsimChain];
    const int tid = threadIdx.x, band = blockIdx.x;
    int firstRow, rows;
    xa_ssim_band(height, band, &firstRow, &rows);
    const int groups = xa_ssim_groups(width);
    const long total = (long)rows * groups;
    const float* from = groupSums + (size_t)firstRow * groups;
    float sum = 0.0f;           /* (lane 0's: calculateSSIM's running float) */
    for (long base = 0; base < total; base += kSsimChain)
    {
        const int n = (int)min((long)kSsimChain, total - base);
        for (int i = tid; i < n; i += 256) staged[i] = from[base + i];
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < n; i++) sum += staged[i];
        __syncthreads();
    }
    if (tid == 0)
    {
        bands[band].sum_bits = __float_as_uint(sum);
        bands[band].cnt = (uint32_t)rows * (uint32_t)(xa_ssim_wb(width) - 1);
    }
}

static bool codedSizeOk(int width, int height, int org_width, int org_height)
{
    return width >= 16 && height >= 16 && !(width & 7) && !(height & 7) && org_width > 0 && org_height > 0 && org_width <= width && org_height <= height && width <= kRedMaxWidth;
}

extern "C" int x265amd_picture_ssd(void* stream, const uint64_t src[3], const uint64_t rec[3], intptr_t stride, intptr_t cstride, int width, int height, int org_width,
                                   int org_height, uint64_t* d_ssd)
{
    if (!src || !rec || !d_ssd || !codedSizeOk(width, height, org_width, org_height) || stride < width || cstride < width / 2)
        return xa_fail(X265AMD_EINVAL, "x265amd_picture_ssd: bad arguments");
    QualityPlanes P;
    for (int k = 0; k < 3; k++)
    {
        if (!src[k] || !rec[k]) return xa_fail(X265AMD_EINVAL, "x265amd_picture_ssd: bad arguments");
        P.src[k] = (const pixel*)(uintptr_t)src[k]; P.rec[k] = (const pixel*)(uintptr_t)rec[k];
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_ssd, 0, 3 * sizeof(uint64_t), st) != hipSuccess) return xa_fail(X265AMD_EHIP, "x265amd_picture_ssd: memset");
    hipLaunchKernelGGL(k_picture_ssd, dim3((height + kRedRows - 1) / kRedRows, 3), dim3(256), 0, st, P, (long)stride, (long)cstride, org_width, height, (unsigned long long*)d_ssd);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}

extern "C" int x265amd_luma_level(void* stream, uint64_t luma, intptr_t stride, int org_width, int org_height, x265amd_luma_level_record* d_level)
{
    if (!luma || !d_level || org_width <= 0 || org_height <= 0 || org_width > kRedMaxWidth || stride < org_width) return xa_fail(X265AMD_EINVAL, "x265amd_luma_level: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_level, 0, sizeof(*d_level), st) != hipSuccess) return xa_fail(X265AMD_EHIP, "x265amd_luma_level: memset");
    hipLaunchKernelGGL(k_luma_level, dim3((org_height + kRedRows - 1) / kRedRows), dim3(256), 0, st, (const pixel*)(uintptr_t)luma, (long)stride, org_width, org_height, d_level);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}

extern "C" int x265amd_picture_ssim(void* stream, uint64_t src_luma, uint64_t rec_luma, intptr_t stride, int width, int height, x265amd_ssim_band* d_bands, void* d_work,
                                    uint64_t block_sums)
{
    if (!src_luma || !rec_luma || !d_bands || !d_work || !codedSizeOk(width, height, width, height) || stride < width)
        return xa_fail(X265AMD_EINVAL, "x265amd_picture_ssim: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int windows = xa_ssim_wb(width) - 1, windowRows = xa_ssim_hb(height) - 1;
    hipLaunchKernelGGL(k_ssim_rows, dim3((windows + kSsimTile - 1) / kSsimTile, windowRows), dim3(256), 0, st, (const pixel*)(uintptr_t)src_luma, (const pixel*)(uintptr_t)rec_luma,
                       (long)stride, width, height, (float*)d_work, (int32_t*)(uintptr_t)block_sums);
    hipLaunchKernelGGL(k_ssim_bands, dim3(xa_ssim_bands(height)), dim3(256), 0, st, (const float*)d_work, width, height, d_bands);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}
