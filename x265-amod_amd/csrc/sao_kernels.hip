/* Sample adaptive offset over a whole picture (include/x265amd.h: x265amd_sao_stats, x265amd_sao_apply).
 *
 * Device restatement of SAO::calcSaoStatsCTU with saoCuStatsBO/E0..E3 (reference: source/encoder/sao.cpp:735-917, :1762-1925; with its
 * --sao-non-deblock skips and without EO_2 / EO_3 as compile-time forms), of SAO::calcSaoStatsCu_BeforeDblk (:919-1197, k_sao_stats_pre) and of SAO::generateLumaOffsets / generateChromaOffsets / applyPixelOffsets (sao.cpp:274-733), 4:2:0.
 * The reference walks CTUs in order and keeps the not-yet-offset samples it still needs in m_tmpU / m_tmpL; here the offset picture
 * is written to separate planes, so every sample is classified on the deblocked input directly and all samples are independent.
 * Statistics: one workgroup per (CTU, plane); every thread keeps the 4 x 5 edge-class sums and counts of its samples in registers
 * and the 32 band classes go through LDS atomics; one flush per thread at the end.  HBM-bound: the picture is read once (plus the
 * source picture for the statistics) and written once.
 */
#include "x265amd_dev.h"
#include "x265amd_host.h"
#include "sao_class.h"

struct SaoPlanes { const pixel* rec[3]; const pixel* fenc[3]; pixel* dst[3]; long stride, cstride; int width, height; int ctuRow0, ctuRows; int ctuCol0, ctuCols; int x0, x1; };      /* the CTU rows (and columns: statistics; luma sample columns x0 .. x1 - 1: offsets) of this launch */

XA_DEV int sao_class(int v, int a, int b) { return xa_sao_class(v, a, b); }           /* SAO::s_eoTable[sign + sign + 2]: sao_class.h, shared with the host model */

/* One workgroup per (CTU, plane).  The CTU's deblocked samples with a halo of one sample and its source samples are staged in LDS first -- sixteen samples per lane
 * and load, rows aligned to sixteen (a CTU starts at a multiple of 32 samples in its plane) -- so that the nine neighbours of a sample are LDS reads instead of nine
 * one-sample loads from the picture (the first form of this kernel: 95 us for a luma CTU, all of it load latency; this one: see profiles/).  Then a lane per sample as
 * before: the four edge classes' sums and counts in registers, the band class into a histogram per wavefront. */
constexpr int kSaoTileW = 64 + 32;              /* 16 samples of margin on either side keep every row's loads aligned; only one of each is read */
/* NON_DEBLOCK: calcSaoStatsCTU's skips under --sao-non-deblock (sao.cpp:812-896) -- BO 3 lines / 4 columns, EO_0 3 / 5, EO_1 4 / 4, EO_2 and EO_3 4 / 5 -- instead of 4 / 5
 * for every type.  EO01_ONLY: a B picture under --limit-sao (sao.cpp:861): EO_2 and EO_3 are not measured, their words come out zero.  Both are compile-time constants: the
 * <false, false> form is the kernel as it was. */
template<bool NON_DEBLOCK, bool EO01_ONLY>
__global__ __launch_bounds__(256) void k_sao_stats(SaoPlanes P, int32_t* count, int32_t* offsetOrg)
{
    constexpr int skipRfull = NON_DEBLOCK ? 4 : 5, skipBbo = NON_DEBLOCK ? 3 : 4, skipBe0 = NON_DEBLOCK ? 3 : 4;
    __shared__ int sCnt[5 * 32], sOrg[5 * 32];
    __shared__ int sBand[4][2][32];
    __shared__ __attribute__((aligned(16))) pixel sRec[66 * kSaoTileW];
    __shared__ __attribute__((aligned(16))) pixel sSrc[64 * 64];
    const int ctuW = (P.width + 63) >> 6;
    const int plane = blockIdx.y, ctu = (P.ctuRow0 + (int)blockIdx.x / P.ctuCols) * ctuW + P.ctuCol0 + (int)blockIdx.x % P.ctuCols;
    const int cx = ctu % ctuW, cy = ctu / ctuW;
    const int sh = plane ? 1 : 0, po = plane ? 2 : 0;
    const long st = plane ? P.cstride : P.stride;
    const int picW = P.width >> sh, picH = P.height >> sh, lpelx = (cx * 64) >> sh, tpely = (cy * 64) >> sh;
    const int rpelx = min(lpelx + (64 >> sh), picW), bpely = min(tpely + (64 >> sh), picH);
    const int cw = rpelx - lpelx, ch = bpely - tpely;
    const pixel* r0 = P.rec[plane] + (long)tpely * st + lpelx;
    const pixel* f0 = P.fenc[plane] + (long)tpely * st + lpelx;
    for (int i = threadIdx.x; i < 5 * 32; i += blockDim.x) { sCnt[i] = 0; sOrg[i] = 0; }
    (&sBand[0][0][0])[threadIdx.x] = 0;            /* 4 x 2 x 32 = the workgroup's 256 lanes */
    {
        /* rows tpely - 1 .. tpely + ch of the deblocked plane, samples lpelx - 16 .. lpelx + cw + 15 as far as they lie inside the picture (what lies outside is never
         * classified, and a caller's planes need no margins), and the CTU's source samples: chunks of sixteen samples.  Whether a chunk is sixteen-byte aligned in memory
         * depends on the plane's origin: the access type says "unaligned", the hardware takes either */
        constexpr int kChunk = 16;
        struct __attribute__((packed, aligned(1))) Chunk { pixel v[kChunk]; };
        const int chunksPerRow = (cw + 2 * kChunk) / kChunk, rows = ch + 2;
        for (int i = threadIdx.x; i < chunksPerRow * rows; i += blockDim.x)
        {
            const int y = i / chunksPerRow, c = i - y * chunksPerRow;
            const int gy = tpely + y - 1, gx0 = lpelx + (c - 1) * kChunk;
            if (gy < 0 || gy >= picH) continue;                     /* a row outside the picture is never looked at (aboveUnavail, endYedge) */
            const pixel* src = r0 + (long)(y - 1) * st + (c - 1) * kChunk;
            if (gx0 >= 0 && gx0 + kChunk <= picW) *reinterpret_cast<Chunk*>(&sRec[y * kSaoTileW + c * kChunk]) = *reinterpret_cast<const Chunk*>(src);
            else
                for (int k = 0; k < kChunk; k++) if (gx0 + k >= 0 && gx0 + k < picW) sRec[y * kSaoTileW + c * kChunk + k] = src[k];      /* nor is a column outside it (x0e, endXedge) */
        }
        const int srcChunks = cw / kChunk;          /* cw is a multiple of 4 (widths are multiples of 8); the tail below */
        for (int i = threadIdx.x; i < srcChunks * ch; i += blockDim.x)
        {
            const int y = i / srcChunks, c = i - y * srcChunks;
            *reinterpret_cast<Chunk*>(&sSrc[y * 64 + c * kChunk]) = *reinterpret_cast<const Chunk*>(f0 + (long)y * st + c * kChunk);
        }
        const int tail = cw - srcChunks * kChunk;
        for (int i = threadIdx.x; i < tail * ch; i += blockDim.x)
        {
            const int y = i / tail, x = srcChunks * kChunk + (i - y * tail);
            sSrc[y * 64 + x] = f0[(long)y * st + x];
        }
    }
    __syncthreads();
    const bool atRight = rpelx == picW, atBottom = bpely == picH;
    const int aboveUnavail = !tpely;
    const int endXfull = atRight ? cw : cw - skipRfull + po, endXedge = atRight ? cw - 1 : cw - 5 + po;
    const int endYfull = atBottom ? ch : ch - skipBbo + po, endYedge = atBottom ? ch - 1 : ch - 4 + po;
    const int x0e = !lpelx;
    int cnt[4][5], org[4][5];
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int c = 0; c < 5; c++) { cnt[t][c] = 0; org[t][c] = 0; }
    const int total = cw * ch, rounds = (total + (int)blockDim.x - 1) / (int)blockDim.x;
    constexpr int TS = kSaoTileW;
    for (int it = 0; it < rounds; it++)         /* uniform trip count: the band step uses wave-wide operations */
    {
        const int i = it * blockDim.x + threadIdx.x;
        const bool live = i < total;
        const int y = live ? i / cw : 0, x = live ? i - y * cw : cw;      /* x = cw lies outside every region */
        const pixel* r = &sRec[(y + 1) * TS + 16 + (live ? x : 0)];
        const int v = r[0], d = live ? (int)sSrc[y * 64 + x] - v : 0;
        /* band offset: a histogram per wavefront in LDS, a pair of LDS atomics per sample (lanes of a wavefront that hit the same band are serialised by the LDS, a
         * hundred cycles at worst; the loop over the wave's distinct bands this replaces cost six microseconds a round on noisy content) */
        if (x < endXfull && y < endYfull)
        {
            const int band = v >> (XA_DEPTH - 5);
            atomicAdd(&sBand[threadIdx.x >> 6][0][band], 1);
            atomicAdd(&sBand[threadIdx.x >> 6][1][band], d);
        }
        const bool inXe = x >= x0e && x < endXedge, inYe = y >= aboveUnavail && y < endYedge;
        int cls;
#define ACC(t, c) { cls = (c); _Pragma("unroll") for (int k = 0; k < 5; k++) if (cls == k) { cnt[t][k]++; org[t][k] += d; } }
        if (inXe && y < ch - skipBe0 + po) ACC(0, sao_class(v, r[-1], r[1]))
        if (x < endXfull && inYe) ACC(1, sao_class(v, r[-TS], r[TS]))
        if (!EO01_ONLY && inXe && inYe)
        {
            ACC(2, sao_class(v, r[-TS - 1], r[TS + 1]))
            ACC(3, sao_class(v, r[-TS + 1], r[TS - 1]))
        }
#undef ACC
    }
    /* the edge classes: summed over the wavefront first (256 lanes adding to the same twenty words one by one is twenty microseconds of LDS serialisation) */
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int c = 0; c < 5; c++)
        {
            if (EO01_ONLY && t >= 2) continue;
            const int cs = xa_wave_sum(cnt[t][c]), os = xa_wave_sum(org[t][c]);
            if ((threadIdx.x & 63) == 0 && cs) { atomicAdd(&sCnt[t * 32 + c], cs); atomicAdd(&sOrg[t * 32 + c], os); }
        }
    __syncthreads();
    if (threadIdx.x < 32)
    {
        sCnt[4 * 32 + threadIdx.x] = sBand[0][0][threadIdx.x] + sBand[1][0][threadIdx.x] + sBand[2][0][threadIdx.x] + sBand[3][0][threadIdx.x];
        sOrg[4 * 32 + threadIdx.x] = sBand[0][1][threadIdx.x] + sBand[1][1][threadIdx.x] + sBand[2][1][threadIdx.x] + sBand[3][1][threadIdx.x];
    }
    __syncthreads();
    const size_t base = ((size_t)ctu * 3 + plane) * 5 * 32;
    for (int i = threadIdx.x; i < 5 * 32; i += blockDim.x) { count[base + i] = sCnt[i]; offsetOrg[base + i] = sOrg[i]; }
}

/* SAO::calcSaoStatsCu_BeforeDblk (sao.cpp:919-1197) for --sao-non-deblock: the statistics of the right and bottom strips of every CTU -- the samples the deblocking of the
 * CTUs to the right and below still changes, which calcSaoStatsCTU leaves out -- on the reconstruction BEFORE any deblocking.  Per type the strips are the samples with
 * x >= startX or y >= startY (the skips of k_sao_stats<true, .> less the plane offset; collapsed at the picture's right / bottom edge as the reference collapses them); the
 * edge types never look into the CTU to the right or below (column cw - 1 / line ch - 1 are left out), nor beyond the picture's first column and line.
 * The region is a few hundred samples: a wavefront per (CTU, plane), four of them in a workgroup.  A lane takes every 64th sample of the right strip (columns sx .. cw - 1,
 * all lines) and then of the rest of the bottom strip (lines sy .. ch - 1, columns 0 .. sx - 1), sx / sy the smallest start of any type; it reads the sample and the
 * neighbours its types ask for straight from the picture (never a sample outside it: each read stands under the predicate of the type that needs it), keeps the edge
 * classes in registers and adds the band into its wavefront's histogram in LDS; one store of the 160 + 160 words at the end. */
constexpr int kSaoPreWaves = 4;
__global__ __launch_bounds__(64 * kSaoPreWaves) void k_sao_stats_pre(SaoPlanes P, int32_t* count, int32_t* offsetOrg)
{
    __shared__ int sCnt[kSaoPreWaves][5 * 32], sOrg[kSaoPreWaves][5 * 32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ctuW = (P.width + 63) >> 6;
    const int item = (int)blockIdx.x * kSaoPreWaves + wave, items = P.ctuCols * P.ctuRows * 3;
    const bool active = item < items;
    const int plane = active ? item % 3 : 0, local = active ? item / 3 : 0;
    const int ctu = (P.ctuRow0 + local / P.ctuCols) * ctuW + P.ctuCol0 + local % P.ctuCols;
    const int cx = ctu % ctuW, cy = ctu / ctuW;
    const int sh = plane ? 1 : 0, po = plane ? 2 : 0;
    const long st = plane ? P.cstride : P.stride;
    const int picW = P.width >> sh, picH = P.height >> sh, lpelx = (cx * 64) >> sh, tpely = (cy * 64) >> sh;
    const int rpelx = min(lpelx + (64 >> sh), picW), bpely = min(tpely + (64 >> sh), picH);
    const int cw = rpelx - lpelx, ch = bpely - tpely;
    const pixel* r0 = P.rec[plane] + (long)tpely * st + lpelx;
    const pixel* f0 = P.fenc[plane] + (long)tpely * st + lpelx;
    for (int i = lane; i < 5 * 32; i += 64) { sCnt[wave][i] = 0; sOrg[wave][i] = 0; }
    __syncthreads();
    const bool atRight = rpelx == picW, atBottom = bpely == picH;
    const int firstX = !lpelx, firstY = !tpely;
    /* startX / startY per type: [0] BO (skipB 3, skipR 4), [1] EO_0 (3, 5), [2] EO_1 (4, 4), [3] EO_2 and EO_3 (4, 5) */
    const int sxBO = atRight ? cw : cw - 4 + po, syBO = atBottom ? ch : ch - 3 + po;
    const int sxE0 = atRight ? cw - 1 : cw - 5 + po, syE0 = atBottom ? ch : ch - 3 + po;
    const int sxE1 = atRight ? cw : cw - 4 + po, syE1 = atBottom ? ch - 1 : ch - 4 + po;
    const int sxE2 = atRight ? cw - 1 : cw - 5 + po, syE2 = atBottom ? ch - 1 : ch - 4 + po;
    const int sx = sxE0, sy = syE1;             /* the smallest of each */
    int cnt[4][5], org[4][5];
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int c = 0; c < 5; c++) { cnt[t][c] = 0; org[t][c] = 0; }
    const int nRight = (cw - sx) * ch, total = active ? nRight + sx * (ch - sy) : 0;
    for (int i = lane; i < total; i += 64)
    {
        int x, y;
        if (i < nRight) { y = i / (cw - sx); x = sx + (i - y * (cw - sx)); }
        else { const int k = i - nRight; y = sy + k / sx; x = k - (y - sy) * sx; }
        const pixel* r = r0 + (long)y * st + x;
        const int v = r[0], d = (int)f0[(long)y * st + x] - v;
        if (x >= sxBO || y >= syBO)
        {
            const int band = v >> (XA_DEPTH - 5);
            atomicAdd(&sCnt[wave][4 * 32 + band], 1);
            atomicAdd(&sOrg[wave][4 * 32 + band], d);
        }
        const bool inX = x >= firstX && x < cw - 1, inY = y >= firstY && y < ch - 1;      /* "not refer right CTU", "not refer below CTU" */
        int cls;
#define ACC(t, c) { cls = (c); _Pragma("unroll") for (int k = 0; k < 5; k++) if (cls == k) { cnt[t][k]++; org[t][k] += d; } }
        if (inX && (x >= sxE0 || y >= syE0)) ACC(0, sao_class(v, r[-1], r[1]))
        if (inY && (x >= sxE1 || y >= syE1)) ACC(1, sao_class(v, r[-st], r[st]))
        if (inX && inY && (x >= sxE2 || y >= syE2))
        {
            ACC(2, sao_class(v, r[-st - 1], r[st + 1]))
            ACC(3, sao_class(v, r[-st + 1], r[st - 1]))
        }
#undef ACC
    }
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int c = 0; c < 5; c++)
        {
            const int cs = xa_wave_sum(cnt[t][c]), os = xa_wave_sum(org[t][c]);
            if (lane == 0) { sCnt[wave][t * 32 + c] = cs; sOrg[wave][t * 32 + c] = os; }
        }
    __syncthreads();
    if (!active) return;
    const size_t base = ((size_t)ctu * 3 + plane) * 5 * 32;
    for (int i = lane; i < 5 * 32; i += 64) { count[base + i] = sCnt[wave][i]; offsetOrg[base + i] = sOrg[wave][i]; }
}

__global__ __launch_bounds__(256) void k_sao_apply(SaoPlanes P, const x265amd_sao_ctu* params)
{
    const int plane = blockIdx.z;
    const int sh = plane ? 1 : 0;
    const long st = plane ? P.cstride : P.stride;
    const int picW = P.width >> sh, picH = P.height >> sh;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = ((P.ctuRow0 * 64) >> sh) + blockIdx.y;
    if (x >= picW || y >= picH || y >= (((P.ctuRow0 + P.ctuRows) * 64) >> sh) || x < (P.x0 >> sh) || x >= (P.x1 >> sh)) return;
    const int ctuW = (P.width + 63) >> 6;
    const x265amd_sao_ctu p = params[((y << sh) >> 6) * ctuW + ((x << sh) >> 6)];
    const int type = p.type[plane ? 1 : 0];
    const pixel* s = P.rec[plane] + (long)y * st + x;
    const int v = s[0];
    int out = v;
    if (type == 4)
    {
        const int k = ((v >> (XA_DEPTH - 5)) - p.band_pos[plane]) & 31;
        if (k < 4) out = v + p.offset[plane][k];
    }
    else if (type >= 0)
    {
        const int dx = type == 1 ? 0 : (type == 3 ? 1 : -1), dy = type == 0 ? 0 : -1;
        const bool edge = (dx && (x == 0 || x == picW - 1)) || (dy && (y == 0 || y == picH - 1));
        if (!edge)
        {
            const int cls = sao_class(v, s[dy * st + dx], s[-dy * st - dx]);
            if (cls) out = v + p.offset[plane][cls - 1];
        }
    }
    P.dst[plane][(long)y * st + x] = xa_clip_pixel(out);
}

static int sao_fill(SaoPlanes& P, const uint64_t* rec, const uint64_t* fenc, const uint64_t* dst, intptr_t stride, intptr_t cstride, int width, int height)
{
    for (int c = 0; c < 3; c++)
    {
        P.rec[c] = (const pixel*)(uintptr_t)rec[c];
        P.fenc[c] = fenc ? (const pixel*)(uintptr_t)fenc[c] : nullptr;
        P.dst[c] = dst ? (pixel*)(uintptr_t)dst[c] : nullptr;
    }
    P.stride = (long)stride; P.cstride = (long)cstride; P.width = width; P.height = height; P.ctuRow0 = 0; P.ctuRows = (height + 63) >> 6;
    P.ctuCol0 = 0; P.ctuCols = (width + 63) >> 6; P.x0 = 0; P.x1 = width;
    return 0;
}

extern "C" int x265amd_sao_stats(void* stream, const uint64_t rec_planes[3], const uint64_t fenc_planes[3], intptr_t stride, intptr_t cstride,
                                 int width, int height, int32_t* d_count, int32_t* d_offset_org)
{
    return x265amd_sao_stats_rows(stream, rec_planes, fenc_planes, stride, cstride, width, height, d_count, d_offset_org, 0, (height + 63) >> 6);
}

/* the statistics of CTU rows ctu_row_begin .. ctu_row_end - 1 (same arrays, indexed by the CTU's address in the picture).  A CTU's statistics leave out
 * the samples the deblocking of the CTUs to its right and below still changes (sao.cpp:760-776), so a row can be measured as soon as it is deblocked itself. */
extern "C" int x265amd_sao_stats_rows(void* stream, const uint64_t rec_planes[3], const uint64_t fenc_planes[3], intptr_t stride, intptr_t cstride,
                                      int width, int height, int32_t* d_count, int32_t* d_offset_org, int ctu_row_begin, int ctu_row_end)
{
    return x265amd_sao_stats_rows_cols(stream, rec_planes, fenc_planes, stride, cstride, width, height, d_count, d_offset_org, ctu_row_begin, ctu_row_end, 0, (width + 63) >> 6);
}

/* ... of the CTU columns ctu_col_begin .. ctu_col_end - 1 of those rows (a CTU's statistics read nothing right of its own columns but what the deblocking of the
 * CTU to its right leaves alone) */
extern "C" int x265amd_sao_stats_rows_cols(void* stream, const uint64_t rec_planes[3], const uint64_t fenc_planes[3], intptr_t stride, intptr_t cstride,
                                           int width, int height, int32_t* d_count, int32_t* d_offset_org, int ctu_row_begin, int ctu_row_end, int ctu_col_begin, int ctu_col_end)
{
    return x265amd_sao_stats_opt_rows_cols(stream, rec_planes, fenc_planes, stride, cstride, width, height, d_count, d_offset_org, 0, ctu_row_begin, ctu_row_end, ctu_col_begin, ctu_col_end);
}

/* the forms of the options: flags = X265AMD_SAO_NON_DEBLOCK | X265AMD_SAO_EO01_ONLY (k_sao_stats<.,.>); 0 is the calls above */
extern "C" int x265amd_sao_stats_opt(void* stream, const uint64_t rec_planes[3], const uint64_t fenc_planes[3], intptr_t stride, intptr_t cstride,
                                     int width, int height, int32_t* d_count, int32_t* d_offset_org, int flags)
{
    return x265amd_sao_stats_opt_rows_cols(stream, rec_planes, fenc_planes, stride, cstride, width, height, d_count, d_offset_org, flags, 0, (height + 63) >> 6, 0, (width + 63) >> 6);
}
extern "C" int x265amd_sao_stats_opt_rows(void* stream, const uint64_t rec_planes[3], const uint64_t fenc_planes[3], intptr_t stride, intptr_t cstride,
                                          int width, int height, int32_t* d_count, int32_t* d_offset_org, int flags, int ctu_row_begin, int ctu_row_end)
{
    return x265amd_sao_stats_opt_rows_cols(stream, rec_planes, fenc_planes, stride, cstride, width, height, d_count, d_offset_org, flags, ctu_row_begin, ctu_row_end, 0, (width + 63) >> 6);
}
extern "C" int x265amd_sao_stats_opt_rows_cols(void* stream, const uint64_t rec_planes[3], const uint64_t fenc_planes[3], intptr_t stride, intptr_t cstride,
                                               int width, int height, int32_t* d_count, int32_t* d_offset_org, int flags, int ctu_row_begin, int ctu_row_end, int ctu_col_begin, int ctu_col_end)
{
    if (flags & ~(X265AMD_SAO_NON_DEBLOCK | X265AMD_SAO_EO01_ONLY)) return xa_fail(X265AMD_EINVAL, "x265amd_sao_stats: flags");
    if (ctu_col_begin < 0 || ctu_col_begin >= ctu_col_end || ctu_col_end > ((width + 63) >> 6)) return xa_fail(X265AMD_EINVAL, "x265amd_sao_stats: column range");
    if (!rec_planes || !fenc_planes || !d_count || !d_offset_org || width <= 0 || height <= 0 || (width & 7) || (height & 7) || ctu_row_begin < 0 || ctu_row_begin >= ctu_row_end ||
        ctu_row_end > ((height + 63) >> 6))
        return xa_fail(X265AMD_EINVAL, "x265amd_sao_stats: bad arguments");
    SaoPlanes P;
    sao_fill(P, rec_planes, fenc_planes, nullptr, stride, cstride, width, height);
    P.ctuRow0 = ctu_row_begin; P.ctuRows = ctu_row_end - ctu_row_begin; P.ctuCol0 = ctu_col_begin; P.ctuCols = ctu_col_end - ctu_col_begin;
    const int nctu = P.ctuCols * P.ctuRows;
    const dim3 grid(nctu, 3), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (flags)
    {
    case 0: hipLaunchKernelGGL((k_sao_stats<false, false>), grid, block, 0, st, P, d_count, d_offset_org); break;
    case X265AMD_SAO_NON_DEBLOCK: hipLaunchKernelGGL((k_sao_stats<true, false>), grid, block, 0, st, P, d_count, d_offset_org); break;
    case X265AMD_SAO_EO01_ONLY: hipLaunchKernelGGL((k_sao_stats<false, true>), grid, block, 0, st, P, d_count, d_offset_org); break;
    default: hipLaunchKernelGGL((k_sao_stats<true, true>), grid, block, 0, st, P, d_count, d_offset_org); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}

/* the pre-deblock statistics of --sao-non-deblock (k_sao_stats_pre): rec_planes = the reconstruction before any deblocking; the same layout as d_count / d_offset_org */
extern "C" int x265amd_sao_stats_pre(void* stream, const uint64_t rec_planes[3], const uint64_t fenc_planes[3], intptr_t stride, intptr_t cstride,
                                     int width, int height, int32_t* d_pre_count, int32_t* d_pre_offset_org)
{
    return x265amd_sao_stats_pre_rows(stream, rec_planes, fenc_planes, stride, cstride, width, height, d_pre_count, d_pre_offset_org, 0, (height + 63) >> 6);
}
/* ... of CTU rows ctu_row_begin .. ctu_row_end - 1: they read the rows themselves and the last line of the row above, none of it deblocked yet */
extern "C" int x265amd_sao_stats_pre_rows(void* stream, const uint64_t rec_planes[3], const uint64_t fenc_planes[3], intptr_t stride, intptr_t cstride,
                                          int width, int height, int32_t* d_pre_count, int32_t* d_pre_offset_org, int ctu_row_begin, int ctu_row_end)
{
    if (!rec_planes || !fenc_planes || !d_pre_count || !d_pre_offset_org || width <= 0 || height <= 0 || (width & 7) || (height & 7) || ctu_row_begin < 0 || ctu_row_begin >= ctu_row_end ||
        ctu_row_end > ((height + 63) >> 6))
        return xa_fail(X265AMD_EINVAL, "x265amd_sao_stats_pre: bad arguments");
    SaoPlanes P;
    sao_fill(P, rec_planes, fenc_planes, nullptr, stride, cstride, width, height);
    P.ctuRow0 = ctu_row_begin; P.ctuRows = ctu_row_end - ctu_row_begin;
    const int items = P.ctuCols * P.ctuRows * 3;
    hipLaunchKernelGGL(k_sao_stats_pre, dim3((items + kSaoPreWaves - 1) / kSaoPreWaves), dim3(64 * kSaoPreWaves), 0, (hipStream_t)stream, P, d_pre_count, d_pre_offset_org);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}

extern "C" int x265amd_sao_apply(void* stream, const uint64_t src_planes[3], const uint64_t dst_planes[3], intptr_t stride, intptr_t cstride,
                                 int width, int height, const x265amd_sao_ctu* d_params)
{
    return x265amd_sao_apply_rows(stream, src_planes, dst_planes, stride, cstride, width, height, d_params, 0, (height + 63) >> 6);
}

/* the offset samples of CTU rows ctu_row_begin .. ctu_row_end - 1; the rows' samples are classified on src, whose row below must be deblocked already */
extern "C" int x265amd_sao_apply_rows(void* stream, const uint64_t src_planes[3], const uint64_t dst_planes[3], intptr_t stride, intptr_t cstride,
                                      int width, int height, const x265amd_sao_ctu* d_params, int ctu_row_begin, int ctu_row_end)
{
    return x265amd_sao_apply_rows_cols(stream, src_planes, dst_planes, stride, cstride, width, height, d_params, ctu_row_begin, ctu_row_end, 0, width);
}

/* ... restricted to the luma sample columns x_begin .. x_end - 1 (even; chroma: half): a sample is classified on itself and its two neighbours along the class
 * direction, so the deblocked input must be final one sample beyond either end */
extern "C" int x265amd_sao_apply_rows_cols(void* stream, const uint64_t src_planes[3], const uint64_t dst_planes[3], intptr_t stride, intptr_t cstride,
                                           int width, int height, const x265amd_sao_ctu* d_params, int ctu_row_begin, int ctu_row_end, int x_begin, int x_end)
{
    if (x_begin < 0 || x_begin >= x_end || x_end > width || (x_begin & 1) || (x_end & 1)) return xa_fail(X265AMD_EINVAL, "x265amd_sao_apply: column range");
    if (!src_planes || !dst_planes || !d_params || width <= 0 || height <= 0 || (width & 7) || (height & 7) || ctu_row_begin < 0 || ctu_row_begin >= ctu_row_end ||
        ctu_row_end > ((height + 63) >> 6))
        return xa_fail(X265AMD_EINVAL, "x265amd_sao_apply: bad arguments");
    SaoPlanes P;
    sao_fill(P, src_planes, nullptr, dst_planes, stride, cstride, width, height);
    P.ctuRow0 = ctu_row_begin; P.ctuRows = ctu_row_end - ctu_row_begin; P.x0 = x_begin; P.x1 = x_end;
    const int lines = (height < ctu_row_end * 64 ? height : ctu_row_end * 64) - ctu_row_begin * 64;
    hipLaunchKernelGGL(k_sao_apply, dim3((width + 255) / 256, lines, 3), dim3(256), 0, (hipStream_t)stream, P, d_params);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}
