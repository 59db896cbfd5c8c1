/* The edge-based recursion skip (--rskip 2), the host half (include/x265amd.h: x265amd_rskip_edge_model, x265amd_rskip_edge_skip).
 * x265amd_rskip_edge_model is the plane and the block counts the device pass x265amd_rskip_edge_counts (csrc/lowres_kernels.hip) has to give: computeEdge
 * (reference: source/encoder/slicetype.cpp:98-157) on the source picture without an angle plane and with white pixel 1, as FrameEncoder::compressFrame calls it
 * (source/encoder/frameencoder.cpp:474-484).  x265amd_rskip_edge_skip is Analysis::complexityCheckCU's edge branch (source/encoder/analysis.cpp:3561-3577) in the
 * reference's operand types and order. */
#include "x265amd.h"
#include "../csrc/aq_edge_dev.h"
#include <string.h>

extern "C" int x265amd_rskip_edge_model(const x265amd_pixel* luma, intptr_t stride, int width, int height, uint8_t* plane, uint32_t* counts)
{
    if (!luma || width <= 0 || height <= 0 || stride < width) return X265AMD_EINVAL;
    const int bw = (width + 31) / 32, bh = (height + 31) / 32;
    if (plane) memset(plane, 0, (size_t)width * height);                /* Frame::create zeroes the plane; the outermost row and column are never written */
    if (counts) memset(counts, 0, sizeof(uint32_t) * bw * bh);
    const int white = (1 << X265AMD_DEPTH) - 1;                         /* EDGE_THRESHOLD: 255.0 / 1023.0 */
    for (int y = 1; y < height - 1; y++)
    {
        const x265amd_pixel* r0 = luma + (intptr_t)(y - 1) * stride; const x265amd_pixel* r1 = r0 + stride; const x265amd_pixel* r2 = r1 + stride;
        for (int x = 1; x < width - 1; x++)
        {
            const int gh = -3 * r0[x - 1] + 3 * r0[x + 1] - 10 * r1[x - 1] + 10 * r1[x + 1] - 3 * r2[x - 1] + 3 * r2[x + 1];
            const int gv = -3 * r0[x - 1] - 10 * r0[x] - 3 * r0[x + 1] + 3 * r2[x - 1] + 10 * r2[x] + 3 * r2[x + 1];
            if (!xa_edge_is_edge(gv, gh, white)) continue;
            if (plane) plane[(size_t)y * width + x] = 1;
            if (counts) counts[(size_t)(y >> 5) * bw + (x >> 5)]++;
        }
    }
    return X265AMD_OK;
}

extern "C" int x265amd_rskip_edge_skip(uint32_t count, int cu_size, float threshold)
{
    /* primitives.cu[].var over a plane of 0 / 1: the sum and the sum of squares are both the number of ones */
    const uint32_t sum = count, ss = count;
    const uint32_t pixelCount = (uint32_t)cu_size * (uint32_t)cu_size;          /* 1 << (log2CUSize * 2) */
    const double cuEdgeVariance = (ss - ((double)sum * sum / pixelCount)) / pixelCount;
    return cuEdgeVariance > (double)threshold ? 0 : 1;
}
