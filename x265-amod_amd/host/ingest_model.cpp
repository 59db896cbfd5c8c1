/* Picture ingest, the host model (include/x265amd.h: x265amd_ingest_model): what x265amd_ingest_picture has to leave in the flat picture buffer, computed on host memory
 * the way the reference goes about it -- pass after pass, as PicYuv::copyFromPicture (source/common/picyuv.cpp:261-515) and extendPicBorder (source/common/pixel.cpp:
 * 1044-1058) do:
 *   1. the planes are copied into the picture area sample by sample, converted (:298-396; the arithmetic is csrc/ingest_dev.h's, the one thing shared with the kernel);
 *      semi-planar chroma is taken apart here, U first;
 *   2. the luma clip (:413-424);
 *   3. the right pad from the last column, then the bottom pad from the last padded row (:479-514), up to the coded size W x H;
 *   4. the margins: left and right of every row, then whole rows above and below (extendPicBorder).
 * What the buffer holds outside the padded area (odd margins only) is zero.  Host C++, loads without a GPU. */
#include "x265amd.h"
#include "../csrc/ingest_dev.h"
#include <stdio.h>
#include <string.h>

int xa_fail(int code, const char* msg);

extern "C" int x265amd_ingest_model(const x265amd_surface* src, int srcW, int srcH, x265amd_pixel* pic, int W, int H, int marginX, int marginY)
{
    static thread_local char why[160];
    const char* bad = xa_ingest_check(src, srcW, srcH, W, H, marginX, marginY);
    if (!bad && (!pic || ((uintptr_t)pic & (sizeof(x265amd_pixel) - 1)))) bad = "null destination, or one at an odd address (alignment)";
    if (bad)
    {
        snprintf(why, sizeof(why), "x265amd_ingest_model: %s", bad);
        return xa_fail(X265AMD_EINVAL, why);
    }
    const intptr_t stride = W + 2 * marginX, cstride = W / 2 + marginX;
    const size_t ysz = (size_t)(H + 2 * marginY) * stride, csz = (size_t)(H / 2 + marginY) * cstride;
    memset(pic, 0, (ysz + 2 * csz) * sizeof(x265amd_pixel));
    const int b = src->bitDepth;
    for (int k = 0; k < 3; k++)
    {
        const int w = k ? W / 2 : W, h = k ? H / 2 : H, mx = k ? marginX / 2 : marginX, my = k ? marginY / 2 : marginY, sw = k ? srcW / 2 : srcW, sh = k ? srcH / 2 : srcH;
        const intptr_t st = k ? cstride : stride;
        x265amd_pixel* org = pic + (k == 0 ? 0 : ysz + (k == 2 ? csz : 0)) + (intptr_t)my * st + mx;
        /* where sample x of row y of this plane lies in the caller's memory: a plane of its own, or every second sample of the pair plane */
        const uint8_t* plane = (const uint8_t*)src->planes[src->layout && k ? 1 : k];
        const intptr_t sst = src->stride[src->layout && k ? 1 : k];
        const int step = src->layout && k ? 2 : 1, first = src->layout && k == 2 ? 1 : 0;
        for (int y = 0; y < sh; y++)
        {
            x265amd_pixel* row = org + (intptr_t)y * st;
            for (int x = 0; x < sw; x++)
            {
                const uint32_t v = b > 8 ? ((const uint16_t*)(plane + (intptr_t)y * sst))[step * x + first] : (plane + (intptr_t)y * sst)[step * x + first];
                row[x] = (x265amd_pixel)xa_ingest_conv(v, b);
            }
        }
        if (k == 0 && (src->clipMin >= 0 || src->clipMax >= 0))
        {
            const uint32_t lo = src->clipMin >= 0 ? (uint32_t)src->clipMin : 0, hi = src->clipMax >= 0 ? (uint32_t)src->clipMax : (1u << X265AMD_DEPTH) - 1;
            for (int y = 0; y < sh; y++)
                for (int x = 0; x < sw; x++) org[(intptr_t)y * st + x] = (x265amd_pixel)xa_ingest_clip(org[(intptr_t)y * st + x], lo, hi);
        }
        for (int y = 0; y < sh; y++)
            for (int x = sw; x < w; x++) org[(intptr_t)y * st + x] = org[(intptr_t)y * st + sw - 1];
        for (int y = sh; y < h; y++) memcpy(org + (intptr_t)y * st, org + (intptr_t)(sh - 1) * st, (size_t)w * sizeof(x265amd_pixel));
        for (int y = 0; y < h; y++)
        {
            x265amd_pixel* row = org + (intptr_t)y * st;
            for (int x = 1; x <= mx; x++) { row[-x] = row[0]; row[w - 1 + x] = row[w - 1]; }
        }
        for (int y = 1; y <= my; y++)
        {
            memcpy(org + (intptr_t)(-y) * st - mx, org - mx, (size_t)(w + 2 * mx) * sizeof(x265amd_pixel));
            memcpy(org + (intptr_t)(h - 1 + y) * st - mx, org + (intptr_t)(h - 1) * st - mx, (size_t)(w + 2 * mx) * sizeof(x265amd_pixel));
        }
    }
    return X265AMD_OK;
}
