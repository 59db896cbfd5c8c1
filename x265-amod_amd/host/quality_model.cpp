/* Quality metrics (--psnr, --ssim, measured light levels), the host half (include/x265amd.h).
 * The three *_model functions give, from host planes and without a GPU, the records that the device passes of csrc/quality_kernels.hip have to give: the reference's loops
 * (FrameFilter::processPostRow with computeSSD and calculateSSIM, source/encoder/framefilter.cpp:654-723, :828-853, source/encoder/encoder.cpp:1121 ff.; ssim_4x4x2_core and
 * ssim_end_4, source/common/pixel.cpp:648-718; PicYuv::copyFromPicture, source/common/picyuv.cpp:426-439) restated over the whole picture, with the term arithmetic and the
 * band geometry of csrc/quality_dev.h, the one source the kernels use too.  x265amd_quality_finish is Encoder::finishFrameStats' part (encoder.cpp:2978-3010, :3071). */
#include "x265amd.h"
#include "../csrc/quality_dev.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace {
bool codedSizeOk(int width, int height, int org_width, int org_height)
{
    return width >= 16 && height >= 16 && !(width & 7) && !(height & 7) && org_width > 0 && org_height > 0 && org_width <= width && org_height <= height;
}
}

extern "C" int x265amd_picture_ssd_model(const x265amd_pixel* const src[3], const x265amd_pixel* const rec[3], intptr_t stride, intptr_t cstride, int width, int height,
                                         int org_width, int org_height, uint64_t* ssd)
{
    if (!src || !rec || !ssd || !codedSizeOk(width, height, org_width, org_height) || stride < width || cstride < width / 2) return X265AMD_EINVAL;
    for (int k = 0; k < 3; k++)
    {
        if (!src[k] || !rec[k]) return X265AMD_EINVAL;
        /* the original width, but every row of the coded height (framefilter.cpp:672-673: getCUHeight comes from the padded height) */
        const int w = k ? org_width >> 1 : org_width, h = k ? height >> 1 : height;
        const intptr_t st = k ? cstride : stride;
        uint64_t sum = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
            {
                const int d = (int)src[k][y * st + x] - (int)rec[k][y * st + x];
                sum += (uint64_t)(d * d);
            }
        ssd[k] = sum;
    }
    return X265AMD_OK;
}

extern "C" int x265amd_picture_ssim_model(const x265amd_pixel* src_luma, const x265amd_pixel* rec_luma, intptr_t stride, int width, int height, x265amd_ssim_band* bands,
                                          int32_t* block_sums)
{
    if (!src_luma || !rec_luma || !bands || !codedSizeOk(width, height, width, height) || stride < width) return X265AMD_EINVAL;
    const int wb = xa_ssim_wb(width), hb = xa_ssim_hb(height);
    int32_t* sums = (int32_t*)malloc((size_t)wb * hb * 4 * sizeof(int32_t));
    if (!sums) return X265AMD_EINVAL;
    for (int by = 0; by < hb; by++)
        for (int bx = 0; bx < wb; bx++)
        {
            const x265amd_pixel* pix1 = rec_luma + (intptr_t)(2 + 4 * by) * stride + 2 + 4 * bx;
            const x265amd_pixel* pix2 = src_luma + (intptr_t)(2 + 4 * by) * stride + 2 + 4 * bx;
            uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
            for (int y = 0; y < 4; y++)
                for (int x = 0; x < 4; x++)
                {
                    const uint32_t a = pix1[x + y * stride], b = pix2[x + y * stride];
                    s1 += a; s2 += b; ss += a * a; ss += b * b; s12 += a * b;
                }
            int32_t* out = sums + ((size_t)by * wb + bx) * 4;
            out[0] = (int32_t)s1; out[1] = (int32_t)s2; out[2] = (int32_t)ss; out[3] = (int32_t)s12;
        }
    if (block_sums) memcpy(block_sums, sums, (size_t)wb * hb * 4 * sizeof(int32_t));
    const int nb = xa_ssim_bands(height);
    for (int r = 0; r < nb; r++)
    {
        int firstRow, rows;
        xa_ssim_band(height, r, &firstRow, &rows);
        float ssim = 0.0f;      /* calculateSSIM's running float */
        for (int wy = firstRow; wy < firstRow + rows; wy++)
            for (int g0 = 0; g0 < wb - 1; g0 += XA_SSIM_GROUP)
            {
                float terms[XA_SSIM_GROUP];
                const int count = wb - 1 - g0 < XA_SSIM_GROUP ? wb - 1 - g0 : XA_SSIM_GROUP;
                for (int i = 0; i < count; i++)
                {
                    const int32_t* a = sums + ((size_t)wy * wb + g0 + i) * 4;           /* blocks (wx, wy), (wx + 1, wy) */
                    const int32_t* b = a + (size_t)wb * 4;                              /* ... and the two below */
                    int s[4];
                    for (int j = 0; j < 4; j++) s[j] = b[j] + b[4 + j] + a[j] + a[4 + j];
                    terms[i] = xa_ssim_end_1(s[0], s[1], s[2], s[3], X265AMD_DEPTH);
                }
                ssim = XA_Q_ADD(ssim, xa_ssim_group_sum(terms, count));
            }
        memcpy(&bands[r].sum_bits, &ssim, sizeof(float));
        bands[r].cnt = (uint32_t)rows * (uint32_t)(wb - 1);
    }
    free(sums);
    return X265AMD_OK;
}

extern "C" int x265amd_luma_level_model(const x265amd_pixel* luma, intptr_t stride, int org_width, int org_height, x265amd_luma_level_record* level)
{
    if (!luma || !level || org_width <= 0 || org_height <= 0 || stride < org_width) return X265AMD_EINVAL;
    memset(level, 0, sizeof(*level));
    for (int y = 0; y < org_height; y++)
        for (int x = 0; x < org_width; x++)
        {
            const uint32_t v = luma[y * stride + x];
            level->sum += v;
            if (v > level->max) level->max = v;
        }
    return X265AMD_OK;
}

extern "C" int x265amd_quality_finish(const uint64_t* ssd, const x265amd_ssim_band* bands, const x265amd_luma_level_record* level, int width, int height, int org_width,
                                      int org_height, x265amd_quality_values* out)
{
    if (!out || !codedSizeOk(width, height, org_width, org_height)) return X265AMD_EINVAL;
    memset(out, 0, sizeof(*out));
    if (ssd)
    {
        /* encoder.cpp:2979-2994, :3071 */
        const int size = org_width * org_height;
        const int maxval = 255 << (X265AMD_DEPTH - 8);
        const double refValueY = (double)maxval * maxval * size;
        const double refValueC = (double)maxval * maxval * size / 4.0;
        out->psnrY = ssd[0] ? 10.0 * log10(refValueY / (double)ssd[0]) : 99.99;
        out->psnrU = ssd[1] ? 10.0 * log10(refValueC / (double)ssd[1]) : 99.99;
        out->psnrV = ssd[2] ? 10.0 * log10(refValueC / (double)ssd[2]) : 99.99;
        out->psnr = (out->psnrY * 6 + out->psnrU + out->psnrV) / 8;
    }
    if (bands)
    {
        /* FrameEncoder::m_ssim is a double that takes every band's float (framefilter.cpp:708-710); encoder.cpp:3006-3010 */
        double sum = 0.0;
        uint32_t cnt = 0;
        const int nb = xa_ssim_bands(height);
        for (int r = 0; r < nb; r++)
        {
            float f;
            memcpy(&f, &bands[r].sum_bits, sizeof(float));
            sum += f;
            cnt += bands[r].cnt;
        }
        out->ssimCnt = cnt;
        out->ssim = cnt ? sum / cnt : 0.0;
    }
    if (level)
    {
        /* picyuv.cpp:438: the sum over the original size divided by the padded size */
        out->maxLumaLevel = level->max;
        out->avgLumaLevel = (double)level->sum / (height * width);
    }
    return X265AMD_OK;
}
