/* Stand-alone check of the host half of the quality metrics (x265-amod_amd/host/quality_model.cpp), meant to be built with -fsanitize=address,undefined for either depth
 * (-DX265AMD_DEPTH=8 / 10): the three models and x265amd_quality_finish on planes, block sums and band records allocated at their exact sizes (a read or write past one of them
 * is the sanitizer's to find), on sizes with one band and with several, with and without a pad, with equal planes and 0 against the maximum checked by hand. */
#include "x265amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int fail(const char* what, int w, int h) { printf("FAILED: %s at %dx%d\n", what, w, h); return 1; }

static int run(int w, int h, int ow, int oh, int content)
{
    const int top = (1 << X265AMD_DEPTH) - 1;
    std::vector<x265amd_pixel> sy((size_t)w * h), su((size_t)(w / 2) * (h / 2)), sv(su.size()), ry(sy.size()), ru(su.size()), rv(su.size());
    uint32_t s = 777u + (uint32_t)content;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (x265amd_pixel)((s >> 16) & (uint32_t)top); };
    for (std::vector<x265amd_pixel>* p : { &sy, &su, &sv }) for (auto& v : *p) v = content == 2 ? 0 : next();
    ry = sy; ru = su; rv = sv;
    if (content == 0) for (std::vector<x265amd_pixel>* p : { &ry, &ru, &rv }) for (auto& v : *p) v = next();
    if (content == 2) for (std::vector<x265amd_pixel>* p : { &ry, &ru, &rv }) for (auto& v : *p) v = (x265amd_pixel)top;
    const x265amd_pixel* src[3] = { sy.data(), su.data(), sv.data() };
    const x265amd_pixel* rec[3] = { ry.data(), ru.data(), rv.data() };
    std::vector<uint64_t> ssd(3);
    if (x265amd_picture_ssd_model(src, rec, w, w / 2, w, h, ow, oh, ssd.data()) != X265AMD_OK) return fail("ssd model", w, h);
    const int wb = (w - 2) >> 2, hb = (h - 2) >> 2, nb = X265AMD_SSIM_BANDS(h);
    std::vector<x265amd_ssim_band> bands((size_t)nb);
    std::vector<int32_t> blocks((size_t)wb * hb * 4);
    if (x265amd_picture_ssim_model(sy.data(), ry.data(), w, w, h, bands.data(), blocks.data()) != X265AMD_OK) return fail("ssim model", w, h);
    x265amd_luma_level_record level;
    if (x265amd_luma_level_model(sy.data(), w, ow, oh, &level) != X265AMD_OK) return fail("level model", w, h);
    x265amd_quality_values v;
    if (x265amd_quality_finish(ssd.data(), bands.data(), &level, w, h, ow, oh, &v) != X265AMD_OK) return fail("finish", w, h);
    if (v.ssimCnt != (uint32_t)((wb - 1) * (hb - 1))) return fail("window count", w, h);
    if (content == 1 && (ssd[0] || ssd[1] || ssd[2] || v.psnrY != 99.99 || v.psnr != 99.99 || fabs(v.ssim - 1.0) > 1e-5)) return fail("equal planes", w, h);
    if (content == 2)
    {
        if (ssd[0] != (uint64_t)top * top * ow * h || ssd[1] != (uint64_t)top * top * (ow / 2) * (h / 2)) return fail("0 against the maximum: ssd", w, h);
        if (level.max != 0 || level.sum != 0 || !(v.ssim > 0.0 && v.ssim < 0.01)) return fail("0 against the maximum: level / ssim", w, h);
        for (int i = 0; i < wb * hb; i++)
            if (blocks[4 * i] != 16 * top || blocks[4 * i + 1] != 0 || blocks[4 * i + 2] != 16 * top * top || blocks[4 * i + 3] != 0) return fail("0 against the maximum: block sums", w, h);
    }
    return 0;
}

int main()
{
    static const int sizes[][4] = { { 64, 16, 64, 16 }, { 72, 136, 72, 136 }, { 424, 240, 420, 236 }, { 16, 16, 2, 2 } };
    for (const auto& z : sizes)
        for (int content = 0; content < 3; content++)
            if (run(z[0], z[1], z[2], z[3], content)) return 1;
    printf("ok\n");
    return 0;
}
