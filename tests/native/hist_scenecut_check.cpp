/* Stand-alone check of the host half of the histogram scene-cut detection (x265-amod_amd/host/hist_scenecut.cpp), meant to be built with -fsanitize=address,undefined:
 * the model, finish and change on planes allocated at their exact sizes (a read or write past a plane, the record or the quarter picture is the sanitizer's to find), on
 * sizes with and without remainders, with the sums, a flat picture and a checkerboard checked by hand. */
#include "x265amd.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int fail(const char* what, int w, int h) { printf("FAILED: %s at %dx%d\n", what, w, h); return 1; }

static int run(int w, int h, int content, x265amd_hist_scene_pic* out)
{
    std::vector<x265amd_pixel> y((size_t)w * h), cb((size_t)(w / 2) * (h / 2)), cr(cb.size()), half(cb.size()), quarter((size_t)(w / 4) * (h / 4));
    uint32_t s = 12345u + (uint32_t)content;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (x265amd_pixel)(s >> 24); };
    for (auto& v : y) v = content == 0 ? next() : content == 1 ? 255 : 0;
    for (auto& v : cb) v = content == 0 ? next() : 255;
    for (auto& v : cr) v = content == 0 ? next() : 0;
    if (content == 2) for (int j = 0; j < h; j++) for (int i = 0; i < w; i++) y[(size_t)j * w + i] = ((i + j) & 1) ? 255 : 0;
    for (int j = 0; j < h / 2; j++)
        for (int i = 0; i < w / 2; i++)
        {
            const int a = y[(size_t)(2 * j) * w + 2 * i], b = y[(size_t)(2 * j + 1) * w + 2 * i], c = y[(size_t)(2 * j) * w + 2 * i + 1], d = y[(size_t)(2 * j + 1) * w + 2 * i + 1];
            half[(size_t)j * (w / 2) + i] = (x265amd_pixel)((((a + b + 1) >> 1) + ((c + d + 1) >> 1) + 1) >> 1);
        }
    std::vector<unsigned char> rec(X265AMD_HIST_SCENE_RECORD_BYTES(h));
    x265amd_hist_scene_record* r = (x265amd_hist_scene_record*)rec.data();
    const x265amd_pixel* planes[3] = { y.data(), cb.data(), cr.data() };
    if (x265amd_hist_scene_model(planes, w, w / 2, half.data(), w / 2, w, h, r, quarter.data()) != X265AMD_OK) return fail("model", w, h);
    uint64_t counted = 0, sum = 0, qsum = 0;
    for (int g = 0; g < 16; g++) { for (int b = 0; b < 256; b++) counted += r->counts[g][0][b]; sum += r->sums[g][0]; }
    for (auto v : quarter) qsum += v;
    if (counted != quarter.size() || sum != qsum) return fail("luma counts", w, h);
    if (x265amd_hist_scene_model(planes, w, w / 2, half.data(), w / 2, w, h, r, nullptr) != X265AMD_OK) return fail("model without the quarter picture", w, h);
    if (x265amd_hist_scene_finish(r, w, h, out) != X265AMD_OK) return fail("finish", w, h);
    if (content == 1 && (out->averageIntensity[0] != 255 || out->picAvgVariance != 0)) return fail("flat picture", w, h);
    if (content == 2 && out->picAvgVariance != (uint16_t)((uint64_t)(h / 8) * (uint16_t)((uint64_t)(w / 8) * 1040400 / w) / h)) return fail("checkerboard variance", w, h);
    return 0;
}

int main()
{
    static const int sizes[][2] = { { 32, 32 }, { 72, 40 }, { 136, 72 }, { 424, 240 }, { 320, 192 } };
    for (const auto& sz : sizes)
    {
        std::vector<x265amd_hist_scene_pic> pics(3);
        for (int c = 0; c < 3; c++) if (run(sz[0], sz[1], c, &pics[c])) return 1;
        x265amd_hist_scene_state st;
        x265amd_hist_scene_state_init(&st);
        int32_t verdicts[16];
        /* noise -> flat -> checkerboard and back: every order of the three, the state carried along */
        static const int order[][3] = { { 0, 1, 2 }, { 1, 2, 0 }, { 2, 0, 1 }, { 0, 0, 0 }, { 0, 0, 1 }, { 1, 1, 0 } };
        for (const auto& o : order)
        {
            const bool first = st.resetRunningAvg != 0 && &o == &order[0];
            const int r = x265amd_hist_scene_change(&pics[o[0]], &pics[o[1]], &pics[o[2]], sz[0], sz[1], &st, verdicts);
            if (r < 0) return fail("change", sz[0], sz[1]);
            /* the first call sets every running average to the difference it then compares it with: no segment can be abrupt, whatever the pictures */
            if (first && (r != 0 || st.resetRunningAvg != 0)) return fail("the first call after the start reported a change", sz[0], sz[1]);
            if (x265amd_hist_scene_change(&pics[o[0]], &pics[o[1]], &pics[o[2]], sz[0], sz[1], &st, nullptr) < 0) return fail("change without verdicts", sz[0], sz[1]);
        }
        if (x265amd_hist_scene_change(nullptr, &pics[0], &pics[1], sz[0], sz[1], &st, nullptr) >= 0) return fail("null picture accepted", sz[0], sz[1]);
    }
    printf("ok\n");
    return 0;
}
