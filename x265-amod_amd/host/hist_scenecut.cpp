/* Histogram-based scene-cut detection (--hist-scenecut), the host half (include/x265amd.h).
 * x265amd_hist_scene_model is the record, and the quarter-size picture, that the device pass x265amd_hist_scene_stats (csrc/lowres_kernels.hip) has to give: the tail of
 * Lowres::init (reference: source/common/lowres.cpp:35-51, :392-402) and the sample loops of LookaheadTLD::computeIntensityHistogramBinsLuma / Chroma, calculateHistogram,
 * computePictureStatistics and calcVariance (source/encoder/slicetype.cpp:1441-1697), with the raw counts and sums kept apart from what the reference makes of them.
 * x265amd_hist_scene_finish is that rest (the bins' start value and scale, the quotients, the per-band truncation); x265amd_hist_scene_change is
 * Lookahead::detectHistBasedSceneChange (slicetype.cpp:3057-3188) in the reference's operand types and order, with everything that looks wrong in it left as it is. */
#include "x265amd.h"
#include <stdlib.h>
#include <string.h>

namespace {
inline uint64_t* bandsOf(x265amd_hist_scene_record* r) { return (uint64_t*)(r + 1); }
inline const uint64_t* bandsOf(const x265amd_hist_scene_record* r) { return (const uint64_t*)(r + 1); }
/* calculateHistogram (slicetype.cpp:1550-1573) on raw counts */
void histogramOf(const x265amd_pixel* src, uint32_t width, uint32_t height, intptr_t stride, uint8_t dsFactor, uint32_t* histogram, uint64_t* sum)
{
    *sum = 0;
    for (uint32_t v = 0; v < height; v += dsFactor)
    {
        for (uint32_t h = 0; h < width; h += dsFactor) { ++histogram[src[h] & 255]; *sum += src[h]; }
        src += stride << (dsFactor >> 1);
    }
}
/* primitives.cu[].var + acEnergyVarHist (slicetype.cpp:90-96, :1441-1453) */
uint32_t blockVariance(const x265amd_pixel* src, intptr_t stride, int size, int shift)
{
    uint32_t sum = 0, ssd = 0;
    for (int y = 0; y < size; y++)
        for (int x = 0; x < size; x++) { const uint32_t v = src[y * stride + x]; sum += v; ssd += v * v; }
    return (uint32_t)(ssd - ((uint64_t)sum * sum >> shift));
}
}

extern "C" int x265amd_hist_scene_model(const x265amd_pixel* const planes[3], intptr_t stride, intptr_t cstride, const x265amd_pixel* half, intptr_t half_stride,
                                        int width, int height, x265amd_hist_scene_record* record, x265amd_pixel* quarter)
{
    if (!planes || !planes[0] || !planes[1] || !planes[2] || !half || !record || width < 32 || height < 32 || (width & 7) || (height & 7) || stride < width || cstride < width / 2 ||
        half_stride < width / 2 || X265AMD_DEPTH != 8)
        return X265AMD_EINVAL;
    memset(record, 0, X265AMD_HIST_SCENE_RECORD_BYTES(height));
    const int qw = width / 4, qh = height / 4;
    /* frame_lowres_core on the half-size full-pel plane (lowres.cpp:35-51) */
    x265amd_pixel* q = (x265amd_pixel*)malloc((size_t)qw * qh * sizeof(x265amd_pixel));
    if (!q) return X265AMD_EINVAL;
    for (int y = 0; y < qh; y++)
    {
        const x265amd_pixel* src0 = half + (intptr_t)2 * y * half_stride; const x265amd_pixel* src1 = src0 + half_stride;
        for (int x = 0; x < qw; x++)
            q[(size_t)y * qw + x] = (x265amd_pixel)((((src0[2 * x] + src1[2 * x] + 1) >> 1) + ((src0[2 * x + 1] + src1[2 * x + 1] + 1) >> 1) + 1) >> 1);
    }
    if (quarter) memcpy(quarter, q, (size_t)qw * qh * sizeof(x265amd_pixel));
    for (uint32_t i = 0; i < 4; i++)
        for (uint32_t j = 0; j < 4; j++)
        {
            /* luma: the quarter picture's segments (slicetype.cpp:1660-1686) */
            uint32_t segmentWidth = (uint32_t)qw / 4, segmentHeight = (uint32_t)qh / 4;
            uint32_t widthOffset = i == 3 ? (uint32_t)qw - 4 * segmentWidth : 0, heightOffset = j == 3 ? (uint32_t)qh - 4 * segmentHeight : 0;
            histogramOf(q + i * segmentWidth + (size_t)(j * segmentHeight) * qw, segmentWidth + widthOffset, segmentHeight + heightOffset, qw, 1, record->counts[i * 4 + j][0], &record->sums[i * 4 + j][0]);
            /* chroma: the same grid in full-resolution units, halved (slicetype.cpp:1586-1634) */
            segmentWidth = (uint32_t)width / 4; segmentHeight = (uint32_t)height / 4;
            widthOffset = i == 3 ? (uint32_t)width - 4 * segmentWidth : 0; heightOffset = j == 3 ? (uint32_t)height - 4 * segmentHeight : 0;
            for (int c = 1; c < 3; c++)
                histogramOf(planes[c] + ((i * segmentWidth) >> 1) + (intptr_t)((j * segmentHeight) >> 1) * cstride, (segmentWidth + widthOffset) >> 1, (segmentHeight + heightOffset) >> 1, cstride, 4,
                            record->counts[i * 4 + j][c], &record->sums[i * 4 + j][c]);
        }
    free(q);
    /* computePictureStatistics (slicetype.cpp:1458-1545): the bands' sums, untruncated */
    uint64_t* bands = bandsOf(record);
    const int nb = height / 8;
    for (int b = 0; b < nb; b++)
        for (int x = 0; x < width; x += 8) bands[b] += blockVariance(planes[0] + x + (intptr_t)(b * 8) * stride, stride, 8, 6);
    for (int c = 1; c < 3; c++)
        for (int b = 0; b < nb; b++)
            for (int x = 0; x < width / 2; x += 4) bands[c * nb + b] += blockVariance(planes[c] + x + (intptr_t)(b * 4) * cstride, cstride, 4, 4);
    return X265AMD_OK;
}

extern "C" int x265amd_hist_scene_finish(const x265amd_hist_scene_record* record, int width, int height, x265amd_hist_scene_pic* out)
{
    if (!record || !out || width < 32 || height < 32 || (width & 7) || (height & 7)) return X265AMD_EINVAL;
    const uint32_t widthFullRes = (uint32_t)width, heightFullRes = (uint32_t)height;
    const uint32_t quarterSampleLowResWidth = widthFullRes / 4, quarterSampleLowResHeight = heightFullRes / 4;
    uint64_t sumAverageIntensity = 0, sumAverageIntensityCb = 0, sumAverageIntensityCr = 0;
    for (uint32_t i = 0; i < 4; i++)
        for (uint32_t j = 0; j < 4; j++)
        {
            /* bins start at 1 and are scaled by 16 once counted (slicetype.cpp:1594-1597, :1621-1624, :1668-1670, :1690-1694) */
            for (int c = 0; c < 3; c++)
                for (int bin = 0; bin < 256; bin++) out->picHistogram[i][j][c][bin] = (1 + record->counts[i * 4 + j][c][bin]) << 4;
            {
                /* luma (slicetype.cpp:1660-1689) */
                const uint32_t segmentWidth = quarterSampleLowResWidth / 4, segmentHeight = quarterSampleLowResHeight / 4;
                const uint32_t segmentWidthOffset = i == 3 ? quarterSampleLowResWidth - 4 * segmentWidth : 0;
                const uint32_t segmentHeightOffset = j == 3 ? quarterSampleLowResHeight - 4 * segmentHeight : 0;
                const uint64_t sum = record->sums[i * 4 + j][0];
                out->averageIntensityPerSegment[i][j][0] = (uint8_t)((sum + (((segmentWidth + segmentWidthOffset) * (segmentWidth + segmentHeightOffset)) >> 1)) / ((segmentWidth + segmentWidthOffset) * (segmentHeight + segmentHeightOffset)));
                sumAverageIntensity += sum << 4;
            }
            {
                /* chroma (slicetype.cpp:1586-1639) */
                const uint32_t segmentWidth = widthFullRes / 4, segmentHeight = heightFullRes / 4;
                const uint32_t segmentWidthOffset = i == 3 ? widthFullRes - 4 * segmentWidth : 0;
                const uint32_t segmentHeightOffset = j == 3 ? heightFullRes - 4 * segmentHeight : 0;
                uint64_t sum = record->sums[i * 4 + j][1] << 4;
                sumAverageIntensityCb += sum;
                out->averageIntensityPerSegment[i][j][1] =
                    (uint8_t)((sum + (((segmentWidth + segmentWidthOffset) * (segmentHeight + segmentHeightOffset)) >> 3)) / (((segmentWidth + segmentWidthOffset) * (segmentHeight + segmentHeightOffset)) >> 2));
                sum = record->sums[i * 4 + j][2] << 4;
                sumAverageIntensityCr += sum;
                out->averageIntensityPerSegment[i][j][2] =
                    (uint8_t)((sum + (((segmentWidth + segmentWidthOffset) * (segmentHeight + segmentHeightOffset)) >> 3)) / (((segmentWidth + segmentHeightOffset) * (segmentHeight + segmentHeightOffset)) >> 2));
            }
        }
    /* collectPictureStatistics (slicetype.cpp:1717-1719) */
    out->averageIntensity[0] = (uint8_t)((sumAverageIntensity + ((widthFullRes * heightFullRes) >> 1)) / (widthFullRes * heightFullRes));
    out->averageIntensity[1] = (uint8_t)((sumAverageIntensityCb + ((widthFullRes * heightFullRes) >> 3)) / ((widthFullRes * heightFullRes) >> 2));
    out->averageIntensity[2] = (uint8_t)((sumAverageIntensityCr + ((widthFullRes * heightFullRes) >> 3)) / ((widthFullRes * heightFullRes) >> 2));
    /* computePictureStatistics (slicetype.cpp:1486-1489, :1517-1520, :1541-1544): each band's quotient goes through a uint16_t */
    const uint64_t* bands = bandsOf(record);
    const int nb = height / 8;
    uint16_t* const dst[3] = { &out->picAvgVariance, &out->picAvgVarianceCb, &out->picAvgVarianceCr };
    for (int c = 0; c < 3; c++)
    {
        const int maxCol = c ? width >> 1 : width, maxRow = c ? height >> 1 : height;
        uint64_t picTotVariance = 0;
        for (int b = 0; b < nb; b++) picTotVariance += (uint16_t)(bands[c * nb + b] / maxCol);
        *dst[c] = (uint16_t)(picTotVariance / maxRow);
    }
    return X265AMD_OK;
}

extern "C" void x265amd_hist_scene_state_init(x265amd_hist_scene_state* s)
{
    /* Lookahead::Lookahead (slicetype.cpp:1072-1095) */
    memset(s, 0, sizeof(*s));
    s->resetRunningAvg = 1;
    s->segmentCountThreshold = (uint32_t)(((float)((4 * 4) * 50) / 100) + 0.5);
}

#define XA_ABS(a) ((a) < 0 ? -(a) : (a))

extern "C" int x265amd_hist_scene_change(const x265amd_hist_scene_pic* prev, const x265amd_hist_scene_pic* cur, const x265amd_hist_scene_pic* next, int width, int height,
                                         x265amd_hist_scene_state* state, int32_t* verdicts)
{
    if (!prev || !cur || !next || !state || width <= 0 || height <= 0) return -1;
    uint32_t abruptChangeCount = 0, sceneChangeCount = 0;
    /* (never reset inside the loops: the remainders accumulate from segment to segment -- and once segmentWidth has grown, the last column's "remainder" is a wrapped
     * difference that takes it back down, all in uint32_t as in the reference) */
    uint32_t segmentWidth = (uint32_t)width / 4, segmentHeight = (uint32_t)height / 4;
    /* the pictures' variances pick the higher or the lower threshold per 64x64 block of the segment (slicetype.h:49-57, :63; slicetype.cpp:3103-3116): `high` and `low`
     * are multiplied by NUM64x64INPIC, (w * h) >> 12 in uint32_t; the chroma pair is the unparenthesised 3500/4 and 2250/4 in front of the product, 875 and 562 */
    auto threshold = [](uint16_t c, uint16_t p, int64_t diffTh, int varTh, uint32_t high, uint32_t low, uint32_t blocks) -> uint32_t {
        return ((XA_ABS((int64_t)c - (int64_t)p)) > diffTh && (c > varTh || p > varTh)) ? high * blocks : low * blocks;
    };
    for (uint32_t i = 0; i < 4; i++)
        for (uint32_t j = 0; j < 4; j++)
        {
            segmentWidth += i == 3 ? (uint32_t)width - 4 * segmentWidth : 0;
            segmentHeight += j == 3 ? (uint32_t)height - 4 * segmentHeight : 0;
            const uint32_t blocks = (segmentWidth * segmentHeight) >> (6 << 1);
            const uint32_t th[3] = { threshold(cur->picAvgVariance, prev->picAvgVariance, 390, 1500, 3500, 2250, blocks),
                                     threshold(cur->picAvgVarianceCb, prev->picAvgVarianceCb, 10, 20, 3500 / 4, 2250 / 4, blocks),
                                     threshold(cur->picAvgVarianceCr, prev->picAvgVarianceCr, 10, 20, 3500 / 4, 2250 / 4, blocks) };
            uint32_t* const avg[3] = { &state->accHistDiffRunningAvg[i][j], &state->accHistDiffRunningAvgCb[i][j], &state->accHistDiffRunningAvgCr[i][j] };
            /* accumulated absolute histogram difference to the picture before, its distance from the running average (slicetype.cpp:3118-3140) */
            bool isAbruptChange = false, isSceneChange = false;
            uint32_t accHistDiff[3];
            for (int c = 0; c < 3; c++)
            {
                accHistDiff[c] = 0;
                for (uint32_t bin = 0; bin < 256; ++bin) accHistDiff[c] += XA_ABS((int32_t)cur->picHistogram[i][j][c][bin] - (int32_t)prev->picHistogram[i][j][c][bin]);
                if (state->resetRunningAvg) *avg[c] = accHistDiff[c];
                const uint32_t error = XA_ABS((int32_t)*avg[c] - (int32_t)accHistDiff[c]);
                if (error > th[c] && accHistDiff[c] >= error) isAbruptChange = true;
            }
            int32_t verdict = 0;
            if (isAbruptChange)
            {
                /* slicetype.cpp:3144-3160: uint8_t differences of the segment's luma averages; FLASH_TH is the double 1.5, FADE_TH and INTENSITY_CHANGE_TH are 4 */
                const uint8_t* const fu = next->averageIntensityPerSegment[i][j]; const uint8_t* const cu = cur->averageIntensityPerSegment[i][j]; const uint8_t* const pa = prev->averageIntensityPerSegment[i][j];
                const uint8_t futurePast = (uint8_t)XA_ABS((int16_t)fu[0] - (int16_t)pa[0]);
                const uint8_t futurePresent = (uint8_t)XA_ABS((int16_t)fu[0] - (int16_t)cu[0]);
                const uint8_t presentPast = (uint8_t)XA_ABS((int16_t)cu[0] - (int16_t)pa[0]);
                if (futurePresent >= 1.5 * futurePast && presentPast >= 1.5 * futurePast) verdict = X265AMD_HIST_FLASH;
                else if (futurePresent < 4 && presentPast < 4) verdict = X265AMD_HIST_FADE;
                else if (XA_ABS(futurePresent - presentPast) < 4 && futurePresent + presentPast >= futurePast) verdict = X265AMD_HIST_INTENSITY;
                else { isSceneChange = true; verdict = X265AMD_HIST_SCENE; }
                verdict |= (int32_t)futurePast << 8 | (int32_t)futurePresent << 16 | (int32_t)((uint32_t)presentPast << 24);          /* (the three numbers of the reference's debug line) */
            }
            else
                *avg[0] = (3 * *avg[0] + accHistDiff[0]) / 4;          /* (only the luma running average moves) */
            if (verdicts) verdicts[i * 4 + j] = verdict;
            abruptChangeCount += isAbruptChange;
            sceneChangeCount += isSceneChange;
        }
    state->resetRunningAvg = abruptChangeCount >= state->segmentCountThreshold;
    return sceneChangeCount >= state->segmentCountThreshold ? 1 : 0;
}
