/* Compile-time check of the quality metrics' members: x265amd_param.bEnablePsnr / bEnableSsim took the places of two reserved int32 (same offsets, the struct's size
 * unchanged), x265amd_quality is what the header says, and -- with -DWITH_REFERENCE_HEADER and the reference's own public header (source/x265.h) on the include path -- the
 * offsets x265_api_abi.cpp writes x265_stats and x265_sliceType_stats at: the generated x265_abi_layout.h lists globalPsnrY, globalSsim, psnrY and ssim, the members between
 * them are derived there (+ 8 each) and pinned here.  In the manner of tests/native/abi_layout_hist_check.cpp. */
#include "x265amd_encoder.h"
#include <cstddef>
static_assert(offsetof(x265amd_param, bEnablePsnr) == offsetof(x265amd_param, vuiDispWinBottom) + 4 && offsetof(x265amd_param, bEnableAccessUnitDelimiters) == offsetof(x265amd_param, bEnablePsnr) + 4,
              "bEnablePsnr lies between the vui members and bEnableAccessUnitDelimiters");
static_assert(offsetof(x265amd_param, bEnableSsim) == offsetof(x265amd_param, decodedPictureHashSEI) + 4 && offsetof(x265amd_param, deblockingFilterTCOffset) == offsetof(x265amd_param, bEnableSsim) + 4,
              "bEnableSsim lies between decodedPictureHashSEI and the deblocking offsets");
static_assert(sizeof(((x265amd_param*)0)->bEnablePsnr) == 4 && sizeof(((x265amd_param*)0)->bEnableSsim) == 4, "four bytes each");
static_assert(offsetof(x265amd_param, edgeVarThreshold) + 4 == sizeof(x265amd_param), "the struct ends where it did");
static_assert(sizeof(x265amd_picture) == 3 * sizeof(void*) + 6 * 4, "x265amd_picture keeps its size: the quality record has an entry point of its own");
static_assert(offsetof(x265amd_quality, ssimSum) == 24 && offsetof(x265amd_quality, lumaSum) == 32 && offsetof(x265amd_quality, ssimCnt) == 40 && offsetof(x265amd_quality, psnrY) == 48 &&
              offsetof(x265amd_quality, poc) == 96 && sizeof(x265amd_quality) == 112, "x265amd_quality");
#ifdef WITH_REFERENCE_HEADER
#include "x265.h"
#include "x265_abi_layout.h"
static_assert(X265ABI_BUILD == X265_BUILD, "build");
static_assert(offsetof(x265_param, bEnablePsnr) == X265ABI_PARAM_bEnablePsnr && offsetof(x265_param, bEnableSsim) == X265ABI_PARAM_bEnableSsim && offsetof(x265_param, logLevel) == X265ABI_PARAM_logLevel, "x265_param");
static_assert(offsetof(x265_stats, globalPsnrY) == X265ABI_STATS_globalPsnrY && offsetof(x265_stats, globalPsnrU) == X265ABI_STATS_globalPsnrY + 8 &&
              offsetof(x265_stats, globalPsnrV) == X265ABI_STATS_globalPsnrY + 16 && offsetof(x265_stats, globalPsnr) == X265ABI_STATS_globalPsnrY + 24 &&
              offsetof(x265_stats, globalSsim) == X265ABI_STATS_globalSsim, "x265_stats: the global values");
static_assert(offsetof(x265_stats, maxCLL) == X265ABI_STATS_maxCLL && offsetof(x265_stats, maxFALL) == X265ABI_STATS_maxFALL && sizeof(((x265_stats*)0)->maxCLL) == 2 && sizeof(((x265_stats*)0)->maxFALL) == 2,
              "x265_stats: the light levels are 16-bit");
static_assert(offsetof(x265_sliceType_stats, psnrY) == X265ABI_SLICESTATS_psnrY && offsetof(x265_sliceType_stats, psnrU) == X265ABI_SLICESTATS_psnrY + 8 &&
              offsetof(x265_sliceType_stats, psnrV) == X265ABI_SLICESTATS_psnrY + 16 && offsetof(x265_sliceType_stats, ssim) == X265ABI_SLICESTATS_ssim &&
              sizeof(x265_sliceType_stats) == X265ABI_SIZEOF_SLICESTATS, "x265_sliceType_stats");
static_assert(offsetof(x265_stats, statsI) == X265ABI_STATS_statsI && offsetof(x265_stats, statsP) == X265ABI_STATS_statsP && offsetof(x265_stats, statsB) == X265ABI_STATS_statsB &&
              sizeof(x265_stats) == X265ABI_SIZEOF_STATS, "x265_stats");
#endif
int main() { return 0; }
