/* Compile-time check: x265amd_param.bHistBasedSceneCut took the place of a reserved int32 (same offset, same four bytes, the struct's size unchanged), and -- with
 * -DWITH_REFERENCE_HEADER and the reference's own public header (source/x265.h) on the include path -- the offset x265_api_abi.cpp reads x265_param.bHistBasedSceneCut at
 * (x265-amod_amd/host/x265_abi_layout.h), in the manner of tests/native/abi_layout_rskip_check.cpp. */
#include "x265amd_encoder.h"
#include <cstddef>
static_assert(offsetof(x265amd_param, bHistBasedSceneCut) == offsetof(x265amd_param, bRepeatHeaders) + 4, "bHistBasedSceneCut follows bRepeatHeaders");
static_assert(offsetof(x265amd_param, vuiSarWidth) == offsetof(x265amd_param, bHistBasedSceneCut) + 4 && sizeof(((x265amd_param*)0)->bHistBasedSceneCut) == 4, "four bytes in front of the vui members");
static_assert(offsetof(x265amd_param, edgeVarThreshold) + 4 == sizeof(x265amd_param), "the struct ends where it did");
#ifdef WITH_REFERENCE_HEADER
#include "x265.h"
#include "x265_abi_layout.h"
static_assert(X265ABI_BUILD == X265_BUILD, "build");
static_assert(offsetof(x265_param, bHistBasedSceneCut) == X265ABI_PARAM_bHistBasedSceneCut, "bHistBasedSceneCut");
static_assert(sizeof(((x265_param*)0)->bHistBasedSceneCut) == sizeof(int), "bHistBasedSceneCut is an int");
#endif
int main() { return 0; }
