/* Compile-time check: the layout of x265amd_param_tools that the tests' ctypes mirror assumes, the job flag and op numbers of the low-pass transform, and -- with the
 * reference's headers -- the offset x265_api_abi.cpp reads and writes x265_param.bLowPassDct at (x265-amod_amd/host/x265_abi_layout.h) against the reference's own
 * public header (source/x265.h), in the manner of tests/native/abi_layout_sao_check.cpp. */
#include "x265amd.h"
#include "x265amd_encoder.h"
#include "x265_abi_layout.h"
#include <cstddef>
static_assert(sizeof(x265amd_param_tools) == 64 && offsetof(x265amd_param_tools, size) == 0 && offsetof(x265amd_param_tools, bLowPassDct) == 4 &&
              offsetof(x265amd_param_tools, reserved) == 8 && sizeof(((x265amd_param_tools*)0)->reserved) == 56, "x265amd_param_tools");
static_assert(sizeof(x265amd_param_ext) == 64, "x265amd_param_ext stays as it is");
static_assert(sizeof(x265amd_tu_job) == 64 && offsetof(x265amd_tu_job, flags) == 63 && offsetof(x265amd_tu_job, sign_hide) == 62 && X265AMD_TU_LOWPASS == 1, "the job's flags byte");
static_assert(X265AMD_OP_LOWPASS_DCT == 80 && X265AMD_OP_LOWPASS_DCT / 32 == X265AMD_OP_DCT / 32 && X265AMD_OP_LOWPASS_DCT > X265AMD_OP_DEQUANT_SCALING, "the job op");
static_assert(X265AMD_SLICE_SIGN_HIDE == 1 && X265AMD_SLICE_LOWPASS_DCT == 0x100, "the slice record's switches");
#ifdef WITH_REFERENCE_HEADER
#include "x265.h"
static_assert(X265ABI_BUILD == X265_BUILD, "build");
static_assert(offsetof(x265_param, bLowPassDct) == X265ABI_PARAM_bLowPassDct && sizeof(((x265_param*)0)->bLowPassDct) == sizeof(int) && X265ABI_PARAM_bLowPassDct + sizeof(int) <= X265ABI_SIZEOF_PARAM, "bLowPassDct");
#endif
int main() { return 0; }
