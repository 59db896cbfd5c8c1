/* Compile-time check: the layout of x265amd_param_ext that the tests' ctypes mirror assumes, and -- with the reference's headers -- the offset x265_api_abi.cpp reads and
 * writes x265_param.bLimitSAO at (x265-amod_amd/host/x265_abi_layout_sao.h) against the reference's own public header (source/x265.h), in the manner of
 * tests/native/abi_layout_ingest_check.cpp. */
#include "x265amd.h"
#include "x265amd_encoder.h"
#include "x265_abi_layout.h"
#include "x265_abi_layout_sao.h"
#include <cstddef>
static_assert(sizeof(x265amd_param_ext) == 64 && offsetof(x265amd_param_ext, size) == 0 && offsetof(x265amd_param_ext, bSaoNonDeblocked) == 4 && offsetof(x265amd_param_ext, bLimitSAO) == 8 &&
              offsetof(x265amd_param_ext, selectiveSAO) == 12 && offsetof(x265amd_param_ext, reserved) == 16 && sizeof(((x265amd_param_ext*)0)->reserved) == 48, "x265amd_param_ext");
static_assert(X265AMD_SAO_NON_DEBLOCK == 1 && X265AMD_SAO_EO01_ONLY == 2, "the statistics' flags word");
#ifdef WITH_REFERENCE_HEADER
#include "x265.h"
static_assert(X265ABI_BUILD == X265_BUILD, "build");
static_assert(offsetof(x265_param, bLimitSAO) == X265ABI_PARAM_bLimitSAO && sizeof(((x265_param*)0)->bLimitSAO) == sizeof(int) && X265ABI_PARAM_bLimitSAO + sizeof(int) <= X265ABI_SIZEOF_PARAM, "bLimitSAO");
static_assert(offsetof(x265_param, bSaoNonDeblocked) == X265ABI_PARAM_bSaoNonDeblocked && offsetof(x265_param, selectiveSAO) == X265ABI_PARAM_selectiveSAO, "bSaoNonDeblocked / selectiveSAO");
#endif
int main() { return 0; }
