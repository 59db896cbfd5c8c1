/* Compile-time check: the offset x265_api_abi.cpp reads and writes x265_param.edgeVarThreshold at (x265-amod_amd/host/x265_abi_layout_rskip.h) against the reference's
 * own public header (source/x265.h), in the manner of tests/abi_layout_check.cpp. */
#include "x265.h"
#include "x265_abi_layout.h"
#include "x265_abi_layout_rskip.h"
#include <cstddef>
static_assert(X265ABI_BUILD == X265_BUILD, "build");
static_assert(offsetof(x265_param, edgeVarThreshold) == X265ABI_PARAM_edgeVarThreshold, "edgeVarThreshold");
static_assert(sizeof(((x265_param*)0)->edgeVarThreshold) == sizeof(float) && X265ABI_PARAM_edgeVarThreshold + sizeof(float) <= X265ABI_SIZEOF_PARAM, "edgeVarThreshold is a float inside x265_param");
static_assert(X265_BUILD >= 196, "the edge-based recursion skip: --rskip 2");
int main() { return 0; }
