/* Compile-time check: the offsets x265_api_abi.cpp reads and writes x265_param.minLuma / maxLuma at and its numbers of the input colour spaces
 * (x265-amod_amd/host/x265_abi_layout_ingest.h) against the reference's own public header (source/x265.h), in the manner of tests/native/abi_layout_rskip_check.cpp;
 * and, with or without the reference's header, the layout of x265amd_surface that the tests' ctypes mirror assumes. */
#include "x265amd.h"
#include "x265amd_encoder.h"
#include "x265_abi_layout.h"
#include "x265_abi_layout_ingest.h"
#include <cstddef>
static_assert(sizeof(x265amd_surface) == 56 && offsetof(x265amd_surface, stride) == 24 && offsetof(x265amd_surface, bitDepth) == 36 && offsetof(x265amd_surface, layout) == 40 &&
              offsetof(x265amd_surface, clipMin) == 44 && offsetof(x265amd_surface, clipMax) == 48, "x265amd_surface");
#ifdef WITH_REFERENCE_HEADER
#include "x265.h"
static_assert(X265ABI_BUILD == X265_BUILD, "build");
static_assert(offsetof(x265_param, minLuma) == X265ABI_PARAM_minLuma && offsetof(x265_param, maxLuma) == X265ABI_PARAM_maxLuma, "minLuma / maxLuma");
static_assert(sizeof(((x265_param*)0)->minLuma) == 2 && sizeof(((x265_param*)0)->maxLuma) == 2, "two uint16_t");
static_assert(X265_CSP_I420 == X265ABI_CSP_I420 && X265_CSP_NV12 == X265ABI_CSP_NV12, "colour space numbers");
#endif
int main() { return 0; }
