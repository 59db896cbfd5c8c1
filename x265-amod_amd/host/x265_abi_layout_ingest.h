/* The byte offsets of x265_param.minLuma / maxLuma (two uint16_t; reference: source/x265.h:1911-1916, build 209) and the number of X265_CSP_NV12, beside the generated
 * x265_abi_layout.h: the generator predates the picture ingest pass and its output is pinned as it is.  tests/native/abi_layout_ingest_check.cpp asserts these numbers
 * against the reference's own header. */
#ifndef X265AMD_X265_ABI_LAYOUT_INGEST_H
#define X265AMD_X265_ABI_LAYOUT_INGEST_H
#define X265ABI_PARAM_minLuma 748
#define X265ABI_PARAM_maxLuma 750
#define X265ABI_CSP_I420 1
#define X265ABI_CSP_NV12 4
#endif
