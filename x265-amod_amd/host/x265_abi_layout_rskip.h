/* The byte offset of x265_param.edgeVarThreshold (a float; reference: source/x265.h, build 209), beside the generated x265_abi_layout.h: the generator predates the
 * edge-based recursion skip and its output is pinned as it is.  tests/native/abi_layout_rskip_check.cpp asserts this number against the reference's own header. */
#ifndef X265AMD_X265_ABI_LAYOUT_RSKIP_H
#define X265AMD_X265_ABI_LAYOUT_RSKIP_H
#define X265ABI_PARAM_edgeVarThreshold 1248
#endif
