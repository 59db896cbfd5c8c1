/* The byte offset of x265_param.bLimitSAO (an int; reference: source/x265.h, build 209), beside the generated x265_abi_layout.h, which has bSaoNonDeblocked and
 * selectiveSAO but predates the use of this member and is pinned as it is.  tests/native/abi_layout_sao_check.cpp asserts this number against the reference's own header. */
#ifndef X265AMD_X265_ABI_LAYOUT_SAO_H
#define X265AMD_X265_ABI_LAYOUT_SAO_H
#define X265ABI_PARAM_bLimitSAO 836
#endif
