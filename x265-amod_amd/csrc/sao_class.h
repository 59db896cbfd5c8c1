/* The edge class of a sample against its two neighbours along a direction: SAO::s_eoTable[sign + sign + 2] (reference: source/encoder/sao.cpp:65-72): {1, 2, 0, 3, 4}.
 * ONE source for the device kernels (sao_kernels.hip) and the host model they are compared with (host/sao_stats_model.cpp); nothing else is shared between the two. */
#ifndef X265AMD_SAO_CLASS_H
#define X265AMD_SAO_CLASS_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XA_SAO_HD __host__ __device__ __forceinline__
#else
#define XA_SAO_HD static inline
#endif

XA_SAO_HD int xa_sao_sgn(int v) { return (v > 0) - (v < 0); }
XA_SAO_HD int xa_sao_class(int v, int a, int b)
{
    const int e = xa_sao_sgn(v - a) + xa_sao_sgn(v - b) + 2;
    return e == 2 ? 0 : (e < 2 ? e + 1 : e);
}

#endif
