/* The per-pixel arithmetic of the edge-based adaptive quantisation modes (--aq-mode 4 / 5; reference: computeEdge, source/encoder/slicetype.cpp:98-157),
 * ONE source for the device kernel (lowres_kernels.hip: k_aq_edge) and for host code (tests/native/aq_theta_check.cpp walks every gradient pair through it).
 *
 * What has to come out is what the reference's -O2 -ffast-math build computes from the two Sobel gradients gV, gH (integers, |g| <= 16 * the largest sample):
 *   rad   = (float)atan2((double)gV, (double)gH)            -- the DOUBLE arctangent, rounded to float
 *   t     = (float)((double)(rad * 180.0f) * C)             -- a float product; C = the double nearest to 1 / 3.14159265 (the source's PI; the division became a product)
 *   if (t < 0) t = t + 180.0f;  theta = (pixel)t            -- truncated; 180 occurs (gV slightly negative)
 *   edge  = gH * gH + gV * gV >= T * T ? white : 0          -- on floats there, the square root gone; T = white = the largest sample.  Every sum near T * T is
 *                                                              below 2^24, so the integer test says the same
 *
 * Nothing here calls a maths library: two libraries' "< 1 ulp" arctangents are not the same function, and the integer theta decides QP offsets.  xa_edge_atan2 uses
 * only operations IEEE 754 defines exactly (integer arithmetic, double add / multiply / divide, conversions), so host and device give the same bits PROVIDED no
 * product and sum are fused: contraction is switched off below, for clang inside the functions (the device compiler contracts by default) and for GCC round them
 * (it contracts by default as soon as the target has a fused operation, -mfma or -march=native); build.sh and the test pass -ffp-contract=off as well.
 * Its error is about one ulp of a double, as the host library's is; the two could only disagree on theta where the true angle lies within ~1e-16 of a value at
 * which the float chain steps to the next integer degree.  The CPU test finds no such pair in the whole 8-bit and 10-bit ranges (it would be listed here as an
 * exception if it did). */
#ifndef X265AMD_AQ_EDGE_DEV_H
#define X265AMD_AQ_EDGE_DEV_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XA_EDGE_HD __host__ __device__
#else
#define XA_EDGE_HD
#endif

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

/* atan2((double)gv, (double)gh) for integers |g| < 2^15.  With n <= d the two magnitudes: atan(n / d) = atan(k / 16) + atan(r), r = (16 n - k d) / (16 d + k n) for the
 * k that makes |r| <= 1/32 (both terms of the quotient are exact integers: one rounding); atan(k / 16) from a table in two parts, atan(r) by its series up to r^13
 * (the next term is below 2^-74 r); then the octant. */
XA_EDGE_HD inline double xa_edge_atan2(int gv, int gh)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double atanTab[17][2] = {
        { 0x0.0p+0, 0x0.0p+0 },
        { 0x1.ff55bb72cfdeap-5, -0x1.c934d86d23f1dp-60 },
        { 0x1.fd5ba9aac2f6ep-4, -0x1.cd37686760c17p-59 },
        { 0x1.7b97b4bce5b02p-3, 0x1.347b0b4f881cap-58 },
        { 0x1.f5b75f92c80ddp-3, 0x1.8ab6e3cf7afbdp-57 },
        { 0x1.362773707ebccp-2, -0x1.963a544b672d8p-57 },
        { 0x1.6f61941e4def1p-2, -0x1.c63aae6f6e918p-56 },
        { 0x1.a64eec3cc23fdp-2, -0x1.24dec1b50b7ffp-56 },
        { 0x1.dac670561bb4fp-2, 0x1.a2b7f222f65e2p-56 },
        { 0x1.0657e94db30d0p-1, -0x1.d5b495f6349e6p-56 },
        { 0x1.1e00babdefeb4p-1, -0x1.928df287a668fp-58 },
        { 0x1.345f01cce37bbp-1, 0x1.1021137c71102p-55 },
        { 0x1.4978fa3269ee1p-1, 0x1.2419a87f2a458p-56 },
        { 0x1.5d58987169b18p-1, 0x1.0028e4bc5e7cap-57 },
        { 0x1.700a7c5784634p-1, -0x1.8c34d25aadef6p-56 },
        { 0x1.819d0b7158a4dp-1, -0x1.bf76229d3b917p-56 },
        { 0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55 },
    };
    const int ay = gv < 0 ? -gv : gv, ax = gh < 0 ? -gh : gh;
    const int n = ay < ax ? ay : ax, d = ay < ax ? ax : ay;
    double a = 0.0;
    if (d)
    {
        const int k = (32 * n + d) / (2 * d);
        const double r = (double)(16 * n - k * d) / (double)(16 * d + k * n), s = r * r;
        double p = 0x1.3b13b13b13b14p-4;                     /* 1/13, -1/11, 1/9, -1/7, 1/5, -1/3 */
        p = p * s - 0x1.745d1745d1746p-4;
        p = p * s + 0x1.c71c71c71c71cp-4;
        p = p * s - 0x1.2492492492492p-3;
        p = p * s + 0x1.999999999999ap-3;
        p = p * s - 0x1.5555555555555p-2;
        p = p * s;
        a = atanTab[k][0] + (atanTab[k][1] + (r + r * p));
    }
    if (ay > ax) a = 0x1.921fb54442d18p+0 - (a - 0x1.1a62633145c07p-54);           /* pi/2 - a */
    if (gh < 0) a = 0x1.921fb54442d18p+1 - (a - 0x1.1a62633145c07p-53);            /* pi - a */
    return gv < 0 ? -a : a;
}

/* edgeTheta's value for the gradient pair: 0..180 */
XA_EDGE_HD inline int xa_edge_theta(int gv, int gh)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float rad = (float)xa_edge_atan2(gv, gh);
    const float deg = rad * 180.0f;
    float t = (float)((double)deg * 0x1.45f306e2dc32dp-2);     /* the double nearest to 1 / 3.14159265 */
    if (t < 0) t = t + 180.0f;
    return (int)t;
}

/* edgePic's value: `white` where the gradient's magnitude reaches the threshold (both are the largest sample: 255 / 1023) */
XA_EDGE_HD inline int xa_edge_is_edge(int gv, int gh, int white)
{
    return gv * gv + gh * gh >= white * white;
}

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC pop_options
#endif

#endif
