/* The arithmetic of the quality metrics (--psnr, --ssim, measured light levels) that has to give the same bits on the device and on the host: ONE source for the kernels
 * (csrc/quality_kernels.hip) and for the host models (host/quality_model.cpp).
 *
 * SSIM (reference: ssim_4x4x2_core, ssim_end_1, ssim_end_4, source/common/pixel.cpp:648-718; calculateSSIM, source/encoder/framefilter.cpp:828-853; the bands of
 * FrameFilter::processPostRow, framefilter.cpp:692-711), luma only, on the CODED size W x H:
 *   blocks    4x4 samples on a grid offset by (2, 2): block (bx, by) covers samples 2 + 4 bx .. +3, 2 + 4 by .. +3; wb = (W - 2) >> 2 blocks per row, HB = (H - 2) >> 2 rows.
 *             Four sums per block, 32-bit: s1 (reconstruction), s2 (source), ss (both squares), s12 (the products).
 *   windows   window (wx, wy) = blocks (wx, wy), (wx + 1, wy), (wx, wy + 1), (wx + 1, wy + 1), their sums added as ints; wb - 1 per row, HB - 1 rows.
 *   bands     CTU row r (64 lines; the last one: what is left) measures the lines minPix .. maxPix - 1, minPix = r ? 64 r - 10 : 2, maxPix = last ? H : 64 (r + 1) - 4:
 *             hb = (maxPix - minPix) >> 2 block rows from block row (minPix - 2) >> 2 on, hb - 1 window rows, cnt = (hb - 1)(wb - 1).  The bands' window rows tile
 *             0 .. HB - 2 without gap or overlap.
 *   order     float32 sums are ORDERED: the windows of a row go four at a time, a group's sum starts at 0.0f and takes its (up to) four terms left to right
 *             (ssim_end_4); the group sums are added one by one, row by row, to the band's float (calculateSSIM).
 *   the term  8-bit: integer vars / covar, c1 / c2 rounded to int, four conversions to float, two products, one quotient -- as written in the source.
 *             10-bit: all float, and the reference is built -ffast-math, which reassociates what the source spells; its build evaluates
 *                 p = fs1 * fs2, t = fs1 * fs1 + fs2 * fs2, covar = fs12 * 64 - p, num = ((covar + covar) + c2) * ((p + p) + c1), den = (t + c1) * ((fss * 64 + c2) - t), num / den
 *             with every operation rounded on its own (no fused multiply-add: the reference's target has none).  tests/golden/make_quality_golden.py asserts this order
 *             against the reference library's own ssim_end_4 on every window of its 10-bit plane sets.
 * Every float operation below is one IEEE 754 operation: contraction is switched off inside the functions for clang (hipcc would contract a * a + b * b into a fused
 * multiply-add on the device) and round them for GCC; the division is hipcc's correctly rounded one (its default). */
#ifndef X265AMD_QUALITY_DEV_H
#define X265AMD_QUALITY_DEV_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XA_Q_HD __host__ __device__
#else
#define XA_Q_HD
#endif

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

/* one rounding each: plain operators, used only inside functions that switch contraction off (HIP's __fmul_rn / __fadd_rn are plain operators in an inline function of
 * the compiler's header and are fused with their neighbours like any others once inlined) */
#define XA_Q_MUL(a, b) ((a) * (b))
#define XA_Q_ADD(a, b) ((a) + (b))
#define XA_Q_SUB(a, b) ((a) - (b))
#define XA_Q_DIV(a, b) ((a) / (b))

enum { XA_SSIM_GROUP = 4 };         /* windows per ssim_end_4 call */

/* geometry of the block grid, the windows and the bands (all from the coded size) */
XA_Q_HD inline int xa_ssim_wb(int width) { return (width - 2) >> 2; }
XA_Q_HD inline int xa_ssim_hb(int height) { return (height - 2) >> 2; }
XA_Q_HD inline int xa_ssim_groups(int width) { return (xa_ssim_wb(width) - 1 + XA_SSIM_GROUP - 1) / XA_SSIM_GROUP; }
XA_Q_HD inline int xa_ssim_bands(int height) { return (height + 63) >> 6; }
/* band r: its first window row and its number of window rows */
XA_Q_HD inline void xa_ssim_band(int height, int r, int* firstRow, int* rows)
{
    const int last = r == xa_ssim_bands(height) - 1;
    const int minPix = r ? 64 * r - 10 : 2, maxPix = last ? height : 64 * (r + 1) - 4;
    *firstRow = (minPix - 2) >> 2;
    *rows = ((maxPix - minPix) >> 2) - 1;
}

/* ssim_end_1 on a window's four sums, in the bit depth the library is built for */
XA_Q_HD inline float xa_ssim_end_1(int s1, int s2, int ss, int s12, int depth)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int pixelMax = (1 << depth) - 1;
    if (depth > 8)
    {
        const float c1 = (float)(.01 * .01 * pixelMax * pixelMax * 64);
        const float c2 = (float)(.03 * .03 * pixelMax * pixelMax * 64 * 63);
        const float fs1 = (float)s1, fs2 = (float)s2, fss = (float)ss, fs12 = (float)s12;
        const float p = XA_Q_MUL(fs1, fs2);
        const float t = XA_Q_ADD(XA_Q_MUL(fs1, fs1), XA_Q_MUL(fs2, fs2));
        const float covar = XA_Q_SUB(XA_Q_MUL(fs12, 64.0f), p);
        const float num = XA_Q_MUL(XA_Q_ADD(XA_Q_ADD(covar, covar), c2), XA_Q_ADD(XA_Q_ADD(p, p), c1));
        const float den = XA_Q_MUL(XA_Q_ADD(t, c1), XA_Q_SUB(XA_Q_ADD(XA_Q_MUL(fss, 64.0f), c2), t));
        return XA_Q_DIV(num, den);
    }
    const int c1 = (int)(.01 * .01 * pixelMax * pixelMax * 64 + .5);
    const int c2 = (int)(.03 * .03 * pixelMax * pixelMax * 64 * 63 + .5);
    const int vars = ss * 64 - s1 * s1 - s2 * s2;
    const int covar = s12 * 64 - s1 * s2;
    const float num = XA_Q_MUL((float)(2 * s1 * s2 + c1), (float)(2 * covar + c2));
    const float den = XA_Q_MUL((float)(s1 * s1 + s2 * s2 + c1), (float)(vars + c2));
    return XA_Q_DIV(num, den);
}

/* ssim_end_4: `count` (1 .. 4) terms added left to right to 0.0f */
XA_Q_HD inline float xa_ssim_group_sum(const float* terms, int count)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float sum = 0.0f;
    for (int i = 0; i < count; i++) sum = XA_Q_ADD(sum, terms[i]);
    return sum;
}

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC pop_options
#endif
#endif
