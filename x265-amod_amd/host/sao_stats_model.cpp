/* The SAO statistics on the host, sample by sample (include/x265amd.h: x265amd_sao_stats_model): what k_sao_stats in its forms and k_sao_stats_pre
 * (csrc/sao_kernels.hip) have to give, word for word, and what the decision of host/sao_rdo.cpp adds up under --sao-non-deblock.
 *
 * (a) SAO::calcSaoStatsCTU (reference: source/encoder/sao.cpp:735-917) on the deblocked planes: per type the samples of the CTU short of skipR columns at the right
 *     and skipB lines at the bottom (plus the plane offset: 0 luma, 2 chroma), whole at the picture's edges; EO_0 is short of its lines at the picture's bottom
 *     edge, too (:836 has no edge case).
 * (b) SAO::calcSaoStatsCu_BeforeDblk (:919-1197) on the planes before deblocking: per type the samples with x >= startX or y >= startY, the skips less the plane
 *     offset; the edge types stop one column / line short of the CTU's end ("not refer right CTU", "not refer below CTU") and of the picture's first column / line.
 * The two regions do not partition the CTU (the offsets have opposite signs): both are written down as the reference has them.
 * Nothing here is shared with the kernels but the class function (csrc/sao_class.h). */
#include "x265amd.h"
#include "../csrc/sao_class.h"
#include <string.h>

namespace {

typedef x265amd_pixel pixel;
enum { BO = 4 };
struct Skip { int b, r; };
/* [non-deblock][type]: type 0..3 = EO_0..3, 4 = BO (sao.cpp:781-782, :812-896, :986-1158) */
const Skip kSkip[2][5] = { { { 4, 5 }, { 4, 5 }, { 4, 5 }, { 4, 5 }, { 4, 5 } }, { { 3, 5 }, { 4, 4 }, { 4, 5 }, { 4, 5 }, { 3, 4 } } };

struct Ctu
{
    const pixel* rec; const pixel* fenc; intptr_t stride;
    int cw, ch, po; bool atLeft, atTop, atRight, atBottom;
};

inline int neighbourClass(const pixel* r, intptr_t stride, int type)
{
    const int v = r[0];
    switch (type)
    {
    case 0: return xa_sao_class(v, r[-1], r[1]);
    case 1: return xa_sao_class(v, r[-stride], r[stride]);
    case 2: return xa_sao_class(v, r[-stride - 1], r[stride + 1]);
    default: return xa_sao_class(v, r[-stride + 1], r[stride - 1]);
    }
}
inline void add(int32_t* count, int32_t* org, int type, int cls, int diff) { count[type * 32 + cls]++; org[type * 32 + cls] += diff; }

void postDeblock(const Ctu& c, int flags, int32_t* count, int32_t* org)
{
    const Skip* skip = kSkip[(flags & X265AMD_SAO_NON_DEBLOCK) ? 1 : 0];
    for (int type = 0; type < 5; type++)
    {
        if ((flags & X265AMD_SAO_EO01_ONLY) && (type == 2 || type == 3)) continue;
        const bool horizontal = type == 0 || type == 2 || type == 3, vertical = type == 1 || type == 2 || type == 3;
        const int x0 = horizontal && c.atLeft ? 1 : 0, y0 = vertical && c.atTop ? 1 : 0;
        const int x1 = c.atRight ? (horizontal ? c.cw - 1 : c.cw) : c.cw - skip[type].r + c.po;
        int y1 = c.atBottom ? (vertical ? c.ch - 1 : c.ch) : c.ch - skip[type].b + c.po;
        if (type == 0) y1 = c.ch - skip[type].b + c.po;
        for (int y = y0; y < y1; y++)
            for (int x = x0; x < x1; x++)
            {
                const pixel* r = c.rec + y * c.stride + x;
                const int diff = (int)c.fenc[y * c.stride + x] - (int)r[0];
                add(count, org, type, type == BO ? r[0] >> (X265AMD_DEPTH - 5) : neighbourClass(r, c.stride, type), diff);
            }
    }
}

void preDeblock(const Ctu& c, int32_t* count, int32_t* org)
{
    const Skip* skip = kSkip[1];
    for (int type = 0; type < 5; type++)
    {
        const bool horizontal = type == 0 || type == 2 || type == 3, vertical = type == 1 || type == 2 || type == 3;
        const int startX = c.atRight ? (horizontal ? c.cw - 1 : c.cw) : c.cw - (skip[type].r - c.po);
        const int startY = c.atBottom ? (vertical ? c.ch - 1 : c.ch) : c.ch - (skip[type].b - c.po);
        const int x0 = horizontal && c.atLeft ? 1 : 0, y0 = vertical && c.atTop ? 1 : 0;
        const int x1 = horizontal ? c.cw - 1 : c.cw, y1 = vertical ? c.ch - 1 : c.ch;
        for (int y = y0; y < y1; y++)
            for (int x = x0; x < x1; x++)
            {
                if (x < startX && y < startY) continue;
                const pixel* r = c.rec + y * c.stride + x;
                const int diff = (int)c.fenc[y * c.stride + x] - (int)r[0];
                add(count, org, type, type == BO ? r[0] >> (X265AMD_DEPTH - 5) : neighbourClass(r, c.stride, type), diff);
            }
    }
}

} // namespace

extern "C" int x265amd_sao_stats_model(const void* const rec_planes[3], const void* const fenc_planes[3], const void* const pre_planes[3], intptr_t stride, intptr_t cstride,
                                       int width, int height, int flags, int32_t* pre_count, int32_t* pre_offset_org, int32_t* count, int32_t* offset_org)
{
    if (flags & ~(X265AMD_SAO_NON_DEBLOCK | X265AMD_SAO_EO01_ONLY)) return X265AMD_EINVAL;
    if (!fenc_planes || width <= 0 || height <= 0 || (width & 7) || (height & 7) || !count != !offset_org || !pre_count != !pre_offset_org) return X265AMD_EINVAL;
    if ((count && !rec_planes) || (pre_count && !pre_planes) || (!count && !pre_count)) return X265AMD_EINVAL;
    for (int plane = 0; plane < 3; plane++)
        if (!fenc_planes[plane] || (count && !rec_planes[plane]) || (pre_count && !pre_planes[plane])) return X265AMD_EINVAL;
    const int ctuW = (width + 63) >> 6, ctuH = (height + 63) >> 6;
    const size_t words = (size_t)ctuW * ctuH * 3 * 5 * 32;
    if (count) { memset(count, 0, words * sizeof(int32_t)); memset(offset_org, 0, words * sizeof(int32_t)); }
    if (pre_count) { memset(pre_count, 0, words * sizeof(int32_t)); memset(pre_offset_org, 0, words * sizeof(int32_t)); }
    for (int cy = 0; cy < ctuH; cy++)
        for (int cx = 0; cx < ctuW; cx++)
            for (int plane = 0; plane < 3; plane++)
            {
                const int sh = plane ? 1 : 0;
                const int picW = width >> sh, picH = height >> sh, lpelx = (cx * 64) >> sh, tpely = (cy * 64) >> sh;
                const int rpelx = lpelx + (64 >> sh) < picW ? lpelx + (64 >> sh) : picW, bpely = tpely + (64 >> sh) < picH ? tpely + (64 >> sh) : picH;
                Ctu c;
                c.stride = plane ? cstride : stride;
                c.cw = rpelx - lpelx; c.ch = bpely - tpely; c.po = plane ? 2 : 0;
                c.atLeft = lpelx == 0; c.atTop = tpely == 0; c.atRight = rpelx == picW; c.atBottom = bpely == picH;
                c.fenc = (const pixel*)fenc_planes[plane] + tpely * c.stride + lpelx;
                const size_t base = ((size_t)(cy * ctuW + cx) * 3 + plane) * 5 * 32;
                if (count) { c.rec = (const pixel*)rec_planes[plane] + tpely * c.stride + lpelx; postDeblock(c, flags, count + base, offset_org + base); }
                if (pre_count) { c.rec = (const pixel*)pre_planes[plane] + tpely * c.stride + lpelx; preDeblock(c, pre_count + base, pre_offset_org + base); }
            }
    return X265AMD_OK;
}
