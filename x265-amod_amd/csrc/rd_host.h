/* The rate-distortion helpers the CU orchestrators share (ctu_analysis.hip, intra_rd.hip, inter_rd.hip): the reference's cost types and arithmetic, the entropy
 * coder's snapshots, the quantiser's QPs, the pooled buffers and the scope that lends a CU's place in the picture's unit map to a candidate (CuScope: intra_rd.hip,
 * inter_rd.hip).  Host code only; every including file gets its own copy (anonymous namespace). */
#ifndef X265AMD_RD_HOST_H
#define X265AMD_RD_HOST_H

#include "x265amd_host.h"
#include "../host/cabac_coder.h"
#include <string.h>
#include <vector>

namespace {

#if X265AMD_DEPTH < 10
typedef uint32_t sse_t;             /* common/common.h:142-146 */
#else
typedef uint64_t sse_t;
#endif
struct Cost { uint64_t rdcost; uint32_t bits; sse_t distortion; uint32_t energy; };       /* search.h:  struct Cost */
const uint64_t kMaxCost = 0x7FFFFFFFFFFFFFFFULL;

/* Entropy::store / load (entropy.h:120-140): the contexts and the fractional bit count */
struct Snap { uint8_t ctx[X265AMD_CTX_STRIDE]; uint64_t frac; };
inline void store(Snap& s, const x265amd_cabac& c) { memcpy(s.ctx, c.ctx, X265AMD_CTX_STRIDE); s.frac = c.fracBits; }
inline void load(x265amd_cabac& c, const Snap& s) { memcpy(c.ctx, s.ctx, X265AMD_CTX_STRIDE); c.fracBits = s.frac; }

struct DevBuf
{
    void* p = nullptr;
    ~DevBuf() { xa_scratch_free(p); }
    hipError_t alloc(size_t bytes) { return xa_scratch_alloc(&p, bytes ? bytes : 16); }
};
struct MappedBuf : XaMapped { void free() { xa_mapped_free(p); p = nullptr; } };

/* The bit-counting coder of one call, or a CU's units as the caller had them, or both: the units go back and the coder is closed on every way out. */
struct CuScope
{
    x265amd_cabac* coder = nullptr;
    x265amd_cu_unit* first = nullptr; int w4 = 0, u4 = 0;          /* the CU's first unit in the picture's map, the map's row length, the CU's extent in units */
    x265amd_cu_unit* candidate = nullptr;                          /* put(): where the map's version of the CU goes before the saved units return */
    std::vector<x265amd_cu_unit> saved;
    x265amd_cu_unit* row(int yy) const { return first + (size_t)yy * w4; }
    /* the coder the analysis of a CTU counts bits with; false: the slice description does not make one */
    bool open(const x265amd_slice_info* si, x265amd_cu_unit* units)
    {
        coder = x265amd_cabac_open(si, units, 1);
        if (coder) coder->ctuInProgress = true;          /* the analysis of a CTU asks (cabac_coder.h: lastQP) */
        return coder != nullptr;
    }
    void save(x265amd_cu_unit* first_, int w4_, int u4_)
    {
        first = first_; w4 = w4_; u4 = u4_;
        saved.resize((size_t)u4 * u4);
        for (int yy = 0; yy < u4; yy++) memcpy(&saved[(size_t)yy * u4], row(yy), sizeof(x265amd_cu_unit) * u4);
    }
    /* save(), then a candidate's own units (raster, row length u4) take the CU's place in the map */
    void put(x265amd_cu_unit* first_, int w4_, int u4_, x265amd_cu_unit* cu_units)
    {
        save(first_, w4_, u4_);
        candidate = cu_units;
        for (int yy = 0; yy < u4; yy++) memcpy(row(yy), candidate + (size_t)yy * u4, sizeof(x265amd_cu_unit) * u4);
    }
    ~CuScope()
    {
        for (int yy = 0; yy < u4; yy++)
        {
            if (candidate) memcpy(candidate + (size_t)yy * u4, row(yy), sizeof(x265amd_cu_unit) * u4);
            memcpy(row(yy), &saved[(size_t)yy * u4], sizeof(x265amd_cu_unit) * u4);
        }
        if (coder) x265amd_cabac_close(coder);
    }
};

inline uint32_t zUnit(int ux, int uy)           /* z-order of the 4x4 unit (ux, uy) inside its CTU */
{
    uint32_t r = 0;
    for (int b = 0; b < 4; b++) r |= (((uint32_t)ux >> b) & 1u) << (2 * b) | (((uint32_t)uy >> b) & 1u) << (2 * b + 1);
    return r;
}
/* the QP of a CU's lambdas (x265amd_rd_cu.reserved[0] when it differs from the quantiser's: QPs above 51) */
inline int lambdaQpOf(const x265amd_rd_cu& cu) { return cu.reserved[0] ? (int)cu.reserved[0] : (int)cu.qp; }

/* g_chromaScale (4:2:0, H.265 table 8-10): the chroma QP of a luma QP */
const uint8_t kChromaScale[58] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31,
                                   32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51 };
/* Quant::setQPforQuant (quant.cpp:221-244) with chroma QP offsets 0: the scaled QPs of the luma and the chroma transform units of a CU coded at `qp` */
inline void quantQps(int qp, int& lumaScaled, int& chromaScaled)
{
    const int bd = 6 * (X265AMD_DEPTH - 8), qpQuant = qp < 0 ? 0 : (qp > 51 ? 51 : qp);
    lumaScaled = qpQuant + bd; chromaScaled = (qpQuant >= 30 ? kChromaScale[qpQuant] : qpQuant) + bd;
}

struct RdCost           /* rdcost.h:99-153 */
{
    uint64_t lambda2, lambda; uint32_t psyRd;
    void setQP(int qp, int sliceType, double psyRdScale)
    {
        uint64_t rd[6];
        x265amd_rdcost(qp, sliceType, psyRdScale, 0, 0, 0, rd);
        lambda2 = rd[0]; lambda = rd[1]; psyRd = (uint32_t)rd[2];
    }
    uint64_t calcRdCost(sse_t dist, uint32_t b) const { return dist + (((uint64_t)b * lambda2 + 128) >> 8); }
    uint64_t calcPsyRdCost(sse_t dist, uint32_t b, uint32_t energy) const { return dist + ((lambda * psyRd * energy) >> 24) + (((uint64_t)b * lambda2) >> 8); }
    uint64_t calcRdSADCost(uint32_t sadCost, uint32_t b) const { return sadCost + (((uint64_t)b * lambda + 128) >> 8); }
    uint64_t cost(sse_t dist, uint32_t b, uint32_t energy) const { return psyRd ? calcPsyRdCost(dist, b, energy) : calcRdCost(dist, b); }
};

} // namespace

#endif
