/* One unit of a host motion field into its mirror in device memory (motion_map.hip: xa_devmap_*; inter_chain_dev.h: XaMapUnit), as two 8-byte stores
 * through the BAR mapping.  Used by the CTU analysis, the frame loop and the mirrors' own row push. */
#ifndef X265AMD_MOTION_MAP_H
#define X265AMD_MOTION_MAP_H
#include "x265amd_host.h"
#include "inter_chain_dev.h"

static inline void devmap_store(XaMapUnit* d, const x265amd_mv_unit& v, int depth)
{
    union { XaMapUnit u; uint64_t w[2]; } t;
    t.w[0] = t.w[1] = 0;
    t.u.pred_mode = v.pred_mode; t.u.inter_dir = v.inter_dir; t.u.ref_idx[0] = v.ref_idx[0]; t.u.ref_idx[1] = v.ref_idx[1];
    t.u.mv[0][0] = v.mv[0][0]; t.u.mv[0][1] = v.mv[0][1]; t.u.mv[1][0] = v.mv[1][0]; t.u.mv[1][1] = v.mv[1][1]; t.u.depth = (uint8_t)depth;
    volatile uint64_t* q = reinterpret_cast<volatile uint64_t*>(d);
    q[0] = t.w[0]; q[1] = t.w[1];
}
#endif
