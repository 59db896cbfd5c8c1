/* What the CTU analysis and the batch entry points share about OTHER pictures' data: the guards in front of every read of reference samples, and the mirrors
 * of the motion fields in device memory (declared in x265amd_host.h).  Host code only: no kernel lives here. */
#include "x265amd_dev.h"
#include "motion_map.h"
#include "xa_fiber.h"
#include <immintrin.h>
#include <atomic>
#include <mutex>

/* ---- reference-picture guards (x265amd_host.h): the row task's hooks live in its task slot ---- */
static int xa_ref_guard_wait(int pic, int yMin, int yMax, int xMax)
{
    void** slot = xa_task_slot();
    const XaRowHooks* h = slot ? (const XaRowHooks*)*slot : nullptr;
    if (!h || !h->ref_wait) return 0;
    return h->ref_wait(h->ctx, pic, yMin, yMax, xMax);
}
int xa_ref_guard_mc(const x265amd_mc_job* jobs, int n)
{
    void** slot = xa_task_slot();
    if (!slot || !*slot) return 0;
    int yMin[32], yMax[32], xMax[32];
    for (int k = 0; k < 32; k++) { yMin[k] = 1 << 30; yMax[k] = -(1 << 30); xMax[k] = -(1 << 30); }
    for (int i = 0; i < n; i++)
    {
        const x265amd_mc_job& j = jobs[i];
        const int refs[2] = { j.ref0, j.ref1 };
        const int16_t* mv[2] = { j.mv0, j.mv1 };
        for (int l = 0; l < 2; l++)
        {
            if (refs[l] < 0 || refs[l] >= 32) continue;
            /* the block moved by the vector's full-sample part (floor) with the taps of the 8-tap luma filter around it (chroma reaches no further in luma terms) */
            const int y0 = j.y + (mv[l][1] >> 2) - 4, y1 = j.y + j.h - 1 + (mv[l][1] >> 2) + 5, x1 = j.x + j.w - 1 + (mv[l][0] >> 2) + 5;
            if (y0 < yMin[refs[l]]) yMin[refs[l]] = y0;
            if (y1 > yMax[refs[l]]) yMax[refs[l]] = y1;
            if (x1 > xMax[refs[l]]) xMax[refs[l]] = x1;
        }
    }
    for (int k = 0; k < 32; k++) if (yMax[k] > -(1 << 30)) if (xa_ref_guard_wait(k, yMin[k], yMax[k], xMax[k])) return -1;
    return 0;
}
int xa_ref_guard_me(const x265amd_me_job* jobs, const int* pics, int n)
{
    void** slot = xa_task_slot();
    if (!slot || !*slot) return 0;
    for (int i = 0; i < n; i++)
    {
        const x265amd_me_job& j = jobs[i];
        /* the search area with the interpolation margins and what the pattern / sub-sample refinement may step outside (x265amd_me_plan's bounds) */
        if (xa_ref_guard_wait(pics[i], j.y + j.mvmin[1] - 8, j.y + j.h + j.mvmax[1] + 8, j.x + j.w + j.mvmax[0] + 10)) return -1;
    }
    return 0;
}

/* ---- device-resident motion maps (inter_chain_dev.h): a host motion field (x265amd_mv_unit array) may have a mirror in device memory the host writes through the BAR;
 * the encoder object registers one per picture, frame-level callers without one get a temporary mirror (xa_analyse_frame) ---- */
namespace {
/* blocks are never given back to the runtime while the process lives (hipFree waits for the device, and the job server's kernel is resident): an entry
 * without a host field is a free block of `units` units */
struct DevMapEntry { std::atomic<const void*> host{ nullptr }; void* dev = nullptr; size_t units = 0; };
DevMapEntry g_devMaps[512];
std::mutex g_devMapM;
}
void* xa_devmap_register(const x265amd_mv_unit* host, size_t units)
{
    if (!host || !units || !xa_queues_enabled()) return nullptr;
    std::lock_guard<std::mutex> g(g_devMapM);
    DevMapEntry* blank = nullptr;
    for (DevMapEntry& e : g_devMaps)
    {
        if (e.host.load(std::memory_order_relaxed)) continue;
        if (e.dev && e.units == units) { e.host.store(host, std::memory_order_release); return e.dev; }
        if (!e.dev && !blank) blank = &e;
    }
    if (!blank) return nullptr;
    void* d = nullptr;
    if (hipExtMallocWithFlags(&d, units * sizeof(XaMapUnit), hipDeviceMallocUncached) != hipSuccess) return nullptr;
    blank->dev = d; blank->units = units;
    blank->host.store(host, std::memory_order_release);
    return d;
}
void xa_devmap_unregister(const x265amd_mv_unit* host)
{
    if (!host) return;
    std::lock_guard<std::mutex> g(g_devMapM);
    for (DevMapEntry& e : g_devMaps)
        if (e.host.load(std::memory_order_relaxed) == host) { e.host.store(nullptr, std::memory_order_release); return; }
}
void* xa_devmap_find(const x265amd_mv_unit* host)
{
    if (!host) return nullptr;
    for (DevMapEntry& e : g_devMaps) if (e.host.load(std::memory_order_acquire) == host) return e.dev;
    return nullptr;
}
/* rows [y4a, y4b) of a host field into its mirror (a picture whose rows arrive from another process: x265amd_encoder_import_row) */
void xa_devmap_push_rows(const x265amd_mv_unit* host, const x265amd_cu_unit* units, int w4, int y4a, int y4b)
{
    XaMapUnit* d = (XaMapUnit*)xa_devmap_find(host);
    if (!d) return;
    for (int i = y4a * w4; i < y4b * w4; i++) devmap_store(d + i, host[i], units ? units[i].depth : 0);
    /* the mirror is written through the write-combining BAR mapping and the caller publishes the rows to OTHER threads next (a release fence drains nothing on
     * x86): the units must have left this core's buffers before a row task on another core can queue a command that reads them */
    _mm_sfence();
}
