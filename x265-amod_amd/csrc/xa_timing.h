/* X265AMD_TIMING=1: what the CTU analysis counts (ctu_analysis.hip: the Analyzer writes it) and the frame loop prints per picture (frame_analysis.hip).
 * Host C++ only. */
#ifndef X265AMD_XA_TIMING_H
#define X265AMD_XA_TIMING_H
#include <atomic>
#include <chrono>
#include <stdint.h>
#include "xa_env.h"

inline bool g_timing = xa_env_present("X265AMD_TIMING");
inline double g_stageMs[8];               /* wall time per analysis stage (StageTimer) */
inline std::atomic<uint64_t> g_aheadStat[4];      /* searches started ahead of a leaf's merge check, searches collected, started behind the merge check of a CU with sub-CUs, results the sub-CUs' restriction ruled out */
inline std::atomic<uint64_t> g_chainStat[4], g_chainTicks[8];      /* skip chains run, CUs they skipped, stops (not a skip / vector beyond what is published); the device's stage clock */
inline std::atomic<uint64_t> g_cuStat[2][4][4];   /* [B / P][depth][skipped on the device, merge check on the host, search, intra try] */
struct StageTimer
{
    int k; std::chrono::steady_clock::time_point t0;
    explicit StageTimer(int k_) : k(k_) { if (g_timing) t0 = std::chrono::steady_clock::now(); }
    ~StageTimer() { if (g_timing) g_stageMs[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
/* the chains', searches-ahead's, CUs' and stages' lines on stderr (ctu_analysis.hip); the stage times start again from zero */
void xa_timing_report();
#endif
