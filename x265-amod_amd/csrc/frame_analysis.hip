/* The frame loop of the CTU analysis (include/x265amd.h: x265amd_analyse_frame[_ex], x265amd_encode_slice_data; x265amd_host.h: xa_analyse_frame): the CTUs of a
 * picture in raster order or as wavefront row tasks, each through xa_compress_ctu (ctu_analysis.hip), and the final CABAC pass.  Host code only: no kernel lives here. */
#include "x265amd_dev.h"
#include "motion_map.h"
#include "xa_queue.h"
#include "xa_fiber.h"
#include "xa_timing.h"
#include "../host/cabac_coder.h"
#include <string.h>
#include <math.h>
#include <atomic>
#include <chrono>
#include <functional>
#include <vector>

/* The CTU loop of one frame: FrameEncoder::processRowEncoder (reference: source/encoder/frameencoder.cpp:1399-1700) without rate control,
 * VBV, slices or filters: every CTU in raster order (which respects the wavefront dependencies), its start state taken from the row coder
 * (one per row under WPP: row r > 0 starts from the state saved after the second CTU of row r - 1, frameencoder.cpp:1568-1573 / :1596-1598;
 * otherwise one coder runs through all rows), compressCTU, then the row coder codes the CTU in bit-counting mode to advance its state.
 * Without WPP the slice data can be written afterwards (FrameEncoder::encodeSlice, :1298-1370).
 * The reference's row coder only counts bits when SAO is on; without SAO it writes the final bitstream itself (frameencoder.cpp:683-699)
 * and its m_fracBits stays 0, so every CTU then starts from a zero bit fraction (ap->use_sao). */
extern "C" int x265amd_analyse_frame_ex(x265amd_me_ctx* me, void* stream, const x265amd_mvpred_info* I, const x265amd_inter_search_params* S,
                                        const x265amd_slice_info* si, const x265amd_analysis_params* A, x265amd_cu_unit* units, x265amd_mv_unit* cur,
                                        const x265amd_mv_unit* col, const uint8_t* ref_depth, const int8_t* ref_qp0, const uint64_t* h_planes, int num_pics,
                                        intptr_t stride, intptr_t cstride, x265amd_cu_stat* cu_stat, int16_t* coeff_out, x265amd_ctu_result* results,
                                        uint8_t* slice_data, size_t cap, uint32_t* substream_sizes, int* num_substreams, const x265amd_rskip_edge* edge)
{
    const XaAnalysisArgs pic = { me, I, S, si, A, units, cur, col, ref_depth, ref_qp0, h_planes, num_pics, stride, cstride, cu_stat, nullptr, nullptr, edge };
    return xa_analyse_frame(pic, stream, coeff_out, results, slice_data, cap, substream_sizes, num_substreams, nullptr);
}
extern "C" int x265amd_analyse_frame(x265amd_me_ctx* me, void* stream, const x265amd_mvpred_info* I, const x265amd_inter_search_params* S,
                                     const x265amd_slice_info* si, const x265amd_analysis_params* A, x265amd_cu_unit* units, x265amd_mv_unit* cur,
                                     const x265amd_mv_unit* col, const uint8_t* ref_depth, const int8_t* ref_qp0, const uint64_t* h_planes, int num_pics,
                                     intptr_t stride, intptr_t cstride, x265amd_cu_stat* cu_stat, int16_t* coeff_out, x265amd_ctu_result* results,
                                     uint8_t* slice_data, size_t cap, uint32_t* substream_sizes, int* num_substreams)
{
    return x265amd_analyse_frame_ex(me, stream, I, S, si, A, units, cur, col, ref_depth, ref_qp0, h_planes, num_pics, stride, cstride, cu_stat, coeff_out, results, slice_data, cap,
                                    substream_sizes, num_substreams, nullptr);
}

/* hooks (pictures coded in parallel, FrameEncoder::compressFrame's row loop, frameencoder.cpp:880-960): before_row blocks until the reference pictures have
 * finished the rows this CTU row may read; after_row hands the analysed row to the in-loop filters */
int xa_analyse_frame(const XaAnalysisArgs& pic, void* stream, int16_t* coeff_out, x265amd_ctu_result* results, uint8_t* slice_data, size_t cap,
                     uint32_t* substream_sizes, int* num_substreams, const XaRowHooks* hooks)
{
    const x265amd_mvpred_info* I = pic.I; const x265amd_slice_info* si = pic.si; const x265amd_analysis_params* A = pic.A;
    x265amd_cu_unit* units = pic.units; x265amd_mv_unit* cur = pic.cur; const x265amd_mv_unit* col = pic.col; x265amd_cu_stat* cu_stat = pic.cu_stat;
    if (!I || !si || !units || !cur || !cu_stat || !coeff_out) return xa_fail(X265AMD_EINVAL, "analyse_frame: null argument");
    const int ctuW = (si->pic_width + 63) >> 6, ctuH = (si->pic_height + 63) >> 6, numCtu = ctuW * ctuH, w4 = si->pic_width >> 2, h4 = si->pic_height >> 2;
    for (int i = 0; i < w4 * h4; i++)
    {
        memset(&units[i], 0, sizeof(x265amd_cu_unit));
        units[i].qp = (int8_t)si->slice_qp;
        memset(&cur[i], 0, sizeof(x265amd_mv_unit));
        cur[i].ref_idx[0] = cur[i].ref_idx[1] = -1;
    }
    memset(cu_stat, 0, sizeof(x265amd_cu_stat) * (numCtu + 1));          /* FrameData::reinit */
    const bool wpp = si->wpp != 0;
    /* the motion fields' mirrors in device memory (inter_chain_dev.h): the encoder object registers them with its pictures; other callers get them for the call */
    struct TmpMap { const x265amd_mv_unit* h = nullptr; ~TmpMap() { if (h) xa_devmap_unregister(h); } } tmpCur, tmpCol;
    XaMapUnit* frameDCur = (XaMapUnit*)xa_devmap_find(cur);
    const XaMapUnit* frameDCol = (const XaMapUnit*)xa_devmap_find(col);
    if (xa_queues_enabled() && !xa_env_present("X265AMD_DUMP_CTU"))
    {
        if (!frameDCur && (frameDCur = (XaMapUnit*)xa_devmap_register(cur, (size_t)w4 * h4)) != nullptr) tmpCur.h = cur;
        if (col && !frameDCol && si->slice_type != 2 && (frameDCol = (const XaMapUnit*)xa_devmap_register(col, (size_t)w4 * h4)) != nullptr)
        {
            tmpCol.h = col;
            for (int i = 0; i < w4 * h4; i++) devmap_store((XaMapUnit*)frameDCol + i, col[i], 0);
        }
    }
    std::vector<x265amd_cabac*> rows(wpp ? ctuH : 1, nullptr);
    for (size_t r = 0; r < rows.size(); r++)
    {
        rows[r] = x265amd_cabac_open(si, units, 1);
        if (!rows[r]) { for (x265amd_cabac* c : rows) if (c) x265amd_cabac_close(c); return xa_fail(X265AMD_EINVAL, "analyse_frame: slice description"); }
    }
    std::vector<uint8_t> buffered((size_t)ctuH * X265AMD_CTX_STRIDE, 0);
    int rc = X265AMD_OK;
    /* one CTU: analysis with the row coder's state, then the row coder codes it (bits only) to carry the contexts on */
    auto doCtu = [&](int addr, void* st) -> int {
        const int row = addr / ctuW, colIdx = addr % ctuW;
        x265amd_cabac* rowCoder = rows[wpp ? row : 0];
        if (wpp && !colIdx && row)
        {
            /* copyState(m_initSliceContext) + loadContexts(bufferedEntropy of the row above) */
            memcpy(rowCoder->ctx, &buffered[(size_t)(row - 1) * X265AMD_CTX_STRIDE], X265AMD_CTX_STRIDE);
            rowCoder->fracBits = 0;
        }
        x265amd_ctu_result res;
        int16_t* coeff = coeff_out + (size_t)addr * kTileElems;
        int r = xa_compress_ctu(pic, st, addr, rowCoder->ctx, A->use_sao ? rowCoder->fracBits : 0, coeff, &res, frameDCur, frameDCol);
        if (r != X265AMD_OK) return r;
        if (results) results[addr] = res;
        xa_phase(XA_PH_ANALYZER);
        { XA_HOSTPROF("row.cabac_encode_ctu"); r = x265amd_cabac_encode_ctu(rowCoder, addr, coeff, coeff + 4096, coeff + 5120); }
        xa_phase(XA_PH_CABAC_CTU);
        if (wpp && colIdx == 1) memcpy(&buffered[(size_t)row * X265AMD_CTX_STRIDE], rowCoder->ctx, X265AMD_CTX_STRIDE);
        return r;
    };
    int rowThreads = 1;
    if (wpp && ctuH > 1 && ctuW > 1)
    {
        const char* e = xa_env_str("X265AMD_ROW_THREADS");
        rowThreads = e ? atoi(e) : 64;        /* the wavefront never holds more than min(rows, columns / 2) CTUs at once */
        if (rowThreads > ctuH) rowThreads = ctuH;
        if (rowThreads > (ctuW + 1) / 2) rowThreads = (ctuW + 1) / 2;
    }
    const bool dumping = xa_env_present("X265AMD_DUMP_CTU");        /* the dump synchronises the device: not behind a resident kernel */
    if (rowThreads <= 1)
    {
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = xa_fail(X265AMD_EHIP, "analyse_frame: synchronize");
        void* q = dumping ? nullptr : xa_queue_acquire();
        for (int addr = 0; addr < numCtu && rc == X265AMD_OK; addr++)
        {
            if (hooks && addr % ctuW == 0)
            {
                struct W { const XaRowHooks* h; int row; } w{ hooks, addr / ctuW };
                xa_wait_until([](void* c) -> int { W* x = (W*)c; return x->h->row_ready(x->h->ctx, x->row) != 0; }, &w);
                if (hooks->row_ready(hooks->ctx, addr / ctuW) < 0) { rc = xa_fail(X265AMD_EHIP, "analyse_frame: a reference picture failed"); break; }
                hooks->before_row(hooks->ctx, addr / ctuW);
            }
            if (hooks && hooks->ctu_wait && hooks->ctu_wait(hooks->ctx, addr / ctuW, addr % ctuW)) { rc = xa_fail(X265AMD_EHIP, "analyse_frame: a reference picture failed"); break; }
            if (hooks && hooks->before_ctu) hooks->before_ctu(hooks->ctx, addr / ctuW, addr % ctuW);
            rc = doCtu(addr, q ? q : stream);
            if (rc == X265AMD_OK && xa_stream_sync(q ? q : stream) != hipSuccess) rc = xa_fail(X265AMD_EHIP, "analyse_frame: synchronize");
            if (hooks && rc == X265AMD_OK && hooks->after_ctu) hooks->after_ctu(hooks->ctx, addr / ctuW, addr % ctuW);
            if (hooks && rc == X265AMD_OK && addr % ctuW == ctuW - 1) hooks->after_row(hooks->ctx, addr / ctuW);
        }
        if (q) xa_queue_release(q);
    }
    else
    {
        /* Wavefront parallel processing as the reference's row jobs run it (frameencoder.cpp:1399-1968): CTU (r, c) starts when (r - 1, c + 1)
         * is finished -- its neighbours' decisions, reconstruction, cost statistics and the contexts saved after (r - 1, 1) are then final, so
         * every CTU sees exactly what the serial order shows it.  Every CTU row is a task on the worker threads (xa_fiber.h) with a device job queue
         * while it runs; the block operations of different rows overlap on the device, and a row that waits (for the device, for the row above, for
         * a reference picture) leaves its worker thread to the rows that can go on.  A row takes its queue only when the reference pictures let it
         * start and after the row above has taken one, and gives it back at the end of the row: every held queue belongs to a row that can run,
         * whatever the number of pictures in flight, so waiting for a queue always ends. */
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = xa_fail(X265AMD_EHIP, "analyse_frame: synchronize");
        struct Frame
        {
            std::vector<volatile uint64_t*> done;   /* CTUs finished per row: counters the parked rows below wait on (xa_fiber.h) */
            volatile uint64_t* queuedRows;          /* rows that hold (or have held) a queue */
            std::atomic<int> firstErr{ X265AMD_OK };
            const XaRowHooks* hooks; int ctuW, ctuH; bool dumping; int poc; bool intraOnly, intraTry, pSlice;
            std::function<int(int, void*)> doCtu;
            explicit Frame(int rowsN) : done(rowsN) { for (auto& d : done) d = xa_counter_alloc(); queuedRows = xa_counter_alloc(); }
            ~Frame() { for (auto& d : done) xa_counter_free(d); xa_counter_free(queuedRows); }
        } F(ctuH);
        F.hooks = hooks; F.ctuW = ctuW; F.ctuH = ctuH; F.dumping = dumping; F.poc = I->poc; F.doCtu = doCtu; F.intraOnly = si->slice_type == 2; F.pSlice = si->slice_type == 1;
        F.intraTry = si->slice_type == 1 || (si->slice_type == 0 && A->b_intra);       /* pictures whose CUs try intra beside their inter modes */
        struct Row { Frame* f; int row; };
        std::vector<Row> rowsArg((size_t)ctuH);
        std::vector<XaTask> tasks((size_t)ctuH);
        static std::atomic<uint64_t> frameSeq{ 0 };
        const uint64_t seqCall = frameSeq.fetch_add(1);     /* analyses start in coding order: older pictures' rows go first */
        const uint64_t seq = hooks && hooks->order ? hooks->order : seqCall;
        auto rowReady = [](void* c) -> int {
            Row* r = (Row*)c; Frame& f = *r->f;
            if (f.firstErr.load() != X265AMD_OK) return 1;
            return f.hooks ? f.hooks->row_ready(f.hooks->ctx, r->row) != 0 : 1;
        };
        auto rowMain = [](void* c) {
            Row* r = (Row*)c; Frame& f = *r->f;
            const int row = r->row, ctuW = f.ctuW;
            const auto tStart = std::chrono::steady_clock::now();
            if (void** slot = xa_task_slot()) *slot = (void*)f.hooks;          /* the guards of this row's reference reads (xa_ref_guard_*) */
            if (f.hooks && f.firstErr.load() == X265AMD_OK)
            {
                if (f.hooks->row_ready(f.hooks->ctx, row) < 0) { int ok = X265AMD_OK; f.firstErr.compare_exchange_strong(ok, xa_fail(X265AMD_EHIP, "analyse_frame: a reference picture failed")); }
                else f.hooks->before_row(f.hooks->ctx, row);
            }
            void* st = f.dumping ? nullptr : xa_queue_acquire();
            hipStream_t own = nullptr;
            if (!st)
            {
                if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) { int ok = X265AMD_OK; f.firstErr.compare_exchange_strong(ok, xa_fail(X265AMD_EHIP, "analyse_frame: stream")); }
                st = own;
            }
            {
                static const char* const lg = xa_env_str("X265AMD_QUEUE_LOG");
                int lp = -1, lr = -1;
                if (lg && sscanf(lg, "%d,%d", &lp, &lr) == 2 && lp == f.poc && lr == row && st && !own) xa_queue_log(st, lp, lr);
            }
            /* I pictures: a second queue for the row when one is to spare -- the two partitionings of an 8x8 CU are evaluated side by side (intra_rd.hip) */
            void* helper = (f.intraOnly && st && !own) ? xa_queue_try_acquire() : nullptr;
            void* helper2 = helper ? xa_queue_try_acquire() : nullptr;         /* and a third and a fourth: the 16x16 / 32x32 CUs' 2Nx2N evaluations beside their sub-CUs */
            void* helper3 = helper2 ? xa_queue_try_acquire() : nullptr;
            /* P pictures: a second queue for the searches that start ahead of their CU's merge check (Analyzer::searchAhead) */
            const int auxSpare = 112;       /* (an I picture started meanwhile needs four queues per row) */
            void* aux = (f.pSlice && st && !own) ? xa_queue_try_acquire_spare(auxSpare) : nullptr;
            void* aux2 = aux ? xa_queue_try_acquire_spare(auxSpare) : nullptr;                /* and a third for the searches of CUs whose sub-CUs come first */
            if (aux) xa_queue_set_aux(st, aux);
            if (aux2) xa_queue_set_aux(aux, aux2);
            if (helper) xa_queue_set_helper(st, helper);
            if (helper2) xa_queue_set_helper(helper, helper2);
            if (helper3) xa_queue_set_helper(helper2, helper3);
            std::atomic_thread_fence(std::memory_order_release);
            *f.queuedRows = (uint64_t)(row + 1);
            const auto tQueue = std::chrono::steady_clock::now();
            for (int c2 = 0; c2 < ctuW; c2++)
            {
                /* a row of an I picture that started while every queue was taken (the picture behind a scene cut starts beside the pictures in front of it) asks again:
                 * without its second to fourth queue its CTUs take twice as long */
                /* a row of a P picture likewise: the rows that started while an I picture held the queues (in lockstep behind it) are the ones still running when it has
                 * ended -- the tail of the clip, where every link is a last-column CTU searched CU by CU -- and the searches ahead of the merge checks need the second and third queue */
                if (f.pSlice && st && !own && !aux2)
                {
                    if (!aux) { aux = xa_queue_try_acquire_spare(auxSpare); if (aux) xa_queue_set_aux(st, aux); }
                    if (aux && !aux2) { aux2 = xa_queue_try_acquire_spare(auxSpare); if (aux2) xa_queue_set_aux(aux, aux2); }
                }
                if (f.intraOnly && st && !own && !helper3)
                {
                    if (!helper) { helper = xa_queue_try_acquire(); if (helper) xa_queue_set_helper(st, helper); }
                    if (helper && !helper2) { helper2 = xa_queue_try_acquire(); if (helper2) xa_queue_set_helper(helper, helper2); }
                    if (helper2 && !helper3) { helper3 = xa_queue_try_acquire(); if (helper3) xa_queue_set_helper(helper2, helper3); }
                }
                if (row)
                {
                    const int need = c2 + 2 < ctuW ? c2 + 2 : ctuW;
                    const auto w0 = std::chrono::steady_clock::now();
                    const int wc = xa_task_wait_class(1);
                    xa_wait_counter(f.done[row - 1], (uint64_t)need);          /* a failing row sets its counter to the end, so this always ends */
                    xa_task_wait_class(wc);
                    std::atomic_thread_fence(std::memory_order_acquire);
                    xa_prof_dependency_wait((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - w0).count());
                }
                int r2 = f.firstErr.load();
                if (r2 == X265AMD_OK && !st) r2 = X265AMD_EHIP;
                /* the reference pictures are published column by column: this CTU follows them (parked on their counters meanwhile) */
                static const bool ctuLog = xa_env_present("X265AMD_CTU_LOG");
                static const int ctuLogPoc = ctuLog && xa_env_str("X265AMD_CTU_LOG")[0] == 'p' ? atoi(xa_env_str("X265AMD_CTU_LOG") + 1) : -1;       /* "p9": every row of picture 9; anything else: the last three rows of every picture */
                static const auto tLog0 = std::chrono::steady_clock::time_point() + std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double, std::milli>(
                    floor(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count() / 1e6) * 1e6));       /* milliseconds modulo 10^6 of the steady clock: X265AMD_PUB_LOG's clock */
                const double tA = ctuLog ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tLog0).count() : 0;
                const int wc2 = xa_task_wait_class(2);
                if (r2 == X265AMD_OK && f.hooks && f.hooks->ctu_wait && f.hooks->ctu_wait(f.hooks->ctx, row, c2)) r2 = xa_fail(X265AMD_EHIP, "analyse_frame: a reference picture failed");
                xa_task_wait_class(wc2);
                const double tB = ctuLog ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tLog0).count() : 0;
                struct CtuLog { bool on; int poc, row, col; double a, b; uint64_t p0[4], run0;
                                ~CtuLog() { if (!on) return; uint64_t p1[4]; xa_task_parked_ns(p1);
                                            fprintf(stderr, "x265amd ctu: poc %d row %d col %d: row-above wait from %.2f, gate passed %.2f, done %.2f; in the CTU: running %.2f, waiting for the device %.2f, for reference samples %.2f\n", poc, row, col, a, b,
                                                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tLog0).count(), (xa_task_run_ns_always() - run0) / 1e6, (p1[0] - p0[0]) / 1e6, (p1[3] - p0[3]) / 1e6); } }
                    ctuLogger{ ctuLog && (ctuLogPoc >= 0 ? f.poc == ctuLogPoc : row >= f.ctuH - 3), f.poc, row, c2, tA, tB, { 0, 0, 0, 0 }, 0 };
                if (ctuLogger.on) { xa_task_parked_ns(ctuLogger.p0); ctuLogger.run0 = xa_task_run_ns_always(); }
                if (r2 == X265AMD_OK && f.hooks && f.hooks->before_ctu) f.hooks->before_ctu(f.hooks->ctx, row, c2);
                if (r2 == X265AMD_OK) r2 = f.doCtu(row * ctuW + c2, st);
                if (r2 == X265AMD_OK && xa_stream_sync(st) != hipSuccess) r2 = xa_fail(X265AMD_EHIP, "analyse_frame: row stream");
                if (r2 != X265AMD_OK) { int ok = X265AMD_OK; f.firstErr.compare_exchange_strong(ok, r2); }
                std::atomic_thread_fence(std::memory_order_release);
                *f.done[row] = (uint64_t)(c2 + 1);
                if (r2 != X265AMD_OK) break;
                if (f.hooks && f.hooks->after_ctu) f.hooks->after_ctu(f.hooks->ctx, row, c2);
                if (f.hooks && c2 == ctuW - 1) f.hooks->after_row(f.hooks->ctx, row);
            }
            if (f.firstErr.load() != X265AMD_OK) *f.done[row] = (uint64_t)ctuW;
            if (aux2) { xa_queue_set_aux(aux, nullptr); xa_queue_release_helper(aux2); }
            if (aux) { xa_queue_set_aux(st, nullptr); xa_queue_release_helper(aux); }
            if (helper3) { xa_queue_set_helper(helper2, nullptr); xa_queue_release_helper(helper3); }
            if (helper2) { xa_queue_set_helper(helper, nullptr); xa_queue_release_helper(helper2); }
            if (helper) { xa_queue_set_helper(st, nullptr); xa_queue_release_helper(helper); }
            if (own) (void)hipStreamDestroy(own);
            else if (st) xa_queue_release(st);
            if (g_timing && f.hooks)
            {
                static const auto t00 = std::chrono::steady_clock::now();
                auto ms = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(t - t00).count(); };
                fprintf(stderr, "x265amd: row: poc %d row %d start %.1f queue %.1f end %.1f ran %.1f\n", f.poc, row, ms(tStart), ms(tQueue), ms(std::chrono::steady_clock::now()), xa_task_run_ns() / 1e6);
            }
        };
        for (int r = 0; r < ctuH; r++)
        {
            rowsArg[r] = Row{ &F, r };
            tasks[r].fn = rowMain; tasks[r].arg = &rowsArg[r]; tasks[r].ready = rowReady; tasks[r].readyCtx = &rowsArg[r];
            tasks[r].startCounter = F.queuedRows; tasks[r].startValue = (uint64_t)r;          /* after the row above has taken its queue */
            tasks[r].priority = (seq << 12) | (uint64_t)r;
        }
        if (rc == X265AMD_OK)
        {
            xa_tasks_run(tasks.data(), ctuH);
            rc = F.firstErr.load();
            if (rc != X265AMD_OK) xa_fail(rc, "analyse_frame: a CTU row failed");
        }
    }
    for (x265amd_cabac* c : rows) x265amd_cabac_close(c);
    if (g_timing)
    {
        uint64_t ss[3];
        xa_sched_stats(ss);
        xa_phase_report();
        fprintf(stderr, "x265amd: workers so far: %.1f ms running tasks, %.1f ms looking for one, %llu switches\n", ss[0] / 1e6, ss[1] / 1e6, (unsigned long long)ss[2]);
        xa_timing_report();
    }
    if (rc == X265AMD_OK && slice_data && substream_sizes && num_substreams)
    {
        if (A->use_sao) return xa_fail(X265AMD_EINVAL, "analyse_frame: with SAO the slice data follows the SAO decision: call x265amd_encode_slice_data afterwards");
        rc = x265amd_encode_slice_data(si, units, coeff_out, nullptr, nullptr, slice_data, cap, substream_sizes, num_substreams);
    }
    return rc;
}

/* FrameEncoder::encodeSlice (frameencoder.cpp:1298-1370): the final CABAC pass over the decided picture.  One sub-stream per CTU row under WPP
 * (each row starts from the state saved after the second CTU of the row above and ends with finishSlice), otherwise one for the picture; the
 * SAO syntax of a CTU precedes its coding tree when the slice uses SAO. */
extern "C" int x265amd_encode_slice_data(const x265amd_slice_info* si, x265amd_cu_unit* units, const int16_t* coeffs, const x265amd_sao_ctu* sao,
                                         const int32_t* sao_flags, uint8_t* slice_data, size_t cap, uint32_t* substream_sizes, int* num_substreams)
{
    if (!si || !units || !coeffs || !slice_data || !substream_sizes || !num_substreams) return xa_fail(X265AMD_EINVAL, "encode_slice_data: null argument");
    const int ctuW = (si->pic_width + 63) >> 6, ctuH = (si->pic_height + 63) >> 6, numCtu = ctuW * ctuH;
    const bool wpp = si->wpp != 0;
    std::vector<uint8_t> buffered((size_t)ctuH * X265AMD_CTX_STRIDE, 0);
    size_t total = 0;
    int count = 0, rc = X265AMD_OK;
    x265amd_cabac* w = nullptr;
    for (int addr = 0; addr < numCtu && rc == X265AMD_OK; addr++)
    {
        const int row = addr / ctuW, colIdx = addr % ctuW;
        if (!w)
        {
            w = x265amd_cabac_open(si, units, 0);
            if (!w) return xa_fail(X265AMD_EINVAL, "encode_slice_data: slice description");
            if (wpp && row) memcpy(w->ctx, &buffered[(size_t)(row - 1) * X265AMD_CTX_STRIDE], X265AMD_CTX_STRIDE);
        }
        if (sao && sao_flags) w->saoCtu(colIdx, row == 0, sao[addr], sao_flags[0] != 0, sao_flags[1] != 0);
        const int16_t* coeff = coeffs + (size_t)addr * kTileElems;
        rc = x265amd_cabac_encode_ctu(w, addr, coeff, coeff + 4096, coeff + 5120);
        if (wpp && colIdx == 1) memcpy(&buffered[(size_t)row * X265AMD_CTX_STRIDE], w->ctx, X265AMD_CTX_STRIDE);
        if ((wpp && colIdx == ctuW - 1) || addr == numCtu - 1)
        {
            const size_t n = x265amd_cabac_finish_slice(w, slice_data + total, cap > total ? cap - total : 0);
            if (total + n > cap) rc = xa_fail(X265AMD_EINVAL, "encode_slice_data: buffer too small");
            substream_sizes[count++] = (uint32_t)n;
            total += n;
            x265amd_cabac_close(w);
            w = nullptr;
        }
    }
    if (w) x265amd_cabac_close(w);
    *num_substreams = count;
    return rc;
}
