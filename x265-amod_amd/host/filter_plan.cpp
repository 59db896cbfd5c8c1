/* The chunking rules of a picture's filter thread when the in-loop filters follow the analysis by columns (include/x265amd.h: x265amd_filter_plan,
 * x265amd_filter_ready; the caller is x265amd_encoder::filterRowsCols, csrc/encoder_frame.hip): host C++, no device work.
 *
 * A CTU row r is filtered in column chunks [c0, c1), each in two steps.  TOP: the vertical edges of the row's first eight lines and its top horizontal edge --
 * which completes the deblocking of the row above.  FULL: the other vertical edges, the inner horizontal edges, the SAO statistics and decisions.  What a step
 * may cover follows from a snapshot of the analysis (analysed[r]: CTUs of row r analysed; the rows only advance):
 *   - a chunk of row r ends at most one CTU behind the analysis of row r (the vertical edge at its right boundary reads both sides' coding data), at the row's
 *     end once the row is analysed completely;
 *   - TOP of row r stays behind FULL of row r - 1 (that row's vertical edges precede this row's top horizontal edge; its decisions are the merge-up candidates);
 *   - FULL of row r stays behind TOP of row r, and one CTU behind the analysis of row r + 1 (whose intra prediction has then read everything it needs of row r's
 *     last line unfiltered: FrameEncoder::m_filterRowDelay, reference source/encoder/frameencoder.cpp:124-126, :1936-1950); without the early TOP step, TOP waits
 *     for row r + 1 as well and both steps are taken together;
 *   - a chunk holds at least min_chunk CTUs (min_chunk_last in the last three CTU rows) unless it ends the row.
 * Behind a TOP step of row r the row r - 1 is final (offsets, borders) up to eight samples short of the step's right end, behind a FULL step of the last row that
 * row itself: the offsets of the last samples need the next chunk's horizontal edges.  (What the filters' reach alone would allow: the deblocking of row k is
 * final left of sample column 64 * c1 -- the vertical edge at 64 * c1 is filtered, the horizontal edges from 64 * c1 on are not -- and an edge offset at column x
 * classifies on column x + 1, in chroma on 2 * (x / 2 + 1): the offsets are final left of 64 * c1 - 2.  The six samples more are slack.) */
#include "x265amd.h"
#include <algorithm>

namespace {

struct Rules
{
    int ctuW, ctuH;
    const int32_t* an; const int32_t* doneTop; const int32_t* doneFull;
    int minChunk, minChunkLast, earlyTop;
    int colsOf(int r) const { return an[r] == ctuW ? ctuW : an[r] - 1; }
    int limTop(int r) const
    {
        int lim = colsOf(r);
        if (r > 0) lim = std::min(lim, (int)doneFull[r - 1]);
        if (!earlyTop && r + 1 < ctuH) lim = std::min(lim, colsOf(r + 1));
        return lim;
    }
    int limFull(int r) const
    {
        int lim = doneTop[r];
        if (r + 1 < ctuH) lim = std::min(lim, colsOf(r + 1));
        return lim;
    }
    /* the last rows are where a chain of pictures waits for each other (they finish last, and cut CTUs make the last row the slowest) */
    int minChunkOf(int r) const { return r >= ctuH - 3 ? minChunkLast : minChunk; }
    bool chunkOk(int r, int c0, int c1) const { return c1 > c0 && (c1 == ctuW || c1 - c0 >= minChunkOf(r)); }
};

bool bad(int width, int height, const int32_t* an, const int32_t* doneTop, const int32_t* doneFull, int minChunk, int minChunkLast)
{
    if (width <= 0 || height <= 0 || (width & 7) || (height & 7) || !an || !doneTop || !doneFull || minChunk < 1 || minChunkLast < 1) return true;
    const int ctuW = (width + 63) >> 6, ctuH = (height + 63) >> 6;
    for (int r = 0; r < ctuH; r++)
        if (an[r] < 0 || an[r] > ctuW || doneTop[r] < 0 || doneTop[r] > ctuW || doneFull[r] < 0 || doneFull[r] > doneTop[r]) return true;
    return false;
}

} // namespace

extern "C" int x265amd_filter_ready(int width, int height, const int32_t* analysed, const int32_t* done_top, const int32_t* done_full,
                                    int min_chunk, int min_chunk_last, int early_top)
{
    if (bad(width, height, analysed, done_top, done_full, min_chunk, min_chunk_last)) return X265AMD_EINVAL;
    const Rules R{ (width + 63) >> 6, (height + 63) >> 6, analysed, done_top, done_full, min_chunk, min_chunk_last, early_top };
    bool allDone = true;
    for (int r = 0; r < R.ctuH; r++)
    {
        if (done_full[r] == R.ctuW) continue;
        allDone = false;
        if (R.chunkOk(r, done_top[r], R.limTop(r))) return 1;
        /* (a FULL step may become possible through the TOP step of the same sweep: the TOP test above covers that case) */
        if (R.chunkOk(r, done_full[r], R.limFull(r))) return 1;
    }
    return allDone ? 1 : 0;
}

extern "C" int x265amd_filter_plan(int width, int height, const int32_t* analysed, int32_t* done_top, int32_t* done_full, int32_t* pub_x,
                                   int min_chunk, int min_chunk_last, int early_top,
                                   x265amd_filter_step* steps, int* num_steps, x265amd_filter_finish* finish, int* num_finish)
{
    if (bad(width, height, analysed, done_top, done_full, min_chunk, min_chunk_last) || !pub_x || !steps || !num_steps || !finish || !num_finish) return X265AMD_EINVAL;
    const Rules R{ (width + 63) >> 6, (height + 63) >> 6, analysed, done_top, done_full, min_chunk, min_chunk_last, early_top };
    const int ctuW = R.ctuW, ctuH = R.ctuH, w4 = width >> 2, h4 = height >> 2;
    int ns = 0, nf = 0;
    /* every step that is ready, top row first: the stream orders them (FULL of row r - 1, TOP of row r, FULL of row r) */
    for (int r = 0; r < ctuH; r++)
    {
        if (done_full[r] == ctuW) continue;
        const int y4b = r * 16, y4e = std::min(h4, y4b + 16), y4t = std::min(y4e, y4b + 2);
        {
            const int c0 = done_top[r], c1 = R.limTop(r);
            if (R.chunkOk(r, c0, c1))
            {
                x265amd_filter_step& s = steps[ns++];
                s.kind = X265AMD_FILTER_TOP; s.row = r; s.col_begin = c0; s.col_end = c1;
                s.y4_begin = y4b; s.y4_end = y4t;
                /* the edge records of the whole row height (both steps read them), + the unit column right of the boundary edge */
                s.rec_y4_end = y4e; s.rec_x4_begin = c0 * 16; s.rec_x4_end = std::min(w4, c1 * 16 + 1);
                done_top[r] = c1;
            }
        }
        {
            const int c0 = done_full[r], c1 = R.limFull(r);
            if (R.chunkOk(r, c0, c1))
            {
                x265amd_filter_step& s = steps[ns++];
                s.kind = X265AMD_FILTER_FULL; s.row = r; s.col_begin = c0; s.col_end = c1;
                s.y4_begin = y4t; s.y4_end = y4e;
                s.rec_y4_end = y4e; s.rec_x4_begin = s.rec_x4_end = 0;
                done_full[r] = c1;
            }
        }
    }
    /* final now: the row above a TOP step (its parameters were decided by its own FULL step, in this sweep at the latest), and the last row behind its FULL step --
     * up to eight samples short of the step's right end */
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < ns; i++)
        {
            const x265amd_filter_step& s = steps[i];
            if (pass == 0 ? (s.kind != X265AMD_FILTER_TOP || s.row == 0) : (s.kind != X265AMD_FILTER_FULL || s.row != ctuH - 1)) continue;
            const int k = pass == 0 ? s.row - 1 : s.row, newX = s.col_end == ctuW ? width : 64 * s.col_end - 8;
            if (newX <= pub_x[k]) continue;
            x265amd_filter_finish& f = finish[nf++];
            f.row = k; f.x_begin = pub_x[k]; f.x_end = newX; f.y_begin = k * 64; f.y_end = std::min(height, k * 64 + 64);
            pub_x[k] = newX;
        }
    *num_steps = ns; *num_finish = nf;
    return X265AMD_OK;
}
