/* The start rule of the frame tasks (include/x265amd.h: x265amd_launch_plan, x265amd_launch_caps; the caller is encoder_encode_impl, csrc/encoder_api.hip): host C++,
 * no device work.  Given the prepared pictures in coding order -- the first one is collected next -- which of them get a frame task now, in which order.
 *
 * IN TURN.  The first picture in coding order always starts (it is the one the caller waits for), and while at most frame_threads tasks run the pictures start in
 * coding order.  Without frame_parallel that is all.  A picture that starts in turn has every picture in front of it started, its references among them.
 *
 * AHEAD OF ITS TURN (frame_parallel only).  An I picture starts as soon as it is typed: nothing it needs comes from another picture, and it takes as long as a dozen
 * of the others.  While a running I picture holds the head of the coding order -- everything behind it waits for its END to be collected, although what the
 * pictures read of each other is only rows apart -- more pictures start than frame_threads + 1, under two conditions:
 *   - EVERY REFERENCE PICTURE OF IT HAS A TASK OR IS COLLECTED.  A task whose reference has none parks at its first CTU and holds a frame slot, row fibers and a
 *     filter thread until that reference's turn comes, which is after the I picture's end: the reference then has nothing to trail, pays a full column of
 *     last-column CTUs on its own, and everything behind it waits for that.  (With the B pyramid and three references a P picture reads the referenced B picture
 *     of the mini-GOP before it: I0 -> P4 -> B2 -> P9 -> B7 -> P14 -> B12 -> P19 is one chain, the referenced B pictures are links of it like the P pictures.)
 *   - first the REFERENCED pictures (P pictures and B pictures that are references), in coding order, while at most frame_threads + ref_cap tasks run: they are the
 *     chain every other picture hangs on.  Then the LEAF b pictures, in coding order, while at most frame_threads + leaf_cap tasks run: they are on nobody's path
 *     but take queues, row tasks, filter threads and frame slots, so by picture size (x265amd_launch_caps).
 * Only behind a running I picture: with P pictures ahead of their turn ALL the time a long clip stood at 52 frames/s where it reaches 100 without -- the pictures far
 * ahead held the places and the queues that the pictures collected next were waiting for -- and a limit of one running I picture helped a long 2160p clip only
 * while they did (profiles/r05_sched_sweep.txt).
 * How many pictures run side by side changes nothing in what they code (the vertical reach of the vectors follows from the parameter frameNumThreads). */
#include "x265amd.h"

namespace {

/* X265_TYPE_* (x265.h:572-577) */
inline bool isIntra(int t) { return t == 1 || t == 2; }

/* today's six P pictures ahead of their turn plus the referenced B pictures between them; the leaf b pictures by size (profiles/r05_early_b_sweep.txt: 2160p clips
 * 15-22 % shorter with 12, the 1080p clips unchanged or longer) */
const int kRefCap = 12;
inline int leafCapOf(int ctuH) { return ctuH > 24 ? 12 : 0; }

} // namespace

extern "C" int x265amd_launch_caps(int ctu_h, int* ref_cap, int* leaf_cap)
{
    if (ctu_h <= 0 || !ref_cap || !leaf_cap) return X265AMD_EINVAL;
    *ref_cap = kRefCap; *leaf_cap = leafCapOf(ctu_h);
    return X265AMD_OK;
}

extern "C" int x265amd_launch_plan(const x265amd_launch_pic* pics, int num_pics, int running, int frame_threads, int ctu_h, int frame_parallel,
                                   int32_t* start, int32_t* ahead, int* num_start)
{
    if (num_pics < 0 || (num_pics && !pics) || running < 0 || frame_threads < 1 || ctu_h <= 0 || !start || !num_start) return X265AMD_EINVAL;
    for (int i = 0; i < num_pics; i++)
    {
        if (pics[i].num_refs < 0 || pics[i].num_refs > X265AMD_LAUNCH_MAX_REFS) return X265AMD_EINVAL;
        /* a reference precedes the picture in coding order (or is collected: -1) */
        for (int k = 0; k < pics[i].num_refs; k++)
            if (pics[i].refs[k] < -1 || pics[i].refs[k] >= i) return X265AMD_EINVAL;
    }
    int n = 0;
    *num_start = 0;
    if (!num_pics) return X265AMD_OK;
    /* started now or before, by place in the list: a bit set would do, the list is short */
    auto startedAt = [&](int i) {
        if (pics[i].started) return true;
        for (int k = 0; k < n; k++) if (start[k] == i) return true;
        return false;
    };
    auto refsStarted = [&](int i) {
        for (int k = 0; k < pics[i].num_refs; k++)
            if (pics[i].refs[k] >= 0 && !startedAt(pics[i].refs[k])) return false;
        return true;
    };
    auto take = [&](int i, int how) { start[n] = i; if (ahead) ahead[n] = how; n++; running++; };

    /* in turn: the head whatever runs, then coding order while at most frame_threads run (the first picture that finds more ends it: `running` only grows) */
    int next = 0;
    for (; next < num_pics; next++)
    {
        if (pics[next].started) continue;
        if (running <= frame_threads || next == 0) take(next, X265AMD_LAUNCH_IN_TURN);
        else break;
    }
    if (frame_parallel && next < num_pics)
    {
        const bool headLong = isIntra(pics[0].type) && startedAt(0) && !pics[0].finished;
        int refCap = 0, leafCap = 0;
        if (headLong) { refCap = kRefCap; leafCap = leafCapOf(ctu_h); }
        /* the chain: I pictures when typed (however many run already), P pictures and referenced B pictures behind a long head */
        for (int i = next; i < num_pics; i++)
        {
            if (startedAt(i)) continue;
            if (isIntra(pics[i].type)) take(i, X265AMD_LAUNCH_INTRA);
            else if (pics[i].referenced && running <= frame_threads + refCap && refCap > 0 && refsStarted(i)) take(i, X265AMD_LAUNCH_AHEAD_REF);
        }
        /* what hangs on it */
        for (int i = next; i < num_pics && leafCap > 0; i++)
            if (!startedAt(i) && !pics[i].referenced && !isIntra(pics[i].type) && running <= frame_threads + leafCap && refsStarted(i)) take(i, X265AMD_LAUNCH_AHEAD_LEAF);
    }
    *num_start = n;
    return X265AMD_OK;
}
