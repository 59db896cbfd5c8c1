"""The start rule of the frame tasks as a host function (x265-amod_amd/host/launch_plan.cpp: x265amd_launch_plan, the function encoder_encode_impl itself calls) on lists
written out by hand.  No GPU: the function is host C++ and the library loads without a device.

A list is the prepared pictures in coding order, the first one collected next.  Per picture: type (X265_TYPE_*), whether later pictures reference it, started / finished,
and its reference pictures as places in the list (-1: already collected).  The function returns the places to start now, in order, and how each starts (in turn, an I
picture when typed, a referenced picture ahead of its turn, a leaf b picture ahead of its turn).

THE INVARIANT: no picture is returned whose reference is neither started (before, or earlier in the same answer) nor collected.  A task without that parks at its first CTU
with a frame slot, row fibers and a filter thread in its hands."""
import ctypes as C

import numpy as np
import pytest

import hevc_testlib as T

IDR, I, P, BREF, B = 1, 2, 3, 4, 5
IN_TURN, INTRA, AHEAD_REF, AHEAD_LEAF = 0, 1, 2, 3
MAX_REFS = 32
PIC_DT = np.dtype([("type", "<i4"), ("referenced", "<i4"), ("started", "<i4"), ("finished", "<i4"), ("num_refs", "<i4"), ("refs", "<i4", (MAX_REFS,))])


@pytest.fixture(scope="module")
def lib():
    L = T.load_hip(8).lib
    L.x265amd_launch_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.x265amd_launch_caps.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def caps(lib, ctu_h):
    a, b = C.c_int(-1), C.c_int(-1)
    assert lib.x265amd_launch_caps(ctu_h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


class Clip:
    """pictures in coding order as (poc, type, [pocs of the references]); `collected` of them are gone from the list, `started` / `finished` are sets of pocs"""

    def __init__(self, pics):
        self.pics = pics
        self.collected = 0
        self.admitted = len(pics)
        self.started, self.finished = set(), set()

    def live(self):
        return self.pics[self.collected:self.admitted]

    def running(self):
        return sum(1 for (poc, _, _) in self.live() if poc in self.started)

    def records(self):
        live = self.live()
        place = {poc: k for k, (poc, _, _) in enumerate(live)}
        rec = np.zeros(len(live), PIC_DT)
        for k, (poc, typ, refs) in enumerate(live):
            rec["type"][k] = typ
            rec["referenced"][k] = typ != B
            rec["started"][k] = poc in self.started
            rec["finished"][k] = poc in self.finished
            rec["num_refs"][k] = len(refs)
            rec["refs"][k, :len(refs)] = [place.get(r, -1) for r in refs]
            for r in refs:
                assert r in place or any(q[0] == r for q in self.pics[:self.collected]), "a reference is in the list or collected"
        return rec

    def plan(self, lib, frame_threads, ctu_h, frame_parallel=None, running=None):
        """one call; returns [(poc, how)] and checks what holds for every answer: places valid and distinct, nothing started twice, the invariant, and the caps"""
        rec = self.records()
        live = self.live()
        n = len(live)
        start, how = np.full(n + 1, -7, np.int32), np.full(n + 1, -7, np.int32)
        got = C.c_int(-1)
        fp = frame_threads > 1 if frame_parallel is None else frame_parallel
        run = self.running() if running is None else running
        rc = lib.x265amd_launch_plan(rec.ctypes.data if n else None, n, run, frame_threads, ctu_h, int(fp), start.ctypes.data, how.ctypes.data, C.byref(got))
        assert rc == 0 and 0 <= got.value <= n and start[n] == -7 and how[n] == -7
        ref_cap, leaf_cap = caps(lib, ctu_h)
        now = set()
        out = []
        for k in range(got.value):
            i, h = int(start[k]), int(how[k])
            assert 0 <= i < n and h in (IN_TURN, INTRA, AHEAD_REF, AHEAD_LEAF)
            poc, typ, refs = live[i]
            assert poc not in self.started and poc not in now, "started twice"
            for r in refs:
                assert r in self.started or r in now or all(q[0] != r for q in live), "poc %d starts before its reference %d" % (poc, r)      # THE INVARIANT
            if h == IN_TURN:
                assert i == 0 or run <= frame_threads
                assert all(q[0] in self.started or q[0] in now for q in live[:i]), "in turn means behind everything in front of it"
            elif h == INTRA:
                assert typ in (I, IDR) and fp
            elif h == AHEAD_REF:
                assert typ in (P, BREF) and fp and run <= frame_threads + ref_cap
            else:
                assert typ == B and fp and leaf_cap > 0 and run <= frame_threads + leaf_cap
            if h in (AHEAD_REF, AHEAD_LEAF):
                head = live[0]
                assert head[1] in (I, IDR) and (head[0] in self.started or head[0] in now) and head[0] not in self.finished, "ahead of its turn only behind a running I picture"
            now.add(poc)
            run += 1
            out.append((poc, h))
        return out


def bench_order():
    """the bench's coding order; a P picture references the three nearest earlier reference pictures, a B picture the two that enclose it"""
    return [(0, IDR, []), (4, P, [0]), (2, BREF, [0, 4]), (1, B, [0, 2]), (3, B, [2, 4]),
            (9, P, [4, 2, 0]), (7, BREF, [4, 9]), (6, B, [4, 7]), (8, B, [7, 9]),
            (14, P, [9, 7, 4]), (12, BREF, [9, 14]), (11, B, [9, 12]), (13, B, [12, 14]),
            (19, P, [14, 12, 9])]


def test_struct_layout_matches_the_header():
    assert PIC_DT.itemsize == 4 * (5 + MAX_REFS)


def test_a_the_chain_behind_a_running_i_picture(lib):
    """(a) I0 runs, frameThreads 5: the referenced B pictures start as links of the chain -- B7 before P14, B12 before P19 -- and the leaf b pictures by picture size"""
    c = Clip(bench_order())
    c.started = {0}
    got = c.plan(lib, 5, 17)
    assert got == [(4, IN_TURN), (2, IN_TURN), (1, IN_TURN), (3, IN_TURN), (9, IN_TURN), (7, AHEAD_REF), (14, AHEAD_REF), (12, AHEAD_REF), (19, AHEAD_REF)]
    order = [poc for poc, _ in got]
    assert order.index(7) < order.index(14) and order.index(12) < order.index(19)
    assert not [poc for poc, h in got[5:] if poc in (6, 8, 11, 13)], "1080p (17 CTU rows): no leaf b beyond the first frameThreads + 1"
    got34 = c.plan(lib, 5, 34)
    assert got34 == got + [(6, AHEAD_LEAF), (8, AHEAD_LEAF), (11, AHEAD_LEAF), (13, AHEAD_LEAF)], "2160p (34 CTU rows): the leaf b pictures behind the chain"
    # the I picture started in the same answer holds the head as well
    c.started = set()
    assert c.plan(lib, 5, 17) == [(0, IN_TURN)] + got
    # a finished head is collected next: nothing starts ahead of its turn any more
    c.started, c.finished = {0}, {0}
    assert c.plan(lib, 5, 17) == got[:5]


def test_a_a_reference_without_a_task_holds_its_picture_back(lib):
    """what the rule before this one did: P14 started while B7 had no task.  With B7 over the cap, P14 stays, too"""
    c = Clip(bench_order())
    ref_cap, _ = caps(lib, 17)
    c.started = {0}
    # as many running as lets exactly one more referenced picture start: B7 takes the place, P14 does not start without it
    got = c.plan(lib, 5, 17, running=5 + ref_cap)
    assert got == [(4, AHEAD_REF)]
    c.started = {0, 4, 2, 1, 3, 9}
    assert c.plan(lib, 5, 17, running=5 + ref_cap) == [(7, AHEAD_REF)]
    assert c.plan(lib, 5, 17, running=5 + ref_cap + 1) == []
    # B7 collected elsewhere is not the case; B7 started is: P14 goes
    c.started.add(7)
    assert c.plan(lib, 5, 17, running=5 + ref_cap) == [(14, AHEAD_REF)]


@pytest.mark.parametrize("ctu_h", [17, 34])
def test_b_every_prefix_of_collected_pictures(lib, ctu_h):
    """(b) the first k pictures collected, k = 0 .. 13: from nothing started, and along a whole run that collects one picture per call -- the invariant and the caps (checked
    in plan() for every answer) hold, and the first picture in coding order is returned whenever it has no task"""
    order = bench_order()
    for k in range(len(order)):
        c = Clip(order)
        c.collected = k
        c.started = c.finished = {q[0] for q in order[:k]}
        got = c.plan(lib, 5, ctu_h)
        assert got and got[0] == (order[k][0], IN_TURN)
        # ... and with everything running that may: the head still starts, alone unless it is an I picture
        got = c.plan(lib, 5, ctu_h, running=40)
        assert got == [(order[k][0], IN_TURN)]
    c = Clip(order)
    for k in range(len(order)):
        got = c.plan(lib, 5, ctu_h)
        if order[k][0] not in c.started:
            assert got and got[0] == (order[k][0], IN_TURN)
        c.started |= {poc for poc, _ in got}
        assert order[k][0] in c.started
        ref_cap, leaf_cap = caps(lib, ctu_h)
        assert c.running() <= 5 + 1 + max(ref_cap, leaf_cap)
        c.finished.add(order[k][0])
        c.collected = k + 1
    assert c.started == {q[0] for q in order}


def in_turn_rule(live_started, running, frame_threads, types, frame_parallel):
    """the launch loop as it stood before the rule was a function of its own, with no I picture running at the head: coding order while at most frame_threads run, the head
    always, I pictures when typed"""
    out = []
    for i, started in enumerate(live_started):
        if started:
            continue
        if running <= frame_threads or i == 0:
            out.append(i); running += 1
            continue
        if not frame_parallel:
            break
        if types[i] in (I, IDR):
            out.append(i); running += 1
    return out


def test_c_no_i_picture_at_the_head_is_the_in_turn_rule(lib):
    """(c) the head is a P picture (I0 collected): pictures start in turn and nothing else does, whatever the size.  Expected lists written out from the loop's logic"""
    order = bench_order()
    for ctu_h in (17, 34):
        c = Clip(order)
        c.collected = 1
        c.started = c.finished = {0}
        c.started = {0, 4}
        assert [p for p, _ in c.plan(lib, 5, ctu_h)] == [2, 1, 3, 9, 7]               # running 1 .. 5 when they start, the sixth finds 6 > 5
        c.started = {0, 4, 2, 1}
        assert [p for p, _ in c.plan(lib, 5, ctu_h)] == [3, 9, 7]
        assert [p for p, _ in c.plan(lib, 3, ctu_h)] == [3]                           # running 3 <= 3, then 4
        c.started = {0, 4, 2, 1, 3, 9, 7}
        assert c.plan(lib, 5, ctu_h) == []                                            # seven run: nobody's turn
        c.started = {0}
        assert c.plan(lib, 5, ctu_h, running=9) == [(4, IN_TURN)]                     # the head starts whatever runs
    # an I picture further back starts when it is typed, behind a P head as well, and brings nobody with it
    order2 = order[:9] + [(24, I, []), (14, P, [9, 7, 4]), (12, BREF, [9, 14])]
    c = Clip(order2)
    c.collected = 1
    c.started = {0, 4, 2, 1, 3, 9, 7}
    c.finished = {0}
    assert c.plan(lib, 5, 34) == [(24, INTRA)]
    # against the loop itself, over every started-prefix of every collected-prefix
    for k in range(1, len(order2)):
        for s in range(k, len(order2) + 1):
            c = Clip(order2)
            c.collected = k
            c.finished = {q[0] for q in order2[:k]}
            c.started = {q[0] for q in order2[:s]}
            live = c.live()
            if live[0][1] in (I, IDR) and live[0][0] in c.started:
                continue        # (the other rule's case)
            for ft in (2, 5):
                want = in_turn_rule([q[0] in c.started for q in live], c.running(), ft, [q[1] for q in live], True)
                if live[0][1] in (I, IDR):
                    continue    # an I head that starts now holds the head from this answer on
                assert [live.index(next(q for q in live if q[0] == p)) for p, _ in c.plan(lib, ft, 34)] == want, (k, s, ft)


def test_d_one_picture_at_a_time_without_frame_parallelism(lib):
    """(d) frameParallel off, or one frame thread: only in turn -- the caller waits for each task before it starts the next --, never ahead, I pictures included"""
    order = bench_order()[:9] + [(24, I, [])]
    for ft, fp in ((1, False), (1, True), (5, False)):
        c = Clip(order)
        seen = []
        for k in range(len(order)):
            got = c.plan(lib, ft, 34, frame_parallel=fp)
            assert all(h == IN_TURN for _, h in got) or (ft, fp) == (1, True)
            if not fp:
                assert all(h == IN_TURN for _, h in got)
                # exactly the next pictures in coding order, as many as bring the count to frame_threads + 1
                nxt = [q[0] for q in c.live() if q[0] not in c.started][:max(0, ft + 1 - c.running())]
                if order[k][0] not in c.started and not nxt:
                    nxt = [order[k][0]]
                assert [p for p, _ in got] == nxt
            seen += [p for p, _ in got]
            c.started |= {p for p, _ in got}
            c.finished.add(order[k][0])
            c.collected = k + 1
        if not fp:
            assert seen == [q[0] for q in order], "coding order"
    # one frame thread, list of pictures without an I picture behind the head: in turn even when the flag is on
    c = Clip(bench_order())
    assert [p for p, _ in c.plan(lib, 1, 34, frame_parallel=False)] == [0, 4]          # (0 and 1 running when they start: the caller has waited for the first)
    c.started = {0}
    assert c.plan(lib, 1, 34, frame_parallel=False) == [(4, IN_TURN)]
    c.started = {0, 4}
    assert c.plan(lib, 1, 34, frame_parallel=False) == []


def random_clip(rng):
    n = int(rng.integers(1, 25))
    pics = [(0, IDR, [])]
    for poc in range(1, n):
        r = rng.random()
        typ = I if r < 0.08 else P if r < 0.4 else BREF if r < 0.6 else B
        refs = []
        if typ not in (I, IDR):
            cand = [q[0] for q in pics if q[1] != B]
            m = int(rng.integers(1, min(4, len(cand)) + 1))
            refs = [int(x) for x in rng.choice(cand, m, replace=False)]
        pics.append((poc, typ, refs))
    return pics


def test_e_random_reference_graphs_never_deadlock(lib):
    """(e) 200 seeded graphs of at most 24 pictures, arriving a few at a time: start what the function returns, collect the head once it has a task (not always at once: a
    head that keeps running is when pictures start ahead of their turn).  Every picture gets its task and the run ends -- nobody waits for a picture without a task that
    only the waiting picture's collection would start"""
    rng = np.random.default_rng(20251)
    ahead = 0
    for _ in range(200):
        pics = random_clip(rng)
        ft = int(rng.integers(1, 7))
        ctu_h = int(rng.choice([4, 17, 34]))
        c = Clip(pics)
        c.admitted = 0
        for step in range(6 * len(pics) + 8):
            c.admitted = min(len(pics), c.admitted + int(rng.integers(0, 6)))
            if c.collected == c.admitted:
                if c.admitted == len(pics):
                    break
                continue
            head = c.live()[0][0]
            got = c.plan(lib, ft, ctu_h)
            c.started |= {p for p, _ in got}
            ahead += sum(1 for _, h in got if h in (AHEAD_REF, AHEAD_LEAF))
            assert head in c.started, "the first picture in coding order always has a task"
            if rng.random() < 0.6 or c.admitted == len(pics):
                c.finished.add(head)
                c.collected += 1
        assert c.collected == len(pics) and c.started == {q[0] for q in pics}, (pics, ft)
    assert ahead > 100, "the graphs do reach the rule under test"


def test_arguments_are_checked(lib):
    rec = Clip(bench_order()).records()
    start = np.zeros(len(rec), np.int32)
    got = C.c_int(0)
    call = lambda r, n, run, ft, h: lib.x265amd_launch_plan(r.ctypes.data, n, run, ft, h, 1, start.ctypes.data, None, C.byref(got))
    assert call(rec, len(rec), 0, 5, 17) == 0 and got.value == 10         # (no `how` array: allowed)
    assert call(rec, len(rec), 0, 0, 17) != 0 and call(rec, len(rec), -1, 5, 17) != 0 and call(rec, len(rec), 0, 5, 0) != 0
    bad = rec.copy(); bad["refs"][3, 0] = 3                               # a picture that references itself (or a later one) is no coding order
    assert call(bad, len(bad), 0, 5, 17) != 0
    bad = rec.copy(); bad["num_refs"][3] = MAX_REFS + 1
    assert call(bad, len(bad), 0, 5, 17) != 0
    assert lib.x265amd_launch_plan(None, 0, 0, 5, 17, 1, start.ctypes.data, None, C.byref(got)) == 0 and got.value == 0
