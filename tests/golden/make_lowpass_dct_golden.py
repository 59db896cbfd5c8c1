#!/usr/bin/env python3
"""Golden data of the low-pass transform (--lowpass-dct) FROM THE REFERENCE ITSELF, below the encoder.

  tests/golden/lowpass_dct_golden.npz
      prim<depth>/<name>/<cu>/in, /out    the reference's own cu[].lowpass_dct (lowpassdct.cpp:34-112) on the inputs of lowpass_dct_lib.prim_inputs
      <set><depth>/<member>               transform units through the reference's own Quant (oracle/refprims.cpp: ref_tu_chain_batch, ref_intra_tu_chain_batch) with the
                                          reference's global `primitives` table switched by the reference's own enableLowpassDCTPrimitives (primitives.cpp:75-86),
                                          called by its mangled name on that table.  Sets: inter (plain quantisation), intra, intra_rdoq.

The table object and the function are reached from ctypes by their mangled names in oracle/_ref/librefprims<depth>.so; the slot numbers, which the script needs to call
the lowpass_dct slots themselves and to put the two dct slots back afterwards (from the standard_dct copies the function makes), come from
x265-amod_amd/host/primitive_table.h (a four-line program compiled against it prints them).  Asserted before anything is written: every lowpass_dct output equals the numpy restatement
(lowpass_dct_lib.lowpass_model) over the reference's dct of half the size; the 8x8 and 4x4 units of every set equal the unswitched table's results; among the 16x16 and
32x32 units of every set some differ from them; the first coefficients of the wraps are the numbers the restatement names.

Reads only oracle/_ref (oracle/build_ref.sh); the output is committed.  Usage: make_lowpass_dct_golden.py
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hevc_testlib as T
import lowpass_dct_lib as LP

TABLE = "_ZN4x26510primitivesE"         # x265::primitives (both depths: one namespace per library file)
ENABLE = "_ZN4x26526enableLowpassDCTPrimitivesERNS_17EncoderPrimitivesE"


def slot_numbers():
    src = '#include "primitive_table.h"\n#include <stdio.h>\nusing namespace x265amd;\nint main() { for (int cu = 0; cu < 5; cu++) printf("%d %d %d\\n", slotCU(cu, CU_dct), ' \
          'slotCU(cu, CU_standard_dct), slotCU(cu, CU_lowpass_dct)); printf("%d\\n", (int)TOTAL_SLOTS); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.cpp"), "w").write(src)
        subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(T.PKG_DIR, "host"), "-o", os.path.join(d, "s"), os.path.join(d, "s.cpp")])
        lines = subprocess.check_output([os.path.join(d, "s")], text=True).split("\n")
    return [tuple(int(v) for v in l.split()) for l in lines[:5]], int(lines[5])


class Switched:
    """enableLowpassDCTPrimitives on the reference's table, for a `with` block"""
    def __init__(self, lib, tab, slots):
        self.lib, self.tab, self.slots = lib, tab, slots

    def __enter__(self):
        for cu in (2, 3):
            assert self.tab[self.slots[cu][2]] and self.tab[self.slots[cu][0]] != self.tab[self.slots[cu][2]], "cu[%d].lowpass_dct is not set up, or is active already" % cu
        getattr(self.lib, ENABLE)(C.byref(self.tab))
        for cu in (2, 3):
            assert self.tab[self.slots[cu][0]] == self.tab[self.slots[cu][2]] and self.tab[self.slots[cu][1]]
        for cu in (0, 1):
            assert self.tab[self.slots[cu][0]] == self.tab[self.slots[cu][1]] != self.tab[self.slots[cu][2]]

    def __exit__(self, *exc):
        for cu in (2, 3):
            self.tab[self.slots[cu][0]] = self.tab[self.slots[cu][1]]
        return False


def differs(a, b):
    return any(not np.array_equal(np.asarray(x).ravel(), np.asarray(y).ravel()) for x, y in zip(a, b))


def make():
    slots, total = slot_numbers()
    out = {}
    for depth in (8, 10):
        R = T.load_ref(depth)
        inter = LP.inter_cases(depth)
        sets = {"intra": LP.intra_cases(depth, False), "intra_rdoq": LP.intra_cases(depth, True)}
        # the unswitched results first: they also set the reference's table up
        plain = {"inter": LP.tu_run_ref(R, inter)}
        for name, cases in sets.items():
            plain[name] = T.intra_tu_run_host(R, cases)
        tab = (C.c_void_p * total).in_dll(R.lib, TABLE)
        for cu in range(4):
            assert tab[slots[cu][0]], "cu[%d].dct" % cu
        with Switched(R.lib, tab, slots):           # (the lowpass_dct slots call through the standard_dct copies, which exist from the first switch on)
            pass

        # ---- the slots themselves ----
        def dct_half_of(cu):
            def f(avg):
                d = np.zeros(avg.shape, np.int16)
                R.call("dct", cu - 1, avg, d, avg.shape[1])
                return d
            return f
        for name, cu, stride, src in LP.prim_inputs(depth):
            N = 4 << cu
            fn = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t)(tab[slots[cu][2]])
            dst = np.full(N * N, 0x55AA, np.uint16).view(np.int16)
            src = np.ascontiguousarray(src)
            fn(src.ctypes.data, dst.ctypes.data, stride)
            want = LP.lowpass_model(src, cu, dct_half_of(cu))
            assert np.array_equal(dst.reshape(N, N), want), (depth, name, cu)
            out[LP.prim_key(depth, name, cu) + "/in"] = src
            out[LP.prim_key(depth, name, cu) + "/out"] = dst.copy()
        if depth == 10:
            for cu in (1, 2, 3):
                assert out[LP.prim_key(10, "pos_max", cu) + "/out"][0] == -128 and out[LP.prim_key(10, "neg_max", cu) + "/out"][0] == 128
            assert out[LP.prim_key(10, "mean256", 2) + "/out"][0] == -32768 and out[LP.prim_key(10, "mean256_less", 2) + "/out"][0] == 32767

        # ---- transform units with the table switched ----
        with Switched(R.lib, tab, slots):
            got = {"inter": LP.tu_run_ref(R, inter)}
            for name, cases in sets.items():
                got[name] = T.intra_tu_run_host(R, cases)
        again = LP.tu_run_ref(R, inter)
        assert not differs([r for t in again for r in t], [r for t in plain["inter"] for r in t]), "the table was not put back"
        for name, cases in dict(sets, inter=inter).items():
            big = [i for i, c in enumerate(cases) if c["log2"] >= 4]
            for i, c in enumerate(cases):
                if c["log2"] < 4:
                    assert not differs(got[name][i], plain[name][i]), "%s %d: unit %d (%dx%d) changed with the table" % (name, depth, i, 1 << c["log2"], 1 << c["log2"])
            changed = [i for i in big if differs(got[name][i], plain[name][i])]
            # (a unit whose residual quantises to nothing under both transforms cannot differ: a quarter of hevc_testlib.tu_cases are of that kind)
            assert len(changed) >= 8, "%s %d: only %d of %d large units differ from the plain table's" % (name, depth, len(changed), len(big))
            for size, plane in ((5, 0), (4, 0), (4, 1), (4, 2)):
                assert any(cases[i]["log2"] == size and cases[i]["ttype"] == plane for i in changed), (name, depth, size, plane)
            names = LP.INTER_NAMES if name == "inter" else LP.INTRA_NAMES
            for member, a in LP.flat(got[name], names).items():
                out["%s%d/%s" % (name, depth, member)] = a
            print(name, depth, "units", len(cases), "large", len(big), "changed by the option", len(changed), flush=True)
        psy = [c for c in sets["intra_rdoq"] if c["log2"] >= 4 and c["ttype"] == 0 and c["psyrdoq"]]
        assert len(psy) >= 4, "psy-RDOQ among the large luma units"
    np.savez_compressed(LP.GOLDEN, **out)
    print(LP.GOLDEN, os.path.getsize(LP.GOLDEN), "bytes")


if __name__ == "__main__":
    make()
