"""Layer 2 of the C ABI as include/x265amd.h documents it: x265amd_run_jobs with real batches.

The per-slot shims (csrc/slot_shims.hip), and with them tests/test_hip_parity.py, launch one job at a time on operands repacked to stride == width in a
256-byte-aligned arena.  Here a family's jobs run as batches of 1, 3, 4 and 5 (a lone wave, a partial block, a full block, a block and a tail) and as one large shuffled
batch whose blocks mix ops and sizes, on operands that stay where a host loop would have them: shared source planes read at odd element offsets with strides of the
block width, the width plus a padding, or an odd value; a disjoint output region per job.  Both arenas exist on the host and on the device byte for byte
(hevc_testlib.JobArena): the oracle's orc_* calls run on the host copy, the kernels on the device copy, and the WHOLE output arena is compared -- every block right,
nothing written outside one, nothing left unwritten.  Integer paths: the tolerance is zero.  Before a launch every address range a record lets a kernel touch is checked
on the host against the arenas (hevc_testlib.job_touch), so no wild address can reach the GPU."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import hevc_testlib as T

FAMILIES = range(T.JOB_FAMILIES)


def _header():
    with open(os.path.join(T.ROOT, "include", "x265amd.h")) as f:
        return f.read()


def test_job_record_layout():
    """the numpy dtype is x265amd_job: 96 bytes, every field where the C compiler puts it"""
    assert T.JOB_DT.itemsize == 96
    checks = ["static_assert(sizeof(x265amd_job) == 96, \"size\");"]
    for name in T.JOB_DT.names:
        checks.append("static_assert(offsetof(x265amd_job, %s) == %d, \"%s\");" % (name, T.JOB_DT.fields[name][1], name))
    src = "#include <stddef.h>\n#include \"x265amd.h\"\n" + "\n".join(checks) + "\n"
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(T.ROOT, "include"), "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_job_ops_match_header():
    """JOB_OPS restates enum x265amd_op: same names, same values, 46 ops, and a coverage figure for each"""
    body = re.search(r"enum x265amd_op\s*\{(.*?)\};", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want, nxt = {}, 0
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        m = re.fullmatch(r"X265AMD_OP_(\w+)(?:\s*=\s*(\d+))?", item)
        assert m, item
        nxt = int(m.group(2)) if m.group(2) else nxt
        want[m.group(1)] = nxt
        nxt += 1
    assert want == T.JOB_OPS
    assert len(T.JOB_OPS) == 46 and set(T.JOB_COVERAGE) == set(T.JOB_OPS)
    assert {v // 32 for v in T.JOB_OPS.values()} == set(FAMILIES)
    for op in T.JOB_OPS:
        assert hasattr(T.JobArena, "j_" + op.lower()), "no builder for " + op


def _assert_coverage(family, specs):
    """every (op, size index, filter phase) of the family is among the jobs: distinct keys per op against the enumeration (hevc_testlib.JOB_COVERAGE)"""
    got = T.job_coverage(specs)
    want = {op: n for op, n in T.JOB_COVERAGE.items() if T.JOB_OPS[op] // 32 == family}
    assert got == want
    if family == 4:
        assert len(specs) == sum(want.values()) == 2318       # every triple exactly once


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("family", FAMILIES)
def test_job_builders_on_the_host(family, depth):
    """without a GPU: the builders cover the enumeration, every record stays inside the arenas, and the oracle writes exactly the ranges job_touch says the
    kernels write (so the whole-arena comparison on the GPU holds the kernels to the same ranges)"""
    L = T.load_oracle(depth)
    A = T.job_family_specs(L, family, "random", 0)
    _assert_coverage(family, A.specs)
    in_base, out_base = 1 << 32, 1 << 40
    recs = T.job_records(A.specs, in_base, out_base)
    T.job_assert_inside(recs, A.specs, depth, in_base, A.inb.size, out_base, A.out_size)
    kept = A.inb.copy()
    want = T.job_expected(L, A, A.specs)
    assert np.array_equal(kept, A.inb)
    written = np.zeros(A.out_size, bool)
    for lo, hi, _ in T.job_regions(A, A.specs, depth):
        assert not written[lo:hi].any()
        written[lo:hi] = True
    assert np.array_equal(want[~written], A.poison()[~written]), "the oracle wrote outside the ranges job_touch gives"
    # ... and a whole-arena comparison names the job: one flipped byte inside a job's output, one in the gap behind it
    lo, hi, i = T.job_regions(A, A.specs, depth)[len(A.specs) // 2]
    for at, text in ((lo, "inside the output of job %d " % i), (hi, "OUTSIDE every job's output")):
        bad = want.copy()
        bad[at] ^= 0xFF
        with pytest.raises(AssertionError, match=re.escape(text)):
            T.job_compare(A, A.specs, depth, bad, want, "self-check")


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("family", FAMILIES)
def test_job_batches(family, depth):
    """per mode one large shuffled batch holding every (op, size index, filter phase) of the family; in random mode also on a non-default stream and as batches of
    1, 3, 4 and 5 jobs"""
    import torch
    hip, orc = T.load_hip(depth), T.load_oracle(depth)
    assert hip.lib.x265amd_device_count() >= 1, "no GPU visible: the HIP path must not silently fall back"
    launched = []
    for mode in T.MODES:
        A = T.job_family_specs(hip, family, mode, 0)
        want = T.job_expected(orc, A, A.specs)          # once per arena: the NULL-stream and the other-stream run share it
        what = "family %d depth %d %s" % (family, depth, mode)
        got = T.job_run_device(hip, A, A.specs, family)
        T.job_compare(A, A.specs, depth, got, want, what + ", %d jobs, NULL stream" % len(A.specs))
        _assert_coverage(family, A.specs)
        launched += A.specs
        if mode != "random":
            continue
        got = T.job_run_device(hip, A, A.specs, family, stream=torch.cuda.Stream())
        T.job_compare(A, A.specs, depth, got, want, what + ", %d jobs, non-default stream" % len(A.specs))
        for n in (1, 3, 4, 5):          # a lone wave, a partial block, a full block, a block plus a tail
            some = T.job_mixed_head(A.specs[n * 7:], n)
            assert len(some) == n
            got = T.job_run_device(hip, A, some, family)
            T.job_compare(A, some, depth, got, T.job_expected(orc, A, some), what + ", batch of %d" % n)
    assert collections.Counter(s.op // 32 for s in launched) == {family: len(launched)}
