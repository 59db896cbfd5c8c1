"""The slot map the product uses to fill an EncoderPrimitives-shaped table (x265-amod_amd/host/primitive_table.h)
is checked against the reference's own header with offsetof static_asserts (tests/layout_check.cpp).  Needs
oracle/_ref/cfg and oracle/_ref/include (oracle/build_ref.sh: where the reference's sources are present)."""
import os
import subprocess

import pytest

import hevc_testlib as T

REF_SRC = os.path.join(T.REF_DIR, "include")      # the reference's source/ headers (oracle/build_ref.sh)


@pytest.mark.skipif(not (os.path.isdir(REF_SRC) and os.path.isdir(os.path.join(T.REF_DIR, "cfg"))), reason="needs oracle/_ref with the reference's headers (oracle/build_ref.sh)")
@pytest.mark.parametrize("depth", [8, 10])
def test_layout(depth, tmp_path):
    cmd = ["g++", "-std=gnu++17", "-fsyntax-only", "-w", "-Wno-invalid-offsetof",
           "-DX265_ARCH_X86=1", "-DX86_64=1", "-DHAVE_INT_TYPES_H=1", "-D__STDC_LIMIT_MACROS=1",
           "-DHIGH_BIT_DEPTH=%d" % (depth > 8), "-DX265_DEPTH=%d" % depth, "-DEXPORT_C_API=1", "-DX265_NS=x265",
           "-I" + os.path.join(T.REF_DIR, "cfg"), "-I" + REF_SRC, "-I" + REF_SRC + "/common",
           "-I" + os.path.join(T.PKG_DIR, "host"), os.path.join(T.ROOT, "tests", "layout_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
