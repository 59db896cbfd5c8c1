#!/usr/bin/env python3
"""Golden data of the picture ingest path FROM THE REFERENCE ITSELF.

  tests/golden/ingest_golden.npz            what the reference library's own x265_dither_image (oracle/_ref/libx265_ref8.so towards 8 bits, libx265_ref10.so towards 10)
                                            leaves of the pictures of tests/test_ingest.py: every plane's bytes and the error row
  tests/golden/encoder_ingest_golden.json   stream md5 + length and the md5 of every reconstructed picture of oracle/_ref/x265_ref{8,10} for the command lines of
                                            tests/test_encoder_ingest.py, in the record layout of encoder_me_full_golden.json

The generator ASSERTS what the tests build on: the 16-bit MSB-aligned raw form of the 10-bit clip gives the stream of the 10-bit clip itself (into the 10-bit reference)
and of the 10-bit clip under -D 8 (into the 8-bit reference); the luma bounds and the dither change the stream.

Reads only oracle/_ref (oracle/build_ref.sh); the outputs are committed.  Usage: make_ingest_golden.py [dither] [encoder]
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hevc_testlib as T
import test_ingest as TI
import test_encoder_ingest as EI


def make_dither_golden():
    out = {}
    for case in TI.dither_cases():
        kind, w, h, depth, target = case
        bufs, errors = TI.dither_call(TI.reference_dither(target), TI.dither_input(kind, w, h, depth), w, h, depth, target)
        for k in range(3):
            out[TI.dither_key(*case) + "/plane%d" % k] = bufs[k].copy()
        out[TI.dither_key(*case) + "/errors"] = errors
    np.savez_compressed(TI.GOLD_PATH, **out)
    print("wrote ingest_golden.npz with", len(out), "arrays")


def make_encoder_ingest_golden():
    out = {}
    for tag, (ref_depth, _, _, cli) in EI.CASES.items():
        cli = cli + T.PRESET_CLI
        with tempfile.TemporaryDirectory() as d:
            name = EI.write_input(d, tag)
            exe = os.path.join(T.REF_DIR, "x265_ref%d" % ref_depth)
            t0 = time.time()
            r = subprocess.run([exe, "--input", name, "-o", "out.hevc", "--recon", "rec.y4m"] + cli, cwd=d, capture_output=True, text=True, timeout=7200)
            assert r.returncode == 0, r.stderr[-2000:]
            rec = EI.read_recon(os.path.join(d, "rec.y4m"), ref_depth)
            stream = open(os.path.join(d, "out.hevc"), "rb").read()
            out[tag] = {"stream_md5": hashlib.md5(stream).hexdigest(), "stream_bytes": len(stream),
                        "recon_md5": [hashlib.md5(rec[k]).hexdigest() for k in range(EI.N)],
                        "reference_command_line": " ".join(cli), "reference_seconds": round(time.time() - t0, 1)}
            print(tag, out[tag], r.stderr.strip().splitlines()[-1])
    key = lambda t: (out[t]["stream_md5"], out[t]["stream_bytes"], out[t]["recon_md5"])
    for a, b in EI.SAME:
        assert key(a) == key(b), ("these two must be one stream", a, b)
    for a, b in EI.DIFFERENT:
        assert out[a]["stream_md5"] != out[b]["stream_md5"], ("these two must differ (bounds that do not bite?)", a, b)
    with open(EI.GOLD_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["dither", "encoder"]
    if "dither" in what:
        make_dither_golden()
    if "encoder" in what:
        make_encoder_ingest_golden()
