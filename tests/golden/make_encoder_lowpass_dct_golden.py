#!/usr/bin/env python3
"""Golden data of --lowpass-dct through the encoder FROM THE REFERENCE ITSELF.

  tests/golden/encoder_lowpass_dct_golden.json  stream md5 + length and the md5 of every reconstructed picture of oracle/_ref/x265_ref{8,10} for the command lines of
                                                tests/test_encoder_lowpass_dct.py, in the record layout of encoder_sao_options_golden.json; and per case the md5 of the
                                                reference's stream for the same line WITHOUT --lowpass-dct, which this script ASSERTS differs from the case's stream:
                                                the case then cannot be met with the option ignored.

Asserted before anything is written, too: a repeat of the first case is identical.

Reads only oracle/_ref (oracle/build_ref.sh); the output is committed.  Usage: make_encoder_lowpass_dct_golden.py
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
import test_encoder_lowpass_dct as EE
from test_encoder_sao_options import write_y4m


def reference_encode(d, depth, cli, out_name, recon=None):
    exe = os.path.join(T.REF_DIR, "x265_ref%d" % depth)
    cmd = [exe, "--input", "clip.y4m", "-o", out_name] + (["--recon", recon] if recon else []) + cli
    r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=7200)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(d, out_name), "rb").read()


def make_encoder():
    out, plain_seen, streams = {}, {}, {}
    for tag, ((w, h), nframes, depth, clip, cli) in EE.CASES.items():
        with tempfile.TemporaryDirectory() as d:
            write_y4m(os.path.join(d, "clip.y4m"), EE.case_frames(tag), w, h, depth)
            t0 = time.time()
            stream = reference_encode(d, depth, cli + T.PRESET_CLI, "out.hevc", "rec.yuv")
            seconds = round(time.time() - t0, 1)
            fsz = w * h * 3 // 2 * (2 if depth == 10 else 1)
            rec = np.fromfile(os.path.join(d, "rec.yuv"), np.uint8)
            assert len(rec) == fsz * nframes
            plain = EE.plain_cli(cli)
            key = (w, h, nframes, depth, clip, tuple(plain))
            if key not in plain_seen:
                plain_seen[key] = reference_encode(d, depth, plain + T.PRESET_CLI, "plain.hevc")
                if not out:
                    assert reference_encode(d, depth, cli + T.PRESET_CLI, "again.hevc") == stream, "the reference's stream is not repeatable"
            assert plain_seen[key] != stream, "%s: the reference's stream without %s is the case's own: lengthen the clip" % (tag, EE.OPT)
            streams[tag] = stream
            out[tag] = {"stream_md5": hashlib.md5(stream).hexdigest(), "stream_bytes": len(stream),
                        "recon_md5": [hashlib.md5(rec[k * fsz:(k + 1) * fsz].tobytes()).hexdigest() for k in range(nframes)],
                        "plain_stream_md5": hashlib.md5(plain_seen[key]).hexdigest(), "plain_command_line": " ".join(plain + T.PRESET_CLI),
                        "reference_command_line": " ".join(cli + T.PRESET_CLI), "reference_seconds": seconds}
            print(tag, out[tag], flush=True)
    with open(EE.GOLD_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    make_encoder()
