#!/usr/bin/env python3
"""Golden data of the SAO options (--sao-non-deblock, --limit-sao, --selective-sao) FROM THE REFERENCE ITSELF.

  tests/golden/encoder_sao_options_golden.json  stream md5 + length and the md5 of every reconstructed picture of oracle/_ref/x265_ref{8,10} for the command lines of
                                                tests/test_encoder_sao_options.py, in the record layout of encoder_rskip_edge_golden.json; and per case the md5 of the
                                                reference's stream for the same line WITHOUT the SAO option(s), which this script ASSERTS differs from the case's stream:
                                                the case then cannot be met with the option ignored.

Asserted before anything is written, too: --selective-sao 0 and --selective-sao 4 give the plain line's stream; --selective-sao 2 --no-sao gives the stream of
--selective-sao 2; a repeat of the first case is identical.

Reads only oracle/_ref (oracle/build_ref.sh); the output is committed.  Usage: make_sao_options_golden.py
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
import test_encoder_sao_options as EE


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
            EE.write_y4m(os.path.join(d, "clip.y4m"), EE.case_frames(tag), w, h, depth)
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
                # once per clip and line: --selective-sao 0 and 4 are the plain line; and (once) the reference repeats itself
                # (not 4 on a --no-sao line: any non-zero value switches SAO back on, which is the sel2_nosao case)
                for value in ("0",) if "--no-sao" in plain else ("0", "4"):
                    assert reference_encode(d, depth, plain + ["--selective-sao", value] + T.PRESET_CLI, "sel.hevc") == plain_seen[key], (tag, value)
                if not out:
                    assert reference_encode(d, depth, cli + T.PRESET_CLI, "again.hevc") == stream, "the reference's stream is not repeatable"
            assert plain_seen[key] != stream, "%s: the reference's stream without %s is the case's own: lengthen the clip" % (tag, " ".join(o for o in cli if o not in plain))
            streams[tag] = stream
            out[tag] = {"stream_md5": hashlib.md5(stream).hexdigest(), "stream_bytes": len(stream),
                        "recon_md5": [hashlib.md5(rec[k * fsz:(k + 1) * fsz].tobytes()).hexdigest() for k in range(nframes)],
                        "plain_stream_md5": hashlib.md5(plain_seen[key]).hexdigest(), "plain_command_line": " ".join(plain + T.PRESET_CLI),
                        "reference_command_line": " ".join(cli + T.PRESET_CLI), "reference_seconds": seconds}
            print(tag, out[tag], flush=True)
    assert streams["sel2_nosao/"] == streams["sel2/"], "--selective-sao 2 --no-sao is not --selective-sao 2"
    with open(EE.GOLD_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    make_encoder()
