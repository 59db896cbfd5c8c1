#!/usr/bin/env python3
"""tests/golden/filter_edges_golden.json: per group of tests/test_filter_edges.py and bit depth the SHA-256 of the oracle's output over the group's cases (deblocking:
the padded planes of every case and pass selection; SAO: count, offsetOrg and the padded offset planes of every case).

With oracle/_ref built, the oracle's output is first ASSERTED equal to the reference's own Deblock / SAO classes (the level-1 tests), so that a digest is never
taken from an oracle the reference contradicts.  The output is committed; the same inputs give the same bytes."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hevc_testlib as T
import test_filter_edges as F


def main():
    out = {}
    for group in F.DB_GROUPS + tuple(sorted(F.SAO_GROUPS)):
        out[group] = {}
        for depth in (8, 10):
            if T.have_ref():
                (F.test_deblock_oracle_vs_reference if group.startswith("deblock") else F.test_sao_oracle_vs_reference)(depth, group)
            res = F.db_oracle(depth, group) if group.startswith("deblock") else F.sao_oracle(depth, group)
            out[group][str(depth)] = F.digest(group, res)
            print(group, depth, out[group][str(depth)], "checked against the reference" if T.have_ref() else "NOT checked against the reference (oracle/_ref not built)")
    with open(F.GOLD_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
