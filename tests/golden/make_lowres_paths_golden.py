#!/usr/bin/env python3
"""Golden data of the lookahead frame cost's sliced, weighted and reuse paths FROM THE REFERENCE ITSELF.

  tests/golden/lowres_paths_golden.npz   <entry>/{lowres_costs, mvs, mv_costs, row_satds, slice_sums} for every entry of hevc_testlib.lowres_paths_specs(), and
                                         <scene>/intra_cost per scene: the reference's own CostEstimateGroup::estimateCUCost over Lowres objects made from the scenes'
                                         luma planes (oracle/refprims.cpp: ref_lowres_frame_cost_paths, in oracle/_ref/librefprims{8,10}.so), looped in cooperative slices
                                         as processTasks does, with the caller's bDoSearch, with weightsAnalyse's weighted planes of a given weight, and with the motion
                                         fields of an earlier entry copied in where a list is not searched.  The entries are computed in the table's order, so an entry that
                                         reuses a field reads what the reference itself found before.

Before it stores anything this script ASSERTS the conditions tests/test_lookahead_paths.py checks on the committed file (the sliced entries differ from the unsliced ones in
upper slices only, the weight changes the search, bi-prediction wins under the weight, every list wins somewhere in the reuse entries), so a seed for which they fail is noticed
here.  Reads only oracle/_ref (oracle/build_ref.sh); the output is committed.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hevc_testlib as T
import test_lookahead_paths as LP


if __name__ == "__main__":
    out = T.lowres_paths_compute_ref()
    LP.check_golden_conditions(out)
    np.savez_compressed(T.PATHS_GOLD, **out)
    print("wrote", T.PATHS_GOLD, len(out), "arrays,", os.path.getsize(T.PATHS_GOLD), "bytes")
