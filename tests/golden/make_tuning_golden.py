#!/usr/bin/env python3
"""Generates tuning_table.json: what rs_set_tuning of a GIVEN BUILD of the library answers (data only).

  RINGSNARK_AMD_LIB=<librs_hip.so of the commit to characterise> python tests/golden/make_tuning_golden.py

The committed fixture was taken from the release library of the last commit whose rs_set_tuning was the hand-written
if-chain, so that tests/test_tuning.py pins the table of csrc/tuning.hpp to that behaviour.  That library has no getter, so
the library is asked only for the STATUS of every (key, value); the default and the value stored after an accepted set are
written down here from the chain's assignments (`rule` below) and checked by the test against rs_get_tuning.
The library is opened with ctypes alone: ringsnark_amd._lib binds symbols an older build does not export.
"""
import ctypes
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.environ.get("RINGSNARK_AMD_LIB", os.path.join(ROOT, "ringsnark_amd", "librs_hip.so"))

VALUES = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15, 20, 21, 63, 64, 1 << 20]
STORED = {"any": lambda v: v, "checked": lambda v: v, "bool": lambda v: 1 if v else 0, "min1": lambda v: max(1, v)}
# key, default, what an ACCEPTED set stores ("checked": some values are rejected, the others stored as given)
KNOBS = [
    ("ntt_variant", 14, "any"), ("force_int_arith", 0, "bool"), ("mac_variant", 5, "any"), ("mac_ct_temporal", 0, "bool"),
    ("plain_variant", 1, "any"), ("prover_lin_io", 1, "any"), ("msm_host_tile", 1024, "min1"), ("msm_c_mib", 2048, "checked"),
    ("mac_chunk_units", 768, "min1"), ("mac_share_keys", 1, "bool"), ("ntt_wide_grid", 256, "min1"), ("int_ntt_variant", 1, "any"),
    ("witness_sub_log", 12, "checked"), ("witness_h_coset", 1, "bool"), ("witness_sub12_cross", 4, "checked"),
    ("witness_cross_pair", 1, "bool"), ("witness_cross_maxr", 6, "checked"), ("witness_force_bc", 0, "checked"),
    ("witness_bc2", 1, "bool"), ("witness_inc", 1, "bool"), ("witness_tree_log", 14, "checked"), ("witness_sub_ct", 2, "checked"),
    ("witness_tree_ct", 2, "any"), ("witness_tree_fwd", 0, "bool"), ("witness_level_turn", 1, "bool"), ("witness_h_turn", 1, "bool"),
    ("witness_tree_once", 1, "bool"), ("witness_big_ws_mib", 6144, "checked"), ("witness_col_budget_mib", 16384, "checked"),
    ("witness_lds_logM", 13, "checked"),
]
EXPERIMENTS = [("ntt_repeat", 1, "any")]  # key of the experiments build only: unknown to the release library
UNKNOWN = "no_such_knob"


def main():
    lib = ctypes.CDLL(LIB)
    lib.rs_set_tuning.restype = ctypes.c_int
    lib.rs_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_int]
    keys = {}
    for experiments, knobs in ((False, KNOBS), (True, EXPERIMENTS)):
        for key, default, rule in knobs:
            status = [lib.rs_set_tuning(key.encode(), v) for v in VALUES]
            keys[key] = {"default": default, "experiments": experiments, "status": status,
                         "stored": [STORED[rule](v) if st == 0 else None for v, st in zip(VALUES, status)]}
    out = {"values": VALUES, "keys": keys,
           "unknown_key": {"name": UNKNOWN, "status": [lib.rs_set_tuning(UNKNOWN.encode(), v) for v in VALUES]}}
    with open(os.path.join(HERE, "tuning_table.json"), "w") as f:
        f.write("{\n \"values\": %s,\n \"unknown_key\": %s,\n \"keys\": {\n" % (json.dumps(VALUES), json.dumps(out["unknown_key"])))
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(e)) for k, e in keys.items()))
        f.write("\n }\n}\n")
    print("wrote tuning_table.json: %d keys from %s" % (len(keys), LIB))


if __name__ == "__main__":
    main()
