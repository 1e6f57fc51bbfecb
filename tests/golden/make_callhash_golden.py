"""Writes tests/golden/callhash_cases.npz: the constructed cases of tests/callhash_craft.py -- message records, counts, entry
slot counters and max_age -- with what tests/ft8_spec_callhash.py makes of them: the resolved records (on a prefill of
callhash_craft.JUNK bytes) and the exit states.  Frozen: the CPU test holds the craft module and the restatement to it, the
GPU test the device.

  python tests/golden/make_callhash_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    import oracle_lib
    import callhash_craft as cc
    oracle_lib.build()
    cases = cc.build_cases(oracle_lib)
    out = dict(names=np.array([c["name"] for c in cases]), max_age=np.array([c["max_age"] for c in cases], np.uint32))
    for c in cases:
        resolved, state = cc.expected(c)
        name = c["name"]
        out[f"msgs_{name}"] = c["msgs"].view(np.uint8)
        out[f"n_msgs_{name}"] = c["n_msgs"]
        out[f"slot0_{name}"] = c["state"]["slot"]
        out[f"resolved_{name}"] = resolved.view(np.uint8)
        out[f"state_{name}"] = state.view(np.uint8)
    np.savez_compressed(os.path.join(HERE, "callhash_cases.npz"), **out)


if __name__ == "__main__":
    main()
