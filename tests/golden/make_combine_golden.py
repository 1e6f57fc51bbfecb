#!/usr/bin/env python3
"""Regenerates tests/golden/combine_constructed.npz: the constructed frames of tests/combine_craft.py (memories, candidates,
fabricated status records, waterfalls) and what the restatement tests/ft8_spec_combine.py answers under every configuration:
the status and info records of ft8gpu_combine_candidates and the exit states of ft8gpu_softmem_update per store_per_slot.

usage: python tests/golden/make_combine_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import combine_craft as cc        # noqa: E402
import oracle_lib as oracle       # noqa: E402


def main():
    oracle.build()
    oracle.lib()
    cases = cc.build_cases(oracle)
    placed = cc.place(oracle, cases)
    want = cc.expected(oracle, placed)
    names = sorted(placed["where"])
    out = dict(mag=placed["mag"], cands=placed["cands"].view(np.uint8), counts=placed["counts"], status_in=placed["status_in"],
               states=placed["states"].view(np.uint8), names=np.array(names), slots=np.array([placed["where"][n] for n in names], np.int32),
               frame_names=np.array([fr["name"] for fr in cases]))
    for name, _age, _gate in cc.CONFIGS:
        status, info, after = want[name]
        out["status_" + name] = status
        out["info_" + name] = info.view(np.uint8)
        for s, st in after.items():
            out[f"after_{name}_{s}"] = st.view(np.uint8)
    np.savez_compressed(cc.GOLDEN, **out)
    print(cc.GOLDEN, os.path.getsize(cc.GOLDEN), "bytes,", len(cases), "frames,", len(names), "candidates,", len(cc.CONFIGS), "configurations")


if __name__ == "__main__":
    main()
