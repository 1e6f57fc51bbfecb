#!/usr/bin/env python3
"""Regenerates tests/golden/match_constructed.npz: the constructed frames of tests/match_craft.py (tables, candidates,
fabricated status records, waterfalls) and what the restatement tests/ft8_spec_match.py answers under every configuration.

usage: python tests/golden/make_match_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import match_craft as mc          # noqa: E402
import oracle_lib as oracle       # noqa: E402


def main():
    oracle.build()
    oracle.lib()
    cases = mc.build_cases(oracle)
    cfgs = mc.configs(cases)
    placed = mc.place(cases)
    want = mc.expected(oracle, placed, cfgs)
    names = sorted(placed["where"])
    out = dict(mag=placed["mag"], cands=placed["cands"].view(np.uint8), counts=placed["counts"], status_in=placed["status_in"],
               states=placed["states"].view(np.uint8), names=np.array(names), slots=np.array([placed["where"][n] for n in names], np.int32),
               frame_names=np.array([fr["name"] for fr in cases]),
               config_names=np.array([c[0] for c in cfgs]), config_max_age=np.array([c[1] for c in cfgs], np.int64),
               config_gate=np.array([c[2] for c in cfgs], np.int32))
    for name, _age, _gate in cfgs:
        status, info = want[name]
        out["status_" + name] = status
        out["info_" + name] = info.view(np.uint8)
    np.savez_compressed(mc.GOLDEN, **out)
    print(mc.GOLDEN, os.path.getsize(mc.GOLDEN), "bytes,", len(cases), "frames,", len(names), "candidates,", len(cfgs), "configurations")


if __name__ == "__main__":
    main()
