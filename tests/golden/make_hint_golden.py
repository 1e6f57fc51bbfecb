"""Writes tests/golden/hint_constructed.npz: the constructed soft bits, placements, tables and parameters of
tests/hint_craft.py and what the restatement (tests/ft8_spec_hint.py, on the oracle's soft bits and bp_decode) makes of them --
the info records of every configuration and the status records it rewrites.  Nothing here comes from the device.
Run from the repository root after the oracle is built: python tests/golden/make_hint_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import hint_craft as hc                                   # noqa: E402
import oracle_lib                                         # noqa: E402
import osd_craft as oc                                    # noqa: E402


def main():
    oracle = oracle_lib
    cases, frames, mag, cfgs = hc.build(oracle)
    want = hc.expected(oracle, frames, mag, cfgs)
    d = dict(vectors=oc.vectors_of(cases), case_names=np.array([c["name"] for c in cases]), cands=frames["cands"].view(np.uint8),
             counts=frames["counts"], status_in=frames["status_in"], vec=frames["vec"], names=np.array([c[0] for c in cfgs]),
             states=np.concatenate([np.asarray(c[1]).view(np.uint8).reshape(1, -1) for c in cfgs]),
             params=np.array([c[2:] for c in cfgs], np.int64))
    for k, c in enumerate(cfgs):
        st, info = want[c[0]]
        hit = np.argwhere((st != frames["status_in"]).any(axis=2))
        d[f"info_{k}"] = info.view(np.uint8).reshape(info.shape[0], -1)
        d[f"rewritten_{k}"] = hit.astype(np.int32)
        d[f"status_{k}"] = st[hit[:, 0], hit[:, 1]]
        res = info["result"][np.arange(info.shape[1])[None, :] < frames["counts"][:, None]]
        print(f"{c[0]:40s} tries {c[2]} gate {c[3]:2d} hard {c[4]:3d}: results {dict(zip(*np.unique(res, return_counts=True)))}, "
              f"rewritten {len(hit)}")
    np.savez_compressed(hc.GOLDEN, **d)
    print(hc.GOLDEN, os.path.getsize(hc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
