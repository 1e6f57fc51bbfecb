"""Writes tests/golden/ap_constructed.npz: the constructed cases of tests/ap_craft.py as integer soft bits with their placements
(the waterfalls are rebuilt by osd_craft.waterfalls), fabricated status records, the configurations (hypothesis tables and
gates) and what tests/ft8_spec_ap.py makes of them at 20 iterations: the info records, and the status records AP rewrote as
(frame, slot) and 48 bytes each -- every other record is status_in's.  Frozen: the CPU test holds the restatement to it,
the GPU test the device.

  python tests/golden/make_ap_constructed_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    import oracle_lib
    import ft8_spec_ap as sa
    import ap_craft as ac
    import osd_craft as oc
    oracle_lib.build()
    cases, frames, mag, configs = ac.build(oracle_lib, seed=0x601D)
    out = dict(vectors=oc.vectors_of(cases), names=np.array([c["name"] for c in cases]), cands=frames["cands"].view(np.uint8),
               counts=frames["counts"], status_in=frames["status_in"], vec=frames["vec"],
               time_offsets=np.array([c.get("time_offset", -1000) for c in cases], np.int16),
               configs=np.array([name for name, _, _ in configs]), gates=np.array([gate for _, _, gate in configs], np.int32))
    for name, hyps, gate in configs:
        st, info = sa.ap_candidates(oracle_lib, mag, frames["cands"], frames["counts"], frames["status_in"], hyps, gate,
                                    status_out=frames["status_in"], iters=ac.ITERS)
        hit = np.argwhere((st != frames["status_in"]).any(axis=2))        # the records AP rewrote; every other one is status_in's
        assert np.array_equal(hit, np.argwhere(info["result"] == 1))
        out[f"hyps_{name}"] = ac.hyps_array(hyps).view(np.uint8)
        out[f"rewritten_{name}"] = hit.astype(np.int16)
        out[f"status_{name}"] = st[hit[:, 0], hit[:, 1]]
        out[f"info_{name}"] = info.view(np.uint8)
    np.savez_compressed(os.path.join(HERE, "ap_constructed.npz"), **out)


if __name__ == "__main__":
    main()
