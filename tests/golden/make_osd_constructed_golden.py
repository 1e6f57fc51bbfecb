"""Writes tests/golden/osd_constructed.npz: the constructed cases a..h of tests/osd_craft.py and the first 24 vectors of its
random sweep as integer soft bits with their placements (the waterfalls are rebuilt by osd_craft.waterfalls), fabricated
status records, and what tests/ft8_spec_osd.py makes of them at orders 0, 1, 2 with the gates 83, 27, 20 and the gates on
both sides of case f's hard-error counts (the status records OSD rewrote, as (frame, slot) and 48 bytes each; every other
record is status_in's).  Frozen: the CPU test holds the restatement to it, the GPU test the device.
Also writes profiles/osd_constructed.json: what the full set of constructed cases reaches, by the restatement.

  python tests/golden/make_osd_constructed_golden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SWEEP = 24


def main():
    import oracle_lib
    import ft8_spec_osd as so
    import osd_craft as oc
    oracle_lib.build()
    every = oc.build_cases(oracle_lib)
    named = [c for c in every if c["case"] != "i"]
    cases = named + [c for c in every if c["case"] == "i"][:SWEEP]
    frames = oc.build_frames(cases, seed=0x601D)
    vectors = oc.vectors_of(cases)
    mag = oc.waterfalls(vectors, frames)
    searches = {}
    out = dict(vectors=vectors, names=np.array([c["name"] for c in cases]), cands=frames["cands"].view(np.uint8), counts=frames["counts"],
               status_in=frames["status_in"], vec=frames["vec"], configs=np.array(oc.CONFIGS, np.int32))
    for order, gate in oc.CONFIGS:
        st, info = so.osd_candidates(oracle_lib, mag, frames["cands"], frames["counts"], frames["status_in"], order, gate,
                                     status_out=frames["status_in"], searches=searches)
        hit = np.argwhere((st != frames["status_in"]).any(axis=2))        # the records OSD rewrote; every other one is status_in's
        assert np.array_equal(hit, np.argwhere(info["result"] == 1))
        out[f"rewritten_o{order}_g{gate}"] = hit.astype(np.int16)
        out[f"status_o{order}_g{gate}"] = st[hit[:, 0], hit[:, 1]]
        out[f"info_o{order}_g{gate}"] = info.view(np.uint8)
    np.savez_compressed(os.path.join(HERE, "osd_constructed.npz"), **out)

    frames = oc.build_frames(every)
    mag = oc.waterfalls(oc.vectors_of(every), frames)
    searches, infos = {}, {}
    for order, gate in oc.CONFIGS:
        infos[(order, gate)] = so.osd_candidates(oracle_lib, mag, frames["cands"], frames["counts"], frames["status_in"], order, gate,
                                                 searches=searches)[1]
    prof = dict(what="constructed soft bits for ft8gpu_osd_candidates (tests/osd_craft.py): what the cases reach, by the restatement "
                     "tests/ft8_spec_osd.py; tests/test_gpu_osd_constructed.py holds the device to the same records byte for byte",
                configs=[list(c) for c in oc.CONFIGS], **oc.tallies(oracle_lib, every, frames, mag, infos))
    with open(os.path.join(ROOT, "profiles", "osd_constructed.json"), "w") as fh:
        json.dump(prof, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
