"""Writes tests/golden/osd_frame.npz: one crowded frame (20 CQ signals, seed 1003) as the oracle's stage outputs, and what
tests/ft8_spec_osd.py makes of its failing candidates at orders 0, 1, 2 with the gates 83, 27 and 20.  Frozen: the CPU
test holds the restatement to it, the GPU test the device.

  python tests/golden/make_osd_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CONFIGS = [(0, 83), (1, 83), (2, 83), (1, 27), (2, 27), (1, 20), (2, 20)]


def main():
    import oracle_lib
    import synth_util as S
    import ft8_spec_messages as sm
    import ft8_spec_osd as so
    oracle_lib.build()
    iq, _ = S.make_frame(1003, 20, S.oracle_encode_fn(oracle_lib), snr_range=(-22.0, 0.0))
    mag, cands, counts, status = sm.oracle_stages(oracle_lib, iq[None], 120, 10, 1)
    searches = {}
    out = dict(mag=mag, cands=cands.view(np.uint8), counts=counts, status_in=status, configs=np.array(CONFIGS, np.int32))
    for order, gate in CONFIGS:
        st, info = so.osd_candidates(oracle_lib, mag, cands, counts, status, order, gate, searches=searches)
        out[f"status_o{order}_g{gate}"] = st
        out[f"info_o{order}_g{gate}"] = info.view(np.uint8)
    np.savez_compressed(os.path.join(HERE, "osd_frame.npz"), **out)


if __name__ == "__main__":
    main()
