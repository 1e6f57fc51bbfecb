#!/usr/bin/env python3
"""How well the subtraction in the I/Q samples cancels a signal whose waveform is known, on the CPU (no GPU needed): single-signal
frames from the oracle's synthesiser with f0 and the start sample uniform off the grid, without noise, at 0 dB and at -18 dB;
decoded by the oracle, refined by tests/ft8_spec_refine.py, subtracted by tests/ft8_spec_subtract.py.  Per set the median and
the worst case of 10 log10(|x' - (x - s)|^2 / |s|^2), s being the synthesiser's own noiseless waveform.
tests/test_subtract_cpu.py asserts the same on fewer frames of other seeds.
--waveform gfsk synthesises the same signals pulse-shaped (tests/ft8_spec_gfsk.py, through tools/gfsk_effect.waveform); --shape
selects the reference the signal is subtracted with (tests/ft8_spec_subtract_gfsk.py; several shapes give one row per set and
shape, on the same frames).  tests/test_subtract_gfsk_cpu.py holds the GFSK reference to the GFSK document.

  python tools/subtract_accuracy.py [--json profiles/subtract_accuracy.json] [--frames 64]
  python tools/subtract_accuracy.py --waveform gfsk --shape 0 1 --json profiles/subtract_gfsk_accuracy.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--waveform", choices=("cpfsk", "gfsk"), default="cpfsk")
    ap.add_argument("--shape", type=int, choices=(0, 1), nargs="+", default=[0])
    args = ap.parse_args()
    import numpy as np
    import oracle_lib
    import ft8_spec_subtract_gfsk as sg
    import subtract_craft as sc
    from gfsk_effect import waveform
    oracle_lib.build()
    oracle_lib.lib()
    out = {"what": "residual of the cancellation against subtracting the truth, dB (tools/subtract_accuracy.py)",
           "frames_per_set": args.frames, "grid_alone_db": -19.0, "sets": []}
    plain = args.waveform == "cpfsk" and args.shape == [0]              # the document this tool has always written
    if not plain:
        out["waveform"] = args.waveform
    for name, snr, seed in (("noiseless", None, 1), ("0dB", 0.0, 2), ("-18dB", -18.0, 3)):
        with waveform(args.waveform):
            iq, s, _f0, _start = sc.suppression_frames(oracle_lib, args.frames, snr, seed)
        for shape in args.shape:
            with sg.rule(shape):
                db = sc.suppression_db(oracle_lib, iq, s, nthreads=args.threads)
            row = {"set": name, "snr_db": snr, "decoded": int(len(db)), "median_db": round(float(np.median(db)), 2),
                   "p90_db": round(float(np.percentile(db, 90)), 2), "worst_db": round(float(db.max()), 2)}
            out["sets"].append(row if plain else dict(row, shape=shape, reference=("cpfsk", "gfsk")[shape]))
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
