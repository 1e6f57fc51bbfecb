#!/usr/bin/env python3
"""Accuracy of the refined time and frequency against known truth, on the CPU (no GPU needed): single-signal frames from the
oracle's synthesiser with f0 and the start sample uniform off the grid, at a strong level and near the threshold of belief
propagation; decoded by the oracle, refined by the restatement tests/ft8_spec_refine.py, estimated by the host helper
ft8gpu_refined_estimate.  tests/test_refine_cpu.py asserts the same on fewer frames.

  python tools/refine_accuracy.py [--json profiles/refine_accuracy.json] [--frames 256]

Per set: median and 90th percentile of the absolute error of freq_hz (Hz) and of the start time (samples of 1 / 3200 s), coarse
(the record's own values; dt_s also with the 256 samples from a row's first sample to its symbol's start added) and refined,
and the median refined snr_db beside the true SNR."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    import oracle_lib
    import refine_craft as rc
    oracle_lib.build()
    oracle_lib.lib()
    out = {"what": "refined against coarse freq_hz / dt_s on single-signal frames of known truth (tools/refine_accuracy.py)",
           "frames_per_set": args.frames, "units": {"hz": "Hz", "samples": "1/3200 s"}, "sets": {}}
    for name, snr, seed in (("strong", rc.STRONG_DB, 1), ("weak", rc.WEAK_DB, 2)):
        iq, f0, start, text = rc.accuracy_frames(oracle_lib, args.frames, snr, seed)
        s = rc.summary(rc.accuracy(oracle_lib, iq, f0, start, text, nthreads=args.threads))
        s["true_snr_db"] = snr
        out["sets"][name] = s
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
