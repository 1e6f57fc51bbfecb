#!/usr/bin/env python3
"""Cost of the wideband RX front end (ft8gpu_wide_frames, ft8gpu_decode_wide), measured on the GPU in one session, device
pointers: 16 captures of 36 000 000 pairs (the size of tools/bench_rx.py), uniform random bytes, on a context of 256 frames.

  python tools/bench_wide.py [--json profiles/wide_bench.json] [--steps 5] [--rounds 3] [--captures 16]

Arms, interleaved round by round: ft8gpu_wide_frames with 1, 2, 8 and 16 channels, ft8gpu_rx_decimate on the same bytes (the
one-channel read-once yardstick), ft8gpu_decode_wide with 16 channels and ft8gpu_decode_messages on the frames the 16-channel
stage left.  Time = events on the context's stream around `steps` calls, after two warm-up calls, best of `rounds`; every round's
figure is kept.  The capture bytes over the stage's time are set against the project's measured read-only ceiling of 6.2 .. 6.4
TB/s (profiles/README.md).  Reading the bytes once shows in the time at 8 channels against 8 times the time at 1 channel: the
ratio is 1 if every channel costs what the first does, and falls below 1 by what the channels share (the fetch of the bytes, the
staging in LDS, the launch).  A machine without a GPU fails at ft8gpu_create; nothing is estimated."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CEILING_TBS = (6.2, 6.4)
CHANNEL_COUNTS = (1, 2, 8, 16)
# sixteen dial offsets over +-1.1 MHz, in 6.25 Hz units: every c and q differs
BINS = tuple(int(-170000 + 22003 * k + 17 * k * k) for k in range(16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--captures", type=int, default=16)
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    ncap, npairs, nmax = args.captures, ft8.WIDE_MAX_PAIRS, max(CHANNEL_COUNTS)
    assert all(abs(b) <= ft8.WIDE_MAX_BIN for b in BINS)
    out = {"what": "cost of the wideband RX front end on one MI355X (tools/bench_wide.py)", "build_id": ft8.check_build_id(),
           "captures": ncap, "npairs": npairs, "capture_bytes": ncap * 2 * npairs, "freq_bins": list(BINS), "steps": args.steps,
           "rounds": args.rounds, "arms": {}}
    with ft8.Decoder(device=0, max_frames=ncap * nmax) as dec:
        stream = torch.cuda.ExternalStream(dec.stream_handle())
        gen = torch.Generator(device="cuda").manual_seed(1)
        raw = torch.randint(0, 256, (ncap, 2 * npairs), dtype=torch.uint8, device="cuda", generator=gen)
        iq = torch.empty((ncap * nmax, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        iq_rx = torch.empty((ncap, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        msgs = torch.zeros((ncap * nmax * 50 * 64,), dtype=torch.uint8, device="cuda")
        n_msgs = torch.zeros((ncap,), dtype=torch.int32, device="cuda")
        fm = torch.zeros((ncap * nmax * 50 * 64,), dtype=torch.uint8, device="cuda")
        fn = torch.zeros((ncap * nmax,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        arms = {f"wide_frames_{n}": (lambda n=n: dec.wide_frames_dev(raw, ncap, npairs, BINS[:n], iq, True)) for n in CHANNEL_COUNTS}
        arms["rx_decimate"] = lambda: dec.rx_decimate_dev(raw, ncap, npairs, iq_rx, True)
        arms["decode_wide_16"] = lambda: dec.decode_wide_dev(raw, ncap, npairs, BINS, msgs, n_msgs)
        arms["decode_messages"] = lambda: dec.decode_messages_dev(iq, ncap * nmax, fm, fn)    # on the frames of wide_frames_16
        ms = {name: [] for name in arms}

        def timed(run):
            for _ in range(2):
                run()
            dec.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                run()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / args.steps

        for _ in range(args.rounds):
            for name, run in arms.items():
                if name == "decode_messages":
                    arms["wide_frames_16"]()                                # its input
                ms[name].append(timed(run))
        dec.synchronize()
        for name in arms:
            out["arms"][name] = {"ms": [round(x, 4) for x in ms[name]], "best_ms": round(min(ms[name]), 4)}
        best = {name: out["arms"][name]["best_ms"] for name in arms}
        out["capture_tb_per_s"] = {str(n): round(out["capture_bytes"] / (best[f"wide_frames_{n}"] * 1e-3) / 1e12, 3) for n in CHANNEL_COUNTS}
        out["rx_decimate_tb_per_s"] = round(out["capture_bytes"] / (best["rx_decimate"] * 1e-3) / 1e12, 3)
        out["read_only_ceiling_tb_per_s"] = list(CEILING_TBS)
        out["fraction_of_ceiling"] = {k: round(v / CEILING_TBS[0], 3) for k, v in out["capture_tb_per_s"].items()}
        out["ms_per_channel"] = {str(n): round(best[f"wide_frames_{n}"] / n, 4) for n in CHANNEL_COUNTS}
        # stage A runs about 30 integer VALU operations per sample and channel
        out["stage_a_gops_per_s"] = {str(n): round(ncap * npairs * n * 30 / (best[f"wide_frames_{n}"] * 1e-3) / 1e9, 1) for n in CHANNEL_COUNTS}
        out["bound"] = "bandwidth" if out["fraction_of_ceiling"]["1"] >= 0.7 else "VALU (integer arithmetic of stage A)"
        out["t8_over_8_t1"] = round(best["wide_frames_8"] / (8 * best["wide_frames_1"]), 4)
        out["t16_over_16_t1"] = round(best["wide_frames_16"] / (16 * best["wide_frames_1"]), 4)
        out["wide_1_over_rx_decimate"] = round(best["wide_frames_1"] / best["rx_decimate"], 3)
        out["front_end_share_of_decode_wide"] = round(best["wide_frames_16"] / best["decode_wide_16"], 4)
        out["decode_wide_minus_parts_ms"] = round(best["decode_wide_16"] - best["wide_frames_16"] - best["decode_messages"], 4)
        out["messages"] = int(n_msgs.sum().item())
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
