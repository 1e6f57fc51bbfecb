#!/usr/bin/env python3
"""Cost of the fading channel (ft8gpu_synth_gfsk_frames_faded, ft8gpu_synth_gfsk_audio_faded) beside the unfaded GFSK entries on
the same batch, measured on the GPU in one session, device pointers.

  python tools/bench_channel.py [--json profiles/channel_bench.json] [--steps 9] [--rounds 3] [--clips 4096]
  python tools/bench_channel.py --parent tools/ab/libft8gpu_parent.so --json profiles/channel_ab_parent.json

The batch is tools/bench_gfsk.py's: 4096 frames (clips) of 20 signals, noise on, peak 0.5.  Arms, interleaved round by round: I/Q
frames unfaded, with one faded path and with two faded paths per signal (spread 1 Hz, delay 2 ms), then audio clips as float32
unfaded and with two paths.  Every step is timed on its own with events on the context's stream, after two warm-up calls; an
arm's figure is the median of its steps over all rounds, and every step's time is kept.  A faded arm is reported as a ratio to the
unfaded arm of the same run.  A call includes the host's share: deriving the headers and the taps and uploading them.

--parent: another build of the library (the parent commit's) is loaded beside this one and the unfaded entries of both are
timed, interleaved arm by arm, and their outputs compared byte for byte: the unfaded entries must not change in output or in
time.  A machine without a GPU fails at ft8gpu_create; nothing is estimated."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
NSIG = 20


def step_times(torch, dec, stream, run, steps):
    """the time of every one of `steps` calls in ms, after two warm-up calls"""
    for _ in range(2):
        run()
    dec.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record(stream)
    for k in range(steps):
        run()
        ev[k + 1].record(stream)
    ev[-1].synchronize()
    return [ev[k].elapsed_time(ev[k + 1]) for k in range(steps)]


def summary(ms):
    return {"ms": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--parent", help="the parent commit's libft8gpu.so: A/B of the unfaded entries instead of the bench")
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    import bench_gfsk
    B, N = args.clips, ft8.AUDIO_NSAMPLES
    sig_iq = bench_gfsk.signals(ft8, workload, B, (100.0, 1500.0), workload.SEED_BASE)
    sig_au = bench_gfsk.signals(ft8, workload, B, (200.0, 3000.0), workload.SEED_BASE + 1)
    out = {"build_id": ft8.check_build_id(), "clips": B, "signals_per_clip": NSIG, "noise_sigma": 1.0, "peak": 0.5, "steps": args.steps,
           "rounds": args.rounds, "arms": {}}
    iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
    au = torch.empty((B, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    if args.parent:
        out["what"] = ("the unfaded GFSK entries of the parent build and of this one, interleaved in one session on one MI355X "
                       "(tools/bench_channel.py --parent)")
        out["parent_build_id"] = ft8.build_id(ft8.load_library_at(args.parent))
        decs = {"parent": ft8.Decoder(device=0, max_frames=B, lib=ft8.load_library_at(args.parent)), "this": ft8.Decoder(device=0, max_frames=B)}
        ms, digests = {}, {}
        for _ in range(args.rounds):
            for entry in ("gfsk_frames", "gfsk_audio_f32"):
                for name in ("parent", "this", "this", "parent"):
                    dec = decs[name]
                    stream = torch.cuda.ExternalStream(dec.stream_handle())
                    if entry == "gfsk_frames":
                        run, buf = (lambda: dec.synth_gfsk_frames_dev(sig_iq, B, NSIG, 1.0, 7, 0, 0.5, iq)), iq
                    else:
                        run, buf = (lambda: dec.synth_gfsk_audio_dev(sig_au, B, NSIG, N, 1.0, 7, 0, 0.5, ft8.AUDIO_F32, au)), au
                    ms.setdefault((entry, name), []).extend(step_times(torch, dec, stream, run, args.steps))
                    dec.synchronize()
                    digests.setdefault(entry, set()).add(hashlib.sha256(buf[:64].cpu().numpy().tobytes()).hexdigest()[:16])
        for dec in decs.values():
            dec.close()
        for entry in ("gfsk_frames", "gfsk_audio_f32"):
            out["arms"][entry] = {name: summary(ms[entry, name]) for name in ("parent", "this")}
            out["arms"][entry]["this_over_parent_median"] = round(out["arms"][entry]["this"]["median_ms"] / out["arms"][entry]["parent"]["median_ms"], 4)
            out["arms"][entry]["digests_of_the_first_64_clips"] = sorted(digests[entry])
        out["outputs_equal"] = all(len(d) == 1 for d in digests.values())
    else:
        out["what"] = "cost of the fading channel beside the unfaded GFSK synthesiser on one MI355X (tools/bench_channel.py)"
        one = ft8.channel_preset("none", (B, NSIG))
        one["spread_hz"], one["delay_ms"], one["path2_gain"], one["mode"] = 1.0, 2.0, 0.0, ft8.CHANNEL_FADED
        two = one.copy()
        two["path2_gain"] = 1.0
        with ft8.Decoder(device=0, max_frames=B) as dec:
            stream = torch.cuda.ExternalStream(dec.stream_handle())
            arms = {"frames_unfaded": lambda: dec.synth_gfsk_frames_dev(sig_iq, B, NSIG, 1.0, 7, 0, 0.5, iq),
                    "frames_one_path": lambda: dec.synth_gfsk_frames_faded_dev(sig_iq, one, B, NSIG, 1.0, 7, 0, 0.5, iq),
                    "frames_two_paths": lambda: dec.synth_gfsk_frames_faded_dev(sig_iq, two, B, NSIG, 1.0, 7, 0, 0.5, iq),
                    "audio_f32_unfaded": lambda: dec.synth_gfsk_audio_dev(sig_au, B, NSIG, N, 1.0, 7, 0, 0.5, ft8.AUDIO_F32, au),
                    "audio_f32_two_paths": lambda: dec.synth_gfsk_audio_faded_dev(sig_au, two, B, NSIG, N, 1.0, 7, 0, 0.5, ft8.AUDIO_F32, au)}
            ms = {name: [] for name in arms}
            for _ in range(args.rounds):
                for name, run in arms.items():
                    ms[name].extend(step_times(torch, dec, stream, run, args.steps))
            dec.synchronize()
            for name in arms:
                out["arms"][name] = summary(ms[name])
            rms = float(np.sqrt((iq[:4].cpu().numpy().astype(np.float64) ** 2).mean()))
        med = {name: out["arms"][name]["median_ms"] for name in arms}
        out["ratio_to_unfaded"] = {"frames_one_path": round(med["frames_one_path"] / med["frames_unfaded"], 3),
                                   "frames_two_paths": round(med["frames_two_paths"] / med["frames_unfaded"], 3),
                                   "audio_f32_two_paths": round(med["audio_f32_two_paths"] / med["audio_f32_unfaded"], 3)}
        out["grid_values_bytes"] = B * NSIG * 2 * ft8.CHANNEL_GRID * 8
        out["frames_rms_last_arm"] = round(rms, 5)
        out["resources"] = bench_gfsk.resources()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
