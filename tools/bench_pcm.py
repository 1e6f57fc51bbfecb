#!/usr/bin/env python3
"""Cost of the PCM front end (ft8gpu_pcm_frames), measured on the GPU in one session, device pointers: 16 captures of 15 s,
complex int16, at 48, 192 and 768 ksps (D = 15, 60, 240) with 1, 2, 8 and 16 channels, and real int16 at 48 ksps with two
channels, uniform random samples, on a context of 256 frames.

  python tools/bench_pcm.py [--json profiles/pcm_bench.json] [--steps 5] [--rounds 3] [--captures 16]

The arms are interleaved round by round.  Time = events on the context's stream around `steps` calls, after two warm-up calls,
best of `rounds`; every round's figure is kept.  The capture bytes over the stage's time are set against the project's measured
read-only ceiling of 6.2 .. 6.4 TB/s (profiles/README.md).  Stage A does 8 M + 1 taps per 9600 sps output and channel, each two
products and two adds from two LDS reads, and 6 operations per sample and channel in the mixer: the VALU operations per second
that follow from the time are reported beside the bytes, and the arm is called bandwidth-bound only at 70 % of the ceiling or
more.  Reading the samples once shows in the time at 16 channels against 16 times the time at 1 channel: the ratio is 1 if every
channel costs what the first does, and falls below 1 by what the channels share (the fetch, the staging in LDS, the launch).
ft8gpu_wide_frames and ft8gpu_audio_frames stand beside it from their committed profiles, as context: their inputs differ.  A
machine without a GPU fails at ft8gpu_create; nothing is estimated."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CEILING_TBS = (6.2, 6.4)
CHANNEL_COUNTS = (1, 2, 8, 16)
DS = (15, 60, 240)


def bins(D, n, real=False):
    """n channels spread over the input band, every c and q different"""
    lo, hi = (0 if real else -256 * D), 256 * D - 256
    return tuple(int(lo + (hi - lo) * (2 * k + 1) // 32 + 3 * k) for k in range(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--captures", type=int, default=16)
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    ncap, nmax = args.captures, max(CHANNEL_COUNTS)
    cplx, real = ft8.PCM_S16 | ft8.PCM_COMPLEX, ft8.PCM_S16
    out = {"what": "cost of the PCM front end on one MI355X (tools/bench_pcm.py)", "build_id": ft8.check_build_id(), "captures": ncap,
           "seconds_per_capture": 15, "steps": args.steps, "rounds": args.rounds, "arms": {}}
    with ft8.Decoder(device=0, max_frames=ncap * nmax) as dec:
        stream = torch.cuda.ExternalStream(dec.stream_handle())
        gen = torch.Generator(device="cuda").manual_seed(1)
        pcm = {D: torch.randint(-32768, 32768, (ncap, 2 * 48000 * D), dtype=torch.int16, device="cuda", generator=gen) for D in DS}
        iq = torch.empty((ncap * nmax, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        arms, info = {}, {}
        for D in DS:
            for n in CHANNEL_COUNTS:
                name = f"pcm_frames_d{D}_complex_{n}"
                arms[name] = (lambda D=D, n=n: dec.pcm_frames_dev(pcm[D], cplx, 3200 * D, ncap, 48000 * D, bins(D, n), iq, True))
                info[name] = (D, n, 2)
        # the real arm reads the first half of each 48 ksps capture's elements as 720 000 real samples
        arms["pcm_frames_d15_real_2"] = lambda: dec.pcm_frames_dev(pcm[15], real, 48000, ncap, 48000 * 15, bins(15, 2, True), iq, True)
        info["pcm_frames_d15_real_2"] = (15, 2, 1)
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
                ms[name].append(timed(run))
        dec.synchronize()
        for name in arms:
            D, n, ncomp = info[name]
            best = min(ms[name])
            in_bytes = ncap * 48000 * D * ncomp * 2
            taps = 8 * (D // 3) + 1
            # per 9600 sps output and channel: 4 operations per tap; per sample and channel: 6 (complex) or 2 (real) in the mixer
            ops = ncap * n * (144000 * taps * 4 + 48000 * D * (6 if ncomp == 2 else 2))
            tbs = in_bytes / (best * 1e-3) / 1e12
            out["arms"][name] = {"ms": [round(x, 4) for x in ms[name]], "best_ms": round(best, 4), "input_bytes": in_bytes,
                                 "input_tb_per_s": round(tbs, 4), "fraction_of_ceiling": round(tbs / CEILING_TBS[0], 4),
                                 "stage_a_valu_tops_per_s": round(ops / (best * 1e-3) / 1e12, 2), "ms_per_channel": round(best / n, 4),
                                 "bound": "bandwidth" if tbs / CEILING_TBS[0] >= 0.7 else "stage A's multiplies and adds from LDS"}
        out["read_only_ceiling_tb_per_s"] = list(CEILING_TBS)
        out["t16_over_16_t1"] = {str(D): round(out["arms"][f"pcm_frames_d{D}_complex_16"]["best_ms"] /
                                               (16 * out["arms"][f"pcm_frames_d{D}_complex_1"]["best_ms"]), 4) for D in DS}
        out["t8_over_8_t1"] = {str(D): round(out["arms"][f"pcm_frames_d{D}_complex_8"]["best_ms"] /
                                             (8 * out["arms"][f"pcm_frames_d{D}_complex_1"]["best_ms"]), 4) for D in DS}
    context = {}
    for key, path, pick in (("wide_frames_ms_1_2_8_16", "wide_bench.json", lambda d: [d["arms"][f"wide_frames_{n}"]["best_ms"] for n in CHANNEL_COUNTS]),
                            ("audio_frames_ms_4096_clips_2_bands", "audio_bench.json",
                             lambda d: next(v["best_ms"] for k, v in d["arms"].items() if "frames" in k))):
        try:
            with open(os.path.join(ROOT, "profiles", path)) as f:
                context[key] = pick(json.load(f))
        except (OSError, KeyError, StopIteration, TypeError):
            context[key] = None
    out["context_from_committed_profiles"] = context
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
