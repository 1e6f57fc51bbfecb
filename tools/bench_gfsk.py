#!/usr/bin/env python3
"""Cost of the GFSK synthesiser (ft8gpu_synth_gfsk_frames, ft8gpu_synth_gfsk_audio) beside the CPFSK synthesiser
ft8gpu_synth_frames on the same batch, measured on the GPU in one session, device pointers.

  python tools/bench_gfsk.py [--json profiles/gfsk_bench.json] [--steps 5] [--rounds 3] [--clips 4096]

The batch: 4096 frames (clips) of 20 signals of the bench's message pool, -18 .. 0 dB in 2500 Hz against noise of sigma 1, 100 ..
1500 Hz (I/Q) and 200 .. 3000 Hz (audio), starting in 0 .. 1.8 s; noise on, peak 0.5 (ft8gpu_synth_frames always normalises).
Four arms, interleaved round by round: GFSK frames, CPFSK frames, GFSK audio as float32 and as int16.  Time = events on the
context's stream around `steps` calls after two warm-up calls, best of `rounds`; every round's figure is kept.  A call includes
the host's share (the upload of the signal records; for GFSK also deriving the headers).  signal-samples per second = signals x
79 symbols x samples per symbol over the time.  The resource line of the GFSK kernels comes from the compiler's assembly
(tools/kernel_resources.py).  A machine without a GPU fails at ft8gpu_create; nothing is estimated."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLIPS, NSIG = 4096, 20


def signals(ft8, workload, n, f_range, seed):
    _, tones = workload.message_pool()
    rng = np.random.default_rng(seed)
    s = np.zeros((n, NSIG), ft8.SIGNAL_DTYPE)
    s["tones"] = tones[rng.integers(0, len(tones), (n, NSIG))]
    s["f0_hz"] = rng.uniform(*f_range, (n, NSIG))
    s["t0_s"] = rng.uniform(0.0, 1.8, (n, NSIG))
    snr = rng.uniform(-18.0, 0.0, (n, NSIG))
    s["amplitude"] = np.sqrt(2.0 * 2500.0 / 3200.0 * 10.0 ** (snr / 10.0))
    return s


def resources():
    import kernel_resources as K
    ks = K.kernels_of(K.assemble(os.path.join(K.CSRC, "gfsk.hip")))
    rows = []
    for k, nice in zip(ks, K.demangle([k["symbol"] for k in ks])):
        waves = K.waves_per_simd(k)
        wg_waves = 256 // 64
        per_cu = min(4 * waves // wg_waves, (160 * 1024) // max(k["lds_bytes"], 1))
        rows.append({"kernel": nice, "vgprs": k["vgprs"], "sgprs": k["sgprs"], "lds_bytes": k["lds_bytes"],
                     "scratch_bytes_per_lane": k["scratch_bytes_per_lane"], "waves_per_simd": waves, "workgroups_per_cu": per_cu})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clips", type=int, default=CLIPS)
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B = args.clips
    out = {"what": "cost of the GFSK synthesiser beside the CPFSK one on one MI355X (tools/bench_gfsk.py)", "build_id": ft8.check_build_id(),
           "clips": B, "signals_per_clip": NSIG, "noise_sigma": 1.0, "peak": 0.5, "steps": args.steps, "rounds": args.rounds, "arms": {}}
    sig_iq = signals(ft8, workload, B, (100.0, 1500.0), workload.SEED_BASE)
    sig_au = signals(ft8, workload, B, (200.0, 3000.0), workload.SEED_BASE + 1)
    with ft8.Decoder(device=0, max_frames=B) as dec:
        stream = torch.cuda.ExternalStream(dec.stream_handle())
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        iq_c = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        au_f = torch.empty((B, ft8.AUDIO_NSAMPLES), dtype=torch.float32, device="cuda")
        au_s = torch.empty((B, ft8.AUDIO_NSAMPLES), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        N = ft8.AUDIO_NSAMPLES
        arms = {"gfsk_frames": lambda: dec.synth_gfsk_frames_dev(sig_iq, B, NSIG, 1.0, 7, 0, 0.5, iq),
                "cpfsk_frames": lambda: dec.synth_frames(sig_iq, B, NSIG, 1.0, 7, iq_c),
                "gfsk_audio_f32": lambda: dec.synth_gfsk_audio_dev(sig_au, B, NSIG, N, 1.0, 7, 0, 0.5, ft8.AUDIO_F32, au_f),
                "gfsk_audio_s16": lambda: dec.synth_gfsk_audio_dev(sig_au, B, NSIG, N, 1.0, 7, 0, 0.5, ft8.AUDIO_S16, au_s)}
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
            sps = 1920 if "audio" in name else 512
            best = min(ms[name])
            out["arms"][name] = {"ms": [round(x, 3) for x in ms[name]], "best_ms": round(best, 3),
                                 "signal_samples_per_s": round(B * NSIG * 79 * sps / (best * 1e-3), 0),
                                 "output_gb_per_s": round((B * (2 * ft8.NSAMPLES * 4 if "frames" in name else N * (2 if "s16" in name else 4)))
                                                          / (best * 1e-3) / 1e9, 1)}
        out["gfsk_over_cpfsk_frames"] = round(out["arms"]["gfsk_frames"]["best_ms"] / out["arms"]["cpfsk_frames"]["best_ms"], 3)
        # both synthesise the same signals in the same noise model; the frames differ only by the pulse shaping
        a, b = iq[:4].cpu().numpy().astype(np.float64), iq_c[:4].cpu().numpy().astype(np.float64)
        out["frames_rms"] = {"gfsk": round(float(np.sqrt((a ** 2).mean())), 5), "cpfsk": round(float(np.sqrt((b ** 2).mean())), 5)}
        out["audio_peak"] = {"f32": float(au_f[:4].abs().max().item()), "s16": int(au_s[:4].to(torch.int32).abs().max().item())}
    out["resources"] = resources()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
