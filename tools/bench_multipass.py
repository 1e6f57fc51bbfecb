"""Cost of multi-pass decoding: ms per 4096-frame batch (synthetic frames, device pointers) of ft8gpu_decode_messages and of
ft8gpu_decode_messages_passes at 2 and 3 passes, interleaved in one session on one context, on the bench workload (20 CQ
signals per frame, SNR U[-18, 0] dB) and on a crowded one (30 signals, U[-22, 0] dB); prints one JSON line.

  python tools/bench_multipass.py [--frames 4096] [--steps 30] [--warmup 5] [--out FILE]

Per-kernel times of the new kernels come from a profiler run of this script:
  rocprofv3 --kernel-trace --stats -d OUTDIR -- python tools/bench_multipass.py --steps 10"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"bench_20sig": (20, (-18.0, 0.0)), "crowded_30sig": (30, (-22.0, 0.0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    bid = ft8.check_build_id()
    B = a.frames
    res = dict(metric="ms per batch", frames=B, steps=a.steps, build_id=bid, workloads={})
    with ft8.Decoder(device=0, max_frames=B) as dec:
        res["overlap_active"] = dec.overlap_active()
        _, tones = workload.message_pool()
        for name, (nsig, snr) in WORKLOADS.items():
            sig, _ = workload.frame_signals(0, B, nsig, tones, snr_range=snr)
            iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
            dec.synth_frames(sig, B, nsig, 1.0, workload.SEED_BASE, iq)
            msgs = torch.zeros((B, 50 * 64), dtype=torch.uint8, device="cuda")
            n = torch.zeros((B,), dtype=torch.int32, device="cuda")
            nbp = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
            nbp2 = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            runs = {"decode_messages": lambda: dec.decode_messages_dev(iq, B, msgs, n),
                    "passes_2": lambda: dec.decode_messages_passes_dev(iq, B, 2, msgs, n, nbp2),
                    "passes_3": lambda: dec.decode_messages_passes_dev(iq, B, 3, msgs, n, nbp)}
            for _ in range(a.warmup):
                for f in runs.values():
                    f()
            dec.synchronize()
            times = {k: [] for k in runs}
            for _ in range(a.steps):                     # interleaved: every form sees the same clocks and neighbours
                for k, f in runs.items():
                    t0 = time.perf_counter()
                    f()
                    dec.synchronize()
                    times[k].append((time.perf_counter() - t0) * 1e3)
            dec.decode_messages_passes_dev(iq, B, 3, msgs, n, nbp)
            dec.synchronize()
            per_pass = nbp.cpu().numpy()
            active = [int(B)] + [int((per_pass[:, p - 1] > (per_pass[:, p - 2] if p >= 2 else 0)).sum()) for p in (1, 2)]
            med = {k: float(np.median(v)) for k, v in times.items()}
            res["workloads"][name] = dict(
                signals_per_frame=nsig, snr_db=list(snr),
                ms={k: round(v, 4) for k, v in med.items()},
                spread_ms={k: [round(float(np.percentile(v, 10)), 4), round(float(np.percentile(v, 90)), 4)] for k, v in times.items()},
                pass_2_extra_ms=round(med["passes_2"] - med["decode_messages"], 4),
                pass_3_extra_ms=round(med["passes_3"] - med["passes_2"], 4),
                pass_2_extra_pct=round(100.0 * (med["passes_2"] / med["decode_messages"] - 1.0), 2),
                messages_per_frame_by_pass=[round(float(per_pass[:, p].mean()), 4) for p in range(3)],
                frames_decoded_in_pass=active)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
