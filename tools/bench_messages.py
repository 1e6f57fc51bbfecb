"""Cost of the messages path: ms per configs[2] batch (4096 synthetic frames, device pointers) of ft8gpu_decode_messages
against ft8gpu_decode_batch, interleaved in one session on one context; prints one JSON line.

  python tools/bench_messages.py [--frames 4096] [--steps 50] [--warmup 5] [--out FILE]

Per-kernel times of the two new kernels come from a profiler run of this script:
  rocprofv3 --kernel-trace --stats -d OUTDIR -- python tools/bench_messages.py --steps 10"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    bid = ft8.check_build_id()
    B = a.frames
    with ft8.Decoder(device=0, max_frames=B) as dec:
        _, tones = workload.message_pool()
        sig, _ = workload.frame_signals(0, B, 20, tones, snr_range=(-18.0, 0.0))
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, 20, 1.0, workload.SEED_BASE, iq)
        spots = torch.zeros((B, 50 * 28), dtype=torch.uint8, device="cuda")
        msgs = torch.zeros((B, 50 * 64), dtype=torch.uint8, device="cuda")
        nres = torch.zeros((B,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        runs = {"decode_batch": lambda: dec.decode_batch_dev(iq, B, spots, nres),
                "decode_messages": lambda: dec.decode_messages_dev(iq, B, msgs, nres)}
        for _ in range(a.warmup):
            for f in runs.values():
                f()
        dec.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.steps):                     # interleaved: both forms see the same clocks and neighbours
            for k, f in runs.items():
                t0 = time.perf_counter()
                f()
                dec.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(v)) for k, v in times.items()}
        res = dict(metric="ms per batch", frames=B, steps=a.steps, build_id=bid, overlap_active=dec.overlap_active(),
                   decode_batch_ms=round(med["decode_batch"], 4), decode_messages_ms=round(med["decode_messages"], 4),
                   overhead_ms=round(med["decode_messages"] - med["decode_batch"], 4),
                   overhead_pct=round(100.0 * (med["decode_messages"] / med["decode_batch"] - 1.0), 2),
                   spread_ms={k: [round(float(np.percentile(v, 10)), 4), round(float(np.percentile(v, 90)), 4)] for k, v in times.items()})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
