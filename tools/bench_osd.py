"""Cost of ordered-statistics decoding: ms per 4096-frame batch (synthetic frames, device pointers) of
ft8gpu_decode_messages, ft8gpu_decode_messages_passes with passes = 2, and ft8gpu_decode_messages_deep at orders 1 and 2
with passes 1 and 2 (the recommended gate), interleaved in one session on one context, on the bench workload (20 CQ signals
per frame, SNR U[-18, 0] dB); prints one JSON line.

  python tools/bench_osd.py [--frames 4096] [--steps 20] [--warmup 3] [--out profiles/osd_bench.json]
  python tools/bench_osd.py --kernel-stats DIR/trace_kernel_stats.csv --out profiles/osd_bench.json     (adds the kernels' own times)

The kernels' own times come from one separate profiler run of this script:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python tools/bench_osd.py --steps 4 --warmup 1"""
import argparse
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


KERNELS = ("ft8_osd_kernel", "ft8_tag_kernel", "ft8_decode_kernel", "ft8_append_kernel")
FORMS = ("p1_o1", "p1_o2", "p2_o1_pass1", "p2_o1_pass2", "p2_o2_pass1", "p2_o2_pass2")   # OSD launches of one step, in order


def kernel_stats(path):
    """name -> (calls, mean us) of the OSD, LDPC and append kernels from a rocprofv3 --stats CSV; and, from the kernel
    trace beside it, the OSD kernel's time per launch of a step (a step runs the four deep forms in the order of FORMS)"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"(ft8_\w+(?:<[^>]*>)?)\(", row.get("Name", ""))
            if m and m.group(1).split("<")[0] in KERNELS:
                out[m.group(1)] = dict(calls=int(row["Calls"]), mean_us=round(float(row["AverageNs"]) / 1e3, 2),
                                       total_ms=round(float(row["TotalDurationNs"]) / 1e6, 3))
    trace = path.replace("kernel_stats.csv", "kernel_trace.csv")
    if os.path.exists(trace):
        with open(trace) as f:
            rows = [r for r in csv.DictReader(f) if "ft8_osd_kernel(" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        if rows and len(rows) % len(FORMS) == 0:
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
            out["ft8_osd_kernel_by_launch_us"] = {name: round(sorted(us[i::len(FORMS)])[len(us) // len(FORMS) // 2], 1)
                                                  for i, name in enumerate(FORMS)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None, help="merge a rocprofv3 trace_kernel_stats.csv into --out and exit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        doc = json.load(open(a.out))
        doc["kernel_stats"] = dict(source="rocprofv3 --kernel-trace --stats of: python tools/bench_osd.py --steps 4 --warmup 1 "
                                          "(every form runs 5 times; OSD launches alternate between orders 1 and 2)",
                                   kernels=kernel_stats(a.kernel_stats))
        with open(a.out, "w") as f:
            f.write(json.dumps(doc) + "\n")
        return
    import numpy as np
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    bid = ft8.check_build_id()
    B, gate = a.frames, ft8.OSD_MAX_HARD_ERRORS
    nsig, snr = 20, (-18.0, 0.0)
    res = dict(metric="ms per batch", frames=B, steps=a.steps, build_id=bid, gate=gate, signals_per_frame=nsig, snr_db=list(snr))
    with ft8.Decoder(device=0, max_frames=B) as dec:
        res["overlap_active"] = dec.overlap_active()
        _, tones = workload.message_pool()
        sig, _ = workload.frame_signals(0, B, nsig, tones, snr_range=snr)
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, nsig, 1.0, workload.SEED_BASE, iq)
        msgs = torch.zeros((B, 50 * 64), dtype=torch.uint8, device="cuda")
        n = torch.zeros((B,), dtype=torch.int32, device="cuda")
        nbp2 = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
        nbs = {p: torch.zeros((B, p, 2), dtype=torch.int32, device="cuda") for p in (1, 2)}
        torch.cuda.synchronize()
        runs = {"decode_messages": lambda: dec.decode_messages_dev(iq, B, msgs, n),
                "passes_2": lambda: dec.decode_messages_passes_dev(iq, B, 2, msgs, n, nbp2)}
        for passes in (1, 2):
            for order in (1, 2):
                runs[f"deep_p{passes}_o{order}"] = (lambda p=passes, o=order: dec.decode_messages_deep_dev(iq, B, p, o, gate, msgs, n, nbs[p]))
        for _ in range(a.warmup):
            for f in runs.values():
                f()
        dec.synchronize()
        times = {k: [] for k in runs}
        per_frame = {}
        for step in range(a.steps):                      # interleaved: every form sees the same clocks and neighbours
            for k, f in runs.items():
                t0 = time.perf_counter()
                f()
                dec.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
                if step == 0:
                    per_frame[k] = round(float(n.float().mean().item()), 4)
        med = {k: float(np.median(v)) for k, v in times.items()}
        res["ms"] = {k: round(v, 4) for k, v in med.items()}
        res["spread_ms"] = {k: [round(float(np.percentile(v, 10)), 4), round(float(np.percentile(v, 90)), 4)] for k, v in times.items()}
        res["messages_per_frame"] = per_frame
        res["osd_extra_ms"] = {f"p{p}_o{o}": round(med[f"deep_p{p}_o{o}"] - med["decode_messages" if p == 1 else "passes_2"], 4)
                               for p in (1, 2) for o in (1, 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
