"""Cost of a-priori decoding: ms per 4096-frame batch (synthetic frames, device pointers) of ft8gpu_decode_messages,
ft8gpu_decode_messages_deep (one pass, OSD order 1 at its recommended gate) and ft8gpu_decode_messages_ap with one ("CQ ? ?")
and two ("CQ ? ?", "CQ DX ? ?") hypotheses at the recommended gate, each without OSD and with OSD order 1 behind it, one
pass, interleaved in one session on one context, on the bench workload (20 CQ signals per frame, SNR U[-18, 0] dB); prints
one JSON line.

  python tools/bench_ap.py [--frames 4096] [--steps 20] [--warmup 3] [--out profiles/ap_bench.json]
  python tools/bench_ap.py --kernel-stats DIR/trace_kernel_stats.csv --out profiles/ap_bench.json     (adds the kernels' own times)

The kernels' own times come from one separate profiler run of this script:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python tools/bench_ap.py --steps 4 --warmup 1"""
import argparse
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


KERNELS = ("ft8_ap_kernel", "ft8_tag_kernel", "ft8_osd_kernel", "ft8_decode_kernel", "ft8_append_kernel")
FORMS = ("ap1", "ap1_osd1", "ap2", "ap2_osd1")           # the AP launches of one step, in order
HYPS = {1: ("CQ ? ?",), 2: ("CQ ? ?", "CQ DX ? ?")}


def kernel_stats(path):
    """name -> (calls, mean us) of the AP, OSD, LDPC and append kernels from a rocprofv3 --stats CSV; and, from the kernel
    trace beside it, the AP kernel's time per launch of a step (a step runs the four AP forms in the order of FORMS)"""
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
            rows = [r for r in csv.DictReader(f) if "ft8_ap_kernel(" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        if rows and len(rows) % len(FORMS) == 0:
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
            out["ft8_ap_kernel_by_launch_us"] = {name: round(sorted(us[i::len(FORMS)])[len(us) // len(FORMS) // 2], 1)
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
        doc["kernel_stats"] = dict(source="rocprofv3 --kernel-trace --stats of: python tools/bench_ap.py --steps 4 --warmup 1 "
                                          "(every form runs 5 times; AP launches alternate between 1 and 2 hypotheses)",
                                   kernels=kernel_stats(a.kernel_stats))
        with open(a.out, "w") as f:
            f.write(json.dumps(doc) + "\n")
        return
    import numpy as np
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    bid = ft8.check_build_id()
    B, gate, osd_gate = a.frames, ft8.AP_MAX_HARD_ERRORS, ft8.OSD_MAX_HARD_ERRORS
    nsig, snr = 20, (-18.0, 0.0)
    res = dict(metric="ms per batch", frames=B, steps=a.steps, build_id=bid, ap_gate=gate, osd_gate=osd_gate, signals_per_frame=nsig,
               snr_db=list(snr), hypotheses={str(k): list(v) for k, v in HYPS.items()})
    with ft8.Decoder(device=0, max_frames=B) as dec:
        res["overlap_active"] = dec.overlap_active()
        _, tones = workload.message_pool()
        sig, _ = workload.frame_signals(0, B, nsig, tones, snr_range=snr)
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, nsig, 1.0, workload.SEED_BASE, iq)
        msgs = torch.zeros((B, 50 * 64), dtype=torch.uint8, device="cuda")
        n = torch.zeros((B,), dtype=torch.int32, device="cuda")
        nbs2 = torch.zeros((B, 1, 2), dtype=torch.int32, device="cuda")
        nbs3 = torch.zeros((B, 1, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        runs = {"decode_messages": lambda: dec.decode_messages_dev(iq, B, msgs, n),
                "deep_osd1": lambda: dec.decode_messages_deep_dev(iq, B, 1, 1, osd_gate, msgs, n, nbs2)}
        for nh in (1, 2):
            for order in (-1, 1):
                runs[f"ap{nh}" + ("_osd1" if order >= 0 else "")] = (
                    lambda h=HYPS[nh], o=order: dec.decode_messages_ap_dev(iq, B, 1, h, gate, o, osd_gate, msgs, n, nbs3))
        for _ in range(a.warmup):
            for f in runs.values():
                f()
        dec.synchronize()
        times = {k: [] for k in runs}
        per_frame, stages = {}, {}
        for step in range(a.steps):                      # interleaved: every form sees the same clocks and neighbours
            for k, f in runs.items():
                t0 = time.perf_counter()
                f()
                dec.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
                if step == 0:
                    per_frame[k] = round(float(n.float().mean().item()), 4)
                    if k.startswith("ap"):
                        stages[k] = [round(float(v), 4) for v in nbs3.float().mean(dim=0)[0].tolist()]
        med = {k: float(np.median(v)) for k, v in times.items()}
        res["ms"] = {k: round(v, 4) for k, v in med.items()}
        res["spread_ms"] = {k: [round(float(np.percentile(v, 10)), 4), round(float(np.percentile(v, 90)), 4)] for k, v in times.items()}
        res["messages_per_frame"] = per_frame
        res["messages_per_frame_after_bp_ap_osd"] = stages
        res["ap_extra_ms"] = {"ap1": round(med["ap1"] - med["decode_messages"], 4), "ap2": round(med["ap2"] - med["decode_messages"], 4),
                              "ap1_before_osd1": round(med["ap1_osd1"] - med["deep_osd1"], 4),
                              "ap2_before_osd1": round(med["ap2_osd1"] - med["deep_osd1"], 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
