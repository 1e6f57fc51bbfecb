#!/usr/bin/env python3
"""Cost of the subtraction in the I/Q samples (ft8gpu_subtract_messages, ft8gpu_decode_messages_subtracted), measured on the GPU
in one session, device pointers, on 4096 frames of the bench workload (20 signals, -18 .. 0 dB, cap 120).

  python tools/bench_subtract.py [--json profiles/subtract_bench.json] [--steps 5] [--rounds 3] [--kernel-stats CSV]
  python tools/bench_subtract.py --stage-only 3          (three stage calls and nothing else: the program of a kernel trace)
  python tools/bench_subtract.py --shapes 0 1 [--json profiles/subtract_gfsk_bench.json]    (the shaped entries, see below)

Arms, interleaved round by round: the subtraction stage (estimate and apply kernels, in place on a copy of the frames) on the
batch's own first-pass records, the refine stage those records need first, ft8gpu_decode_messages, ft8gpu_decode_messages_passes
and ft8gpu_decode_messages_subtracted at 2 and 3 passes, and one LDPC launch (ft8gpu_decode_candidates) of the same batch.
Time = events on the context's stream around `steps` calls, after two warm-up calls, best of `rounds`; every round's figure is
kept.  --kernel-stats takes the trace_kernel_stats.csv of `rocprofv3 --kernel-trace --stats -- python tools/bench_subtract.py
--stage-only N` and adds the two kernels' own times per stage call; the apply kernel's is set against the time its floor of one
read and one write of every frame (768 KB) takes at 8 TB/s.  A machine without a GPU fails at ft8gpu_create; nothing is
estimated.
--shapes 0 1 goes through the shaped entries (ft8gpu_subtract_messages_shaped, ft8gpu_decode_messages_subtracted_shaped): the
stage and the whole path at two and three passes once per shape, the arms of shape 1 ("..._gfsk") right behind those of shape 0
in every round, and each GFSK arm's ratio to its CPFSK arm.  With --stage-only, N stage calls per shape; --kernel-stats then
finds the GFSK kernels beside the CPFSK ones and gives their ratios."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES, CAP = 4096, 120
HBM_BYTES_PER_S = 8e12


def kernel_times(path, calls):
    """ms per stage call of the two kernels from a trace_kernel_stats.csv covering `calls` stage calls"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for key in ("ft8_subtract_estimate_kernel", "ft8_subtract_apply_kernel", "ft8_subtract_estimate_gfsk_kernel",
                        "ft8_subtract_apply_gfsk_kernel"):
                if key in row["Name"]:
                    out[key] = {"launches": int(row["Calls"]), "ms_per_stage_call": round(float(row["TotalDurationNs"]) / 1e6 / calls, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--stage-only", type=int, default=0)
    ap.add_argument("--shapes", type=int, nargs="+", choices=(0, 1), help="use the shaped entries, one set of arms per shape")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--kernel-stats-calls", type=int, default=3)
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B = args.frames
    out = {"what": "cost of the subtraction in the I/Q samples on one MI355X (tools/bench_subtract.py)", "build_id": ft8.check_build_id(),
           "frames": B, "max_candidates": CAP, "steps": args.steps, "rounds": args.rounds, "arms": {}}
    with ft8.Decoder(device=0, max_frames=B, max_candidates=CAP) as dec:
        stream = torch.cuda.ExternalStream(dec.stream_handle())
        _, tones = workload.message_pool()
        sig, _ = workload.frame_signals(0, B, 20, tones, snr_range=(-18.0, 0.0))
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, 20, 1.0, workload.SEED_BASE, iq)
        u8 = lambda n: torch.zeros((n,), dtype=torch.uint8, device="cuda")
        i32 = lambda n: torch.zeros((n,), dtype=torch.int32, device="cuda")
        mag, cands, status, counts = u8(B * ft8.MAG_ARRAY), u8(B * CAP * 8), u8(B * CAP * 48), i32(B)
        msgs, n_msgs, refined, zero = u8(B * 50 * 64), i32(B), u8(B * 50 * 48), i32(B)
        msgs2, n_msgs2, nbp2, nbp3 = u8(B * 50 * 64), i32(B), i32(B * 2), i32(B * 3)
        x = iq.clone()
        dec.waterfall_dev(iq, B, mag)
        dec.find_sync_dev(mag, B, cands, counts)
        dec.decode_messages_dev(iq, B, msgs, n_msgs)
        dec.refine_messages_dev(iq, msgs, n_msgs, B, refined)
        dec.synchronize()
        out["messages"] = int(n_msgs.sum().item())
        # in place: the figures do not depend on the samples.  shape None: the entries without a shape
        stage_of = lambda shape: lambda: dec.subtract_messages_dev(x, msgs, refined, zero, n_msgs, B, x, shape=shape)
        whole_of = lambda shape, passes, nbp: lambda: dec.decode_messages_subtracted_dev(iq, B, passes, msgs2, n_msgs2, nbp, shape=shape)
        shapes = args.shapes or [None]
        tag = lambda shape: "_gfsk" if shape == ft8.SUBTRACT_GFSK else ""
        if args.stage_only:
            for shape in shapes:
                for _ in range(args.stage_only):
                    stage_of(shape)()
            dec.synchronize()
            return 0
        arms = {}
        for shape in shapes:
            arms["subtract_stage" + tag(shape)] = stage_of(shape)
        arms.update({"refine_stage": lambda: dec.refine_messages_dev(iq, msgs, n_msgs, B, refined),
                     "decode_messages": lambda: dec.decode_messages_dev(iq, B, msgs2, n_msgs2),
                     "decode_messages_passes_2": lambda: dec.decode_messages_passes_dev(iq, B, 2, msgs2, n_msgs2, nbp2),
                     "decode_messages_passes_3": lambda: dec.decode_messages_passes_dev(iq, B, 3, msgs2, n_msgs2, nbp3)})
        for passes, nbp in ((2, nbp2), (3, nbp3)):
            for shape in shapes:
                arms["decode_messages_subtracted_%d" % passes + tag(shape)] = whole_of(shape, passes, nbp)
        arms["ldpc_launch"] = lambda: dec.decode_candidates_dev(mag, cands, counts, B, status)
        if args.shapes:
            out["shapes"] = args.shapes
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
        for name in arms:
            out["arms"][name] = {"ms": [round(v, 4) for v in ms[name]], "best_ms": round(min(ms[name]), 4)}
        ldpc, plain = out["arms"]["ldpc_launch"]["best_ms"], out["arms"]["decode_messages"]["best_ms"]
        for name in arms:
            out["arms"][name]["ratio_to_ldpc_launch"] = round(out["arms"][name]["best_ms"] / ldpc, 4)
            out["arms"][name]["ratio_to_decode_messages"] = round(out["arms"][name]["best_ms"] / plain, 4)
            if name.endswith("_gfsk") and name[:-5] in arms:
                out["arms"][name]["ratio_to_cpfsk_arm"] = round(out["arms"][name]["best_ms"] / out["arms"][name[:-5]]["best_ms"], 4)
        # what the paths decode on this batch, counted once more outside the timed loops
        arms["decode_messages_passes_3"]()
        dec.synchronize()
        out["records_masking_by_pass"] = nbp3.view(B, 3).sum(dim=0).tolist()
        arms["decode_messages_subtracted_3"]()
        dec.synchronize()
        out["records_subtracted_by_pass"] = nbp3.view(B, 3).sum(dim=0).tolist()
        if "decode_messages_subtracted_3_gfsk" in arms:                 # CPFSK frames: the bench workload's synthesiser makes no GFSK
            arms["decode_messages_subtracted_3_gfsk"]()
            dec.synchronize()
            out["records_subtracted_gfsk_by_pass"] = nbp3.view(B, 3).sum(dim=0).tolist()
    floor_ms = B * 2 * 2 * ft8.NSAMPLES * 4 / HBM_BYTES_PER_S * 1e3
    out["apply_floor"] = {"bytes_per_frame": 2 * 2 * ft8.NSAMPLES * 4, "hbm_bytes_per_s": HBM_BYTES_PER_S, "floor_ms": round(floor_ms, 4)}
    if args.kernel_stats:
        out["kernels"] = kernel_times(args.kernel_stats, args.kernel_stats_calls)
        k = out["kernels"].get("ft8_subtract_apply_kernel")
        if k:
            k["floor_over_measured"] = round(floor_ms / k["ms_per_stage_call"], 4)
        for name in ("estimate", "apply"):
            c, g = out["kernels"].get("ft8_subtract_%s_kernel" % name), out["kernels"].get("ft8_subtract_%s_gfsk_kernel" % name)
            if c and g:
                g["ratio_to_cpfsk_kernel"] = round(g["ms_per_stage_call"] / c["ms_per_stage_call"], 4)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
