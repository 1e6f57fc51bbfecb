#!/usr/bin/env python3
"""Cost of the refined time and frequency (ft8gpu_refine_messages, ft8gpu_decode_messages_refined), measured on the GPU in one
session, device pointers, on 4096 frames of the bench workload (20 signals, -18 .. 0 dB, cap 120).

  python tools/bench_refine.py [--json profiles/refine_bench.json] [--steps 10] [--rounds 3]

Four arms, interleaved round by round: the refine stage alone on the batch's own message records, ft8gpu_decode_messages,
ft8gpu_decode_messages_refined, and one LDPC launch (ft8gpu_decode_candidates) of the same batch.  Time = events on the
context's stream around `steps` calls, after three warm-up calls, best of `rounds`; every round's figure is kept.  msgs and
n_msgs of the whole path must equal ft8gpu_decode_messages'.  A machine without a GPU fails at ft8gpu_create; nothing is
estimated."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES, CAP = 4096, 120


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=FRAMES)
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B = args.frames
    out = {"what": "cost of the refined time and frequency on one MI355X (tools/bench_refine.py)", "build_id": ft8.check_build_id(),
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
        msgs, n_msgs, refined = u8(B * 50 * 64), i32(B), u8(B * 50 * 48)
        msgs2, n_msgs2, refined2 = u8(B * 50 * 64), i32(B), u8(B * 50 * 48)
        dec.waterfall_dev(iq, B, mag)
        dec.find_sync_dev(mag, B, cands, counts)
        dec.decode_messages_dev(iq, B, msgs, n_msgs)
        dec.synchronize()
        out["messages"] = int(n_msgs.sum().item())
        arms = {"refine_stage": lambda: dec.refine_messages_dev(iq, msgs, n_msgs, B, refined),
                "decode_messages": lambda: dec.decode_messages_dev(iq, B, msgs2, n_msgs2),
                "decode_messages_refined": lambda: dec.decode_messages_refined_dev(iq, B, msgs2, n_msgs2, refined2),
                "ldpc_launch": lambda: dec.decode_candidates_dev(mag, cands, counts, B, status)}
        ms = {name: [] for name in arms}

        def timed(run):
            for _ in range(3):
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
            out["arms"][name] = {"ms": [round(x, 4) for x in ms[name]], "best_ms": round(min(ms[name]), 4)}
        ldpc, plain = out["arms"]["ldpc_launch"]["best_ms"], out["arms"]["decode_messages"]["best_ms"]
        for name in arms:
            out["arms"][name]["ratio_to_ldpc_launch"] = round(out["arms"][name]["best_ms"] / ldpc, 4)
            out["arms"][name]["ratio_to_decode_messages"] = round(out["arms"][name]["best_ms"] / plain, 4)
        out["ms_per_message"] = round(out["arms"]["refine_stage"]["best_ms"] / max(out["messages"], 1), 7)
        dec.synchronize()
        out["records_equal_decode_messages"] = bool(torch.equal(msgs, msgs2) and torch.equal(n_msgs, n_msgs2))
        out["refined_equal_stage"] = bool(torch.equal(refined, refined2))
        out["refined_digest"] = hashlib.sha256(refined.cpu().numpy().tobytes()).hexdigest()[:16]
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if out["records_equal_decode_messages"] and out["refined_equal_stage"] else 1


if __name__ == "__main__":
    sys.exit(main())
