#!/usr/bin/env python3
"""Cost of the demodulation from the I/Q samples (ft8gpu_demod_candidates, ft8gpu_decode_messages_demod), measured on the GPU
in one session, device pointers, on 4096 frames of the bench workload (20 signals, -18 .. 0 dB, cap 120).

  python tools/bench_demod.py [--json profiles/demod_bench.json] [--steps 5] [--rounds 3] [--parent LIB [LIB]]

Arms, interleaved round by round: the stage alone on the batch's own BP status records at max_per_frame = 16, 48 and the cap
with the recommended sets, each set alone at the cap, ft8gpu_decode_messages, ft8gpu_decode_messages_demod with the recommended
parameters, and one LDPC launch (ft8gpu_decode_candidates) of the same batch.  Time = events on the context's stream around
`steps` calls, after two warm-up calls, best of `rounds`; every round's figure is kept.  The records [0, n1) of the whole path
must equal ft8gpu_decode_messages'.  --parent: builds of the parent commit, handed to tools/ab_libs.py beside this build for
ft8gpu_decode_batch and ft8gpu_decode_messages (fresh processes, after this one's context is closed); the bar for the product
path is the parent arms' own spread.  A machine without a GPU fails at ft8gpu_create; nothing is estimated."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES, CAP = 4096, 120


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--parent", nargs="*", default=[])
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B = args.frames
    SETS, GATE = ft8.DEMOD_SETS, ft8.DEMOD_MAX_HARD_ERRORS
    out = {"what": "cost of the demodulation from the I/Q samples on one MI355X (tools/bench_demod.py)", "build_id": ft8.check_build_id(),
           "frames": B, "max_candidates": CAP, "sets": SETS, "max_hard_errors": GATE, "steps": args.steps, "rounds": args.rounds, "arms": {}}
    with ft8.Decoder(device=0, max_frames=B, max_candidates=CAP) as dec:
        stream = torch.cuda.ExternalStream(dec.stream_handle())
        _, tones = workload.message_pool()
        sig, _ = workload.frame_signals(0, B, 20, tones, snr_range=(-18.0, 0.0))
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, 20, 1.0, workload.SEED_BASE, iq)
        u8 = lambda n: torch.zeros((n,), dtype=torch.uint8, device="cuda")
        i32 = lambda n: torch.zeros((n,), dtype=torch.int32, device="cuda")
        mag, cands, status, counts = u8(B * ft8.MAG_ARRAY), u8(B * CAP * 8), u8(B * CAP * 48), i32(B)
        status2, info = u8(B * CAP * 48), u8(B * CAP * 16)
        msgs, n_msgs = u8(B * 50 * 64), i32(B)
        msgs2, n_msgs2, nbs = u8(B * 50 * 64), i32(B), i32(2 * B)
        dec.waterfall_dev(iq, B, mag)
        dec.find_sync_dev(mag, B, cands, counts)
        dec.decode_candidates_dev(mag, cands, counts, B, status)
        dec.decode_messages_dev(iq, B, msgs, n_msgs)
        dec.synchronize()
        st = status.cpu().numpy().view(ft8.STATUS_DTYPE).reshape(B, CAP)
        cnt = counts.cpu().numpy()
        live = (torch.arange(CAP)[None, :].numpy() < cnt[:, None])
        failing = live & (st["ok"] == 0) & (st["ldpc_errors"] != 0)
        out["candidates"], out["failing_candidates"], out["messages"] = int(cnt.sum()), int(failing.sum()), int(n_msgs.sum().item())
        stage = lambda sets, mpf: (lambda: dec.demod_candidates_dev(iq, cands, counts, status, B, sets, GATE, mpf, status2, info))
        arms = {"stage_mpf16": stage(SETS, 16), "stage_mpf48": stage(SETS, 48), "stage_mpf%d" % CAP: stage(SETS, CAP),
                "stage_set1": stage(1, CAP), "stage_set2": stage(2, CAP), "stage_set3": stage(4, CAP),
                "decode_messages": lambda: dec.decode_messages_dev(iq, B, msgs2, n_msgs2),
                "decode_messages_demod": lambda: dec.decode_messages_demod_dev(iq, B, SETS, GATE, CAP, msgs2, n_msgs2, nbs),
                "ldpc_launch": lambda: dec.decode_candidates_dev(mag, cands, counts, B, status2)}
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
            out["arms"][name] = {"ms": [round(x, 4) for x in ms[name]], "best_ms": round(min(ms[name]), 4)}
        ldpc, plain = out["arms"]["ldpc_launch"]["best_ms"], out["arms"]["decode_messages"]["best_ms"]
        for name in arms:
            out["arms"][name]["ratio_to_ldpc_launch"] = round(out["arms"][name]["best_ms"] / ldpc, 4)
            out["arms"][name]["ratio_to_decode_messages"] = round(out["arms"][name]["best_ms"] / plain, 4)
        out["us_per_attempted_candidate"] = round(1e3 * out["arms"]["stage_mpf%d" % CAP]["best_ms"] / max(out["failing_candidates"], 1), 4)
        # the whole path once more for the figures: records [0, n1) and the counts
        dec.decode_messages_demod_dev(iq, B, SETS, GATE, CAP, msgs2, n_msgs2, nbs)
        dec.synchronize()
        n1, n2, hb = n_msgs.cpu().numpy(), n_msgs2.cpu().numpy(), nbs.cpu().numpy().reshape(B, 2)
        a, b = msgs.cpu().numpy().reshape(B, 50, 64), msgs2.cpu().numpy().reshape(B, 50, 64)
        out["records_equal_decode_messages"] = bool((hb[:, 0] == n1).all() and (hb[:, 1] == n2).all() and
                                                    all(a[f, :n1[f]].tobytes() == b[f, :n1[f]].tobytes() for f in range(B)))
        out["messages_after_stage"] = int(n2.sum())
    if args.parent:
        out["product_path"] = {}
        libs = list(args.parent) + [os.path.relpath(ft8.LIB_PATH, ROOT)]
        for entry in ("batch", "messages"):
            text = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "ab_libs.py"), "--libs"] + libs +
                                           ["--entry", entry, "--steps", "20", "--rounds", "3"], cwd=ROOT, text=True)
            out["product_path"]["decode_" + entry] = json.loads(text.strip().splitlines()[-1])
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0 if out["records_equal_decode_messages"] else 1


if __name__ == "__main__":
    sys.exit(main())
