#!/usr/bin/env python3
"""Cost of the call hash table (ft8gpu_resolve_calls, ft8gpu_decode_messages_resolved), measured on the GPU in one session.

  python tools/bench_callhash.py [--json profiles/callhash_bench.json] [--steps 20] [--rounds 3]

  stage   ft8gpu_resolve_calls, device form, on 4096 frames of 20 records laid out 4096 x 1, 256 x 16 and 16 x 256
          (receivers x slots): many receivers side by side at one end, the serial walk of a receiver at the other.  The
          records are made on the host: a91 from ft8gpu_pack77, about a third of them with a hashed call, the text with
          "<...>" in its place.  Time = host clock around `steps` calls that end in a synchronise, best of `rounds`.
  whole   ft8gpu_decode_messages_resolved against ft8gpu_decode_messages on the same 4096 synthesised frames (20 signals,
          -18 .. 0 dB, laid out 256 x 16), the two arms interleaved round by round; msgs and n_msgs of both must be equal.
A machine without a GPU fails at ft8gpu_create; nothing is estimated."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES, RECORDS = 4096, 20
LAYOUTS = ((4096, 1), (256, 16), (16, 256))
LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"


def make_records(ft8, seed=0xCA11):
    """msgs [4096][50], n_msgs [4096]: 20 records per frame from a pool of 400 calls"""
    rng = np.random.default_rng(seed)
    calls = ["".join([rng.choice(["K", "W", "N", "G", "DL", "JA"]), str(rng.integers(0, 10))] + list(rng.choice(list(LETTERS), size=3))) for _ in range(400)]
    longs = [p + c for p, c in zip(rng.choice(["PJ4/", "KH1/", "VP2E/"], size=100), calls[:100])]
    pool = []
    for k in range(2000):
        a, b, l = calls[rng.integers(0, 400)], calls[rng.integers(0, 400)], longs[rng.integers(0, 100)]
        text = [f"CQ {a} FN42", f"{a} {b} -07", f"{a} {b} RR73", f"<{l}> {a} R-12", f"<{a}> {l} RRR", f"CQ {l}"][k % 6]
        shown = text
        for call in (l, a):
            shown = shown.replace(f"<{call}>", "<...>")
        pool.append((ft8.pack77(text), shown.encode()))
    msgs = np.zeros((FRAMES, ft8.MAX_MESSAGES), ft8.MESSAGE_DTYPE)
    pick = rng.integers(0, len(pool), (FRAMES, RECORDS))
    for f in range(FRAMES):
        for k in range(RECORDS):
            p, shown = pool[pick[f, k]]
            msgs[f, k]["a91"][:10] = p
            msgs[f, k]["text"] = shown
    return msgs, np.full(FRAMES, RECORDS, np.int32)


def timed(run, sync, steps):
    for _ in range(3):
        run()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    sync()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    build_id = ft8.check_build_id()
    out = {"what": "cost of the call hash table on one MI355X (tools/bench_callhash.py)", "build_id": build_id, "frames": FRAMES,
           "records_per_frame": RECORDS, "steps": args.steps, "rounds": args.rounds, "stage": [], "whole_path": None}
    with ft8.Decoder(device=0, max_frames=FRAMES) as dec:
        msgs, n_msgs = make_records(ft8)
        msgs_d = torch.from_numpy(msgs.view(np.uint8).reshape(-1)).cuda()
        n_d = torch.from_numpy(n_msgs).cuda()
        res_d = torch.zeros((FRAMES * ft8.MAX_MESSAGES * 48,), dtype=torch.uint8, device="cuda")
        for R, S in LAYOUTS:
            state_d = torch.zeros((R * ft8.CALLHASH_STATE_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ms = [timed(lambda: dec.resolve_calls_dev(msgs_d, n_d, R, S, state_d, 0, res_d), dec.synchronize, args.steps) for _ in range(args.rounds)]
            res = res_d.cpu().numpy().view(ft8.RESOLVED_DTYPE).reshape(FRAMES, ft8.MAX_MESSAGES)[:, :RECORDS]
            out["stage"].append({"receivers": R, "slots": S, "ms": [round(x, 4) for x in ms], "best_ms": round(min(ms), 4),
                                 "us_per_slot_of_a_receiver": round(1e3 * min(ms) / S, 3),
                                 "hashed_fields": int(res["n_hashed"].sum()), "resolved_fields": int(res["n_resolved"].sum()),
                                 "digest": hashlib.sha256(res.tobytes()).hexdigest()[:16]})
            del state_d
        # the whole path against the entry it wraps
        _, tones = workload.message_pool()
        sig, _ = workload.frame_signals(0, FRAMES, 20, tones, snr_range=(-18.0, 0.0))
        iq = torch.empty((FRAMES, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, FRAMES, 20, 1.0, workload.SEED_BASE, iq)
        R, S = 256, 16
        m0 = torch.zeros((FRAMES * ft8.MAX_MESSAGES * 64,), dtype=torch.uint8, device="cuda")
        m1, k0, k1 = torch.zeros_like(m0), torch.zeros((FRAMES,), dtype=torch.int32, device="cuda"), torch.zeros((FRAMES,), dtype=torch.int32, device="cuda")
        state_d = torch.zeros((R * ft8.CALLHASH_STATE_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plain, resolved = [], []
        for _ in range(args.rounds):
            plain.append(timed(lambda: dec.decode_messages_dev(iq, FRAMES, m0, k0), dec.synchronize, args.steps))
            resolved.append(timed(lambda: dec.decode_messages_resolved_dev(iq, R, S, state_d, 0, m1, k1, res_d), dec.synchronize, args.steps))
        same = bool(torch.equal(m0, m1) and torch.equal(k0, k1))
        out["whole_path"] = {"receivers": R, "slots": S, "decode_messages_ms": [round(x, 4) for x in plain],
                             "decode_messages_resolved_ms": [round(x, 4) for x in resolved],
                             "best_decode_messages_ms": round(min(plain), 4), "best_decode_messages_resolved_ms": round(min(resolved), 4),
                             "messages": int(k0.sum().item()), "msgs_and_counts_equal": same}
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if out["whole_path"]["msgs_and_counts_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
