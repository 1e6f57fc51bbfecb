#!/usr/bin/env python3
"""Cost of matching against expected messages (ft8gpu_match_candidates, ft8gpu_decode_messages_expected), measured on the GPU
in one session, device pointers, on 4096 frames of the bench workload (20 signals, -18 .. 0 dB, cap 120).

  python tools/bench_match.py [--json profiles/match_bench.json] [--steps 20] [--rounds 3]

  stage   ft8gpu_match_candidates (pre-kernel + match launch) on the batch's own BP status records with 20 / 64 / 512 live
          entries per table, against the LDPC launch (ft8gpu_decode_candidates) of the same batch, the arms interleaved round by
          round.  "prekernel" is the same entry with every count zero: the match launch leaves at once, what remains is the
          encoding of the 4096 tables.  The tables hold random type 1 payloads, the same in every frame.
  whole   ft8gpu_decode_messages_expected laid out 4096 x 1, 256 x 16 and 16 x 256 (receivers x slots) against
          ft8gpu_decode_messages on the same frames, interleaved; the count after BP must equal ft8gpu_decode_messages' count.
Time = host clock around `steps` calls that end in a synchronise, best of `rounds`.  A machine without a GPU fails at
ft8gpu_create; nothing is estimated."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES, CAP = 4096, 120
LIVE = (20, 64, 512)
LAYOUTS = ((4096, 1), (256, 16), (16, 256))


def random_table(ft8, nlive, seed):
    """one EXPECT_STATE_DTYPE table with nlive live entries spread over the ring: type 1 payloads with random standard calls"""
    rng = np.random.default_rng(seed)
    st = ft8.expect_state(1)
    for j in np.sort(rng.permutation(ft8.EXPECT_ENTRIES)[:nlive]):
        n28a, n28b = (int(x) for x in rng.integers(2063592 + 4194304, 1 << 28, 2))
        v = ((((n28a << 1) << 29 | (n28b << 1)) << 1) << 15 | int(rng.integers(0, 32400))) << 3 | 1
        st[0]["entry"]["payload"][j] = np.frombuffer((v << 3).to_bytes(10, "big"), np.uint8)
        st[0]["entry"]["used"][j] = 1
    st[0]["cursor"] = nlive
    return st


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
    gate = ft8.MATCH_MAX_HARD_ERRORS
    out = {"what": "cost of matching against expected messages on one MI355X (tools/bench_match.py)", "build_id": build_id, "frames": FRAMES,
           "max_candidates": CAP, "gate": gate, "steps": args.steps, "rounds": args.rounds, "stage": {}, "whole_path": []}
    with ft8.Decoder(device=0, max_frames=FRAMES, max_candidates=CAP) as dec:
        _, tones = workload.message_pool()
        sig, _ = workload.frame_signals(0, FRAMES, 20, tones, snr_range=(-18.0, 0.0))
        iq = torch.empty((FRAMES, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, FRAMES, 20, 1.0, workload.SEED_BASE, iq)
        u8 = lambda n: torch.zeros((n,), dtype=torch.uint8, device="cuda")
        mag, cands, status = u8(FRAMES * ft8.MAG_ARRAY), u8(FRAMES * CAP * 8), u8(FRAMES * CAP * 48)
        counts = torch.zeros((FRAMES,), dtype=torch.int32, device="cuda")
        zero_counts = torch.zeros_like(counts)
        dec.waterfall_dev(iq, FRAMES, mag)
        dec.find_sync_dev(mag, FRAMES, cands, counts)
        dec.decode_candidates_dev(mag, cands, counts, FRAMES, status)
        dec.synchronize()
        st = status.cpu().numpy().view(ft8.STATUS_DTYPE).reshape(FRAMES, CAP)
        k = counts.cpu().numpy()
        live_rec = np.arange(CAP)[None, :] < k[:, None]
        failing = int(((st["ok"] == 0) & (st["ldpc_errors"] != 0) & live_rec).sum())
        out["candidates"] = int(k.sum())
        out["failing_candidates"] = failing
        status_out, info = u8(FRAMES * CAP * 48), u8(FRAMES * CAP * 8)
        tables = {n: torch.from_numpy(np.tile(random_table(ft8, n, 0x7AB + n).view(np.uint8).reshape(-1), FRAMES)).cuda() for n in LIVE}
        torch.cuda.synchronize()
        arms = {"ldpc": lambda: dec.decode_candidates_dev(mag, cands, counts, FRAMES, status_out),
                "prekernel": lambda: dec.match_candidates_dev(mag, cands, zero_counts, status, FRAMES, tables[512], 0, gate, status_out, info)}
        for n in LIVE:
            arms["match_%d_live" % n] = (lambda t: lambda: dec.match_candidates_dev(mag, cands, counts, status, FRAMES, t, 0, gate, status_out, info))(tables[n])
        ms = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, run in arms.items():
                ms[name].append(timed(run, dec.synchronize, args.steps))
        for name in arms:
            out["stage"][name] = {"ms": [round(x, 4) for x in ms[name]], "best_ms": round(min(ms[name]), 4)}
        for n in LIVE:
            arms["match_%d_live" % n]()
            dec.synchronize()
            inf = info.cpu().numpy().view(ft8.MATCH_INFO_DTYPE).reshape(FRAMES, CAP)
            out["stage"]["match_%d_live" % n].update(compared=int(((inf["result"] != 0) & live_rec).sum()), accepted=int(((inf["result"] == 1) & live_rec).sum()),
                                                     digest=hashlib.sha256(inf[live_rec].tobytes()).hexdigest()[:16])
        del tables, status_out, info, mag, cands, status
        # the whole path against ft8gpu_decode_messages
        m0 = u8(FRAMES * ft8.MAX_MESSAGES * 64)
        m1, k0, k1 = torch.zeros_like(m0), torch.zeros_like(counts), torch.zeros_like(counts)
        nbs = torch.zeros((FRAMES, 2), dtype=torch.int32, device="cuda")
        for R, S in LAYOUTS:
            state = u8(R * ft8.EXPECT_STATE_DTYPE.itemsize)
            torch.cuda.synchronize()
            plain, expected = [], []
            for _ in range(args.rounds):
                plain.append(timed(lambda: dec.decode_messages_dev(iq, FRAMES, m0, k0), dec.synchronize, args.steps))
                expected.append(timed(lambda: dec.decode_messages_expected_dev(iq, R, S, state, gate, 0, 1, m1, k1, nbs), dec.synchronize, args.steps))
            h = nbs.cpu().numpy()
            out["whole_path"].append({"receivers": R, "slots": S, "decode_messages_ms": [round(x, 4) for x in plain],
                                      "decode_messages_expected_ms": [round(x, 4) for x in expected],
                                      "best_decode_messages_ms": round(min(plain), 4), "best_decode_messages_expected_ms": round(min(expected), 4),
                                      "messages_after_bp": int(h[:, 0].sum()), "messages_after_matching": int(h[:, 1].sum()),
                                      "bp_counts_equal": bool(np.array_equal(h[:, 0], k0.cpu().numpy()))})
            del state
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if all(w["bp_counts_equal"] for w in out["whole_path"]) else 1


if __name__ == "__main__":
    sys.exit(main())
