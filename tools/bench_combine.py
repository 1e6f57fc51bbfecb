#!/usr/bin/env python3
"""Cost of the soft-bit memory (ft8gpu_combine_candidates, ft8gpu_softmem_update, ft8gpu_decode_messages_combined), measured on
the GPU in one session, device pointers, on 4096 frames of the bench workload (20 signals, -18 .. 0 dB, cap 120).

  python tools/bench_combine.py [--json profiles/combine_bench.json] [--steps 20] [--rounds 3]

  stage   ft8gpu_combine_candidates on the batch's own BP status records against the LDPC launch (ft8gpu_decode_candidates) of
          the same batch, the arms interleaved round by round: "empty" memories (every failing candidate leaves after the
          partner search), "self" memories -- what ft8gpu_softmem_update stores from this very batch at store_per_slot 128 and
          at the recommended value, so that every stored candidate finds itself as a partner and BP runs on it: the bound of
          one BP run per failing candidate, reached.  "update" is ft8gpu_softmem_update alone.  The ratio of
          every arm to the LDPC launch is reported.
  whole   ft8gpu_decode_messages_combined laid out 4096 x 1, 256 x 16 and 16 x 256 (receivers x slots) against
          ft8gpu_decode_messages on the same frames, interleaved; the count after BP must equal ft8gpu_decode_messages' count.
          The memories carry on from call to call, so the 4096 x 1 layout meets the same frames again: BP runs on every
          stored candidate.
Time = host clock around `steps` calls that end in a synchronise, after three warm-up calls, best of `rounds`.  A machine
without a GPU fails at ft8gpu_create; nothing is estimated."""
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
LAYOUTS = ((4096, 1), (256, 16), (16, 256))


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
    gate, store = ft8.COMBINE_MIN_AGREE, ft8.COMBINE_STORE_PER_SLOT
    SB = ft8.SOFTMEM_STATE_DTYPE.itemsize
    out = {"what": "cost of the soft-bit memory on one MI355X (tools/bench_combine.py)", "build_id": build_id, "frames": FRAMES,
           "max_candidates": CAP, "min_agree": gate, "store_per_slot": store, "steps": args.steps, "rounds": args.rounds, "stage": {},
           "whole_path": []}
    with ft8.Decoder(device=0, max_frames=FRAMES, max_candidates=CAP) as dec:
        _, tones = workload.message_pool()
        sig, _ = workload.frame_signals(0, FRAMES, 20, tones, snr_range=(-18.0, 0.0))
        iq = torch.empty((FRAMES, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, FRAMES, 20, 1.0, workload.SEED_BASE, iq)
        u8 = lambda n: torch.zeros((n,), dtype=torch.uint8, device="cuda")
        mag, cands, status = u8(FRAMES * ft8.MAG_ARRAY), u8(FRAMES * CAP * 8), u8(FRAMES * CAP * 48)
        counts = torch.zeros((FRAMES,), dtype=torch.int32, device="cuda")
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
        status_out, info, zero_info = u8(FRAMES * CAP * 48), u8(FRAMES * CAP * 8), u8(FRAMES * CAP * 8)
        mem = {"empty": u8(FRAMES * SB)}
        for name, n in (("self_128", 128), ("self_%d" % store, store)):
            mem[name] = u8(FRAMES * SB)
            dec.softmem_update_dev(mag, cands, counts, status, zero_info, FRAMES, mem[name], n)
        dec.synchronize()
        scratch = u8(FRAMES * SB)
        arms = {"ldpc": lambda: dec.decode_candidates_dev(mag, cands, counts, FRAMES, status_out)}
        for name, m in mem.items():
            arms["combine_" + name] = (lambda t: lambda: dec.combine_candidates_dev(mag, cands, counts, status, FRAMES, t, 0, gate, status_out, info))(m)
        arms["update_%d" % store] = lambda: dec.softmem_update_dev(mag, cands, counts, status, zero_info, FRAMES, scratch, store)
        ms = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, run in arms.items():
                ms[name].append(timed(run, dec.synchronize, args.steps))
        for name in arms:
            out["stage"][name] = {"ms": [round(x, 4) for x in ms[name]], "best_ms": round(min(ms[name]), 4)}
        ldpc = out["stage"]["ldpc"]["best_ms"]
        for name in arms:
            out["stage"][name]["ratio_to_ldpc_launch"] = round(out["stage"][name]["best_ms"] / ldpc, 4)
        for name in [n for n in arms if n.startswith("combine_")]:
            arms[name]()
            dec.synchronize()
            inf = info.cpu().numpy().view(ft8.COMBINE_INFO_DTYPE).reshape(FRAMES, CAP)
            r = inf["result"][live_rec]
            out["stage"][name].update(bp_runs=int(np.isin(r, (1, 3, 4, 5, 7)).sum()), accepted=int((r == 1).sum()), gated=int((r == 8).sum()),
                                      digest=hashlib.sha256(inf[live_rec].tobytes()).hexdigest()[:16])
        del mem, scratch, status_out, info, zero_info, mag, cands, status
        # the whole path against ft8gpu_decode_messages
        m0 = u8(FRAMES * ft8.MAX_MESSAGES * 64)
        m1, k0, k1 = torch.zeros_like(m0), torch.zeros_like(counts), torch.zeros_like(counts)
        nbs = torch.zeros((FRAMES, 2), dtype=torch.int32, device="cuda")
        for R, S in LAYOUTS:
            state = u8(R * SB)
            torch.cuda.synchronize()
            plain, combined = [], []
            for _ in range(args.rounds):
                plain.append(timed(lambda: dec.decode_messages_dev(iq, FRAMES, m0, k0), dec.synchronize, args.steps))
                combined.append(timed(lambda: dec.decode_messages_combined_dev(iq, R, S, state, gate, 0, store, m1, k1, nbs), dec.synchronize, args.steps))
            h = nbs.cpu().numpy()
            out["whole_path"].append({"receivers": R, "slots": S, "decode_messages_ms": [round(x, 4) for x in plain],
                                      "decode_messages_combined_ms": [round(x, 4) for x in combined],
                                      "best_decode_messages_ms": round(min(plain), 4), "best_decode_messages_combined_ms": round(min(combined), 4),
                                      "messages_after_bp": int(h[:, 0].sum()), "messages_after_combining": int(h[:, 1].sum()),
                                      "bp_counts_equal": bool(np.array_equal(h[:, 0], k0.cpu().numpy()))})
            del state
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if all(w["bp_counts_equal"] for w in out["whole_path"]) else 1


if __name__ == "__main__":
    sys.exit(main())
