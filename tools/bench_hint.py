#!/usr/bin/env python3
"""Cost of the call hints (ft8gpu_hint_candidates, ft8gpu_hint_update, ft8gpu_decode_messages_hinted), measured on the GPU in
one session, device pointers, on 4096 frames of the bench workload (20 signals, -18 .. 0 dB, cap 120).

  python tools/bench_hint.py [--json profiles/hint_bench.json] [--steps 20] [--rounds 3]

  stage   ft8gpu_hint_candidates on the batch's own BP status records with empty, 64-entry and 512-entry tables (entries of
          every kind from random calls, the same in every frame) at tries 1 and 4, against the LDPC launch
          (ft8gpu_decode_candidates) and ft8gpu_ap_candidates with 1 and 4 hypotheses on the same batch, the arms interleaved
          round by round, at the preselection gates 16 and FT8GPU_HINT_MAX_BAD_PER_64 and the recommended hard-error gate.
          Every hint arm runs in both forms of the table words: the product's (a pre-kernel encodes the tables once per
          frame and call into a scratch block) and, through the A/B build with FT8GPU_AB_HINT_IN_WAVE, the form that converts
          the entries in the wave; the info records of the two forms must be equal.
  update  ft8gpu_hint_update over the records of ft8gpu_decode_messages laid out 256 x 16.
  whole   ft8gpu_decode_messages_hinted (recommended constants) laid out 4096 x 1 and 256 x 16 (receivers x slots) against
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
ENTRIES = (0, 64, 512)
LAYOUTS = ((4096, 1), (256, 16))
AP_HYPS = ("CQ ? ?", "CQ DX ? ?", "CQ POTA ? ?", "K1ABC ? ?")


def random_table(ft8, n, seed):
    """one HINT_STATE_DTYPE table with n live entries spread over the ring: every kind, fields of random standard calls"""
    rng = np.random.default_rng(seed)
    st = ft8.hint_state(1)
    for j in np.sort(rng.permutation(ft8.HINT_ENTRIES)[:n]):
        a, b = (int(x) << 1 for x in rng.integers(2063592 + 4194304, 1 << 28, 2))
        kind = int(rng.integers(1, 4))
        st[0]["entry"][j] = (a if kind & 1 else 0, b if kind & 2 else 0, 0, kind, 1, 0, 0)
    st[0]["cursor"] = n
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
    gates, hard, rec_tries = (16, ft8.HINT_MAX_BAD_PER_64), ft8.HINT_MAX_HARD_ERRORS, ft8.HINT_TRIES
    out = {"what": "cost of the call hints on one MI355X (tools/bench_hint.py)", "build_id": build_id, "frames": FRAMES, "max_candidates": CAP,
           "gates": gates, "max_hard_errors": hard, "steps": args.steps, "rounds": args.rounds, "stage": {}, "whole_path": []}
    with ft8.Decoder(device=0, max_frames=FRAMES, max_candidates=CAP) as dec, \
            ft8.Decoder(device=0, max_frames=FRAMES, max_candidates=CAP, lib=ft8.load_ab_library()) as dec_ab:
        dec_ab.set_debug_flags(ft8.AB_HINT_IN_WAVE)
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
        out["candidates"] = int(k.sum())
        out["failing_candidates"] = int(((st["ok"] == 0) & (st["ldpc_errors"] != 0) & live_rec).sum())
        status_out, info, ap_info = u8(FRAMES * CAP * 48), u8(FRAMES * CAP * 16), u8(FRAMES * CAP * 8)
        tables = {n: torch.from_numpy(np.tile(random_table(ft8, n, 0x417 + n).view(np.uint8).reshape(-1), FRAMES)).cuda() for n in ENTRIES}
        torch.cuda.synchronize()
        arms = {"ldpc": lambda: dec.decode_candidates_dev(mag, cands, counts, FRAMES, status_out)}
        for nh in (1, 4):
            arms["ap_%d_hyp" % nh] = (lambda h: lambda: dec.ap_candidates_dev(mag, cands, counts, status, FRAMES, h, hard, status_out, ap_info))(AP_HYPS[:nh])
        for gate in gates:
            for n in ENTRIES:
                for tries in (1, 4):
                    for form, d in (("", dec), ("_in_wave", dec_ab)):
                        arms["hint_gate_%d_%d_entries_tries_%d%s" % (gate, n, tries, form)] = (lambda d, t, tr, g: lambda: d.hint_candidates_dev(
                            mag, cands, counts, status, FRAMES, t, tr, g, hard, 0, 0, status_out, info))(d, tables[n], tries, gate)
        ms = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, run in arms.items():
                ms[name].append(timed(run, (dec_ab if name.endswith("_in_wave") else dec).synchronize, args.steps))
        for name in arms:
            out["stage"][name] = {"ms": [round(x, 4) for x in ms[name]], "best_ms": round(min(ms[name]), 4)}
        for name in arms:
            if not name.startswith("hint_"):
                continue
            arms[name]()
            (dec_ab if name.endswith("_in_wave") else dec).synchronize()
            inf = info.cpu().numpy().view(ft8.HINT_INFO_DTYPE).reshape(FRAMES, CAP)
            out["stage"][name].update(candidates_with_a_passing_entry=int(((inf["ntried"] != 0) & live_rec).sum()),
                                      tries=int(inf["ntried"][live_rec].sum()), accepted=int(((inf["result"] == 1) & live_rec).sum()),
                                      digest=hashlib.sha256(inf[live_rec].tobytes()).hexdigest()[:16])
        forms_equal = all(out["stage"][n]["digest"] == out["stage"][n + "_in_wave"]["digest"] for n in arms if n.startswith("hint_") and not n.endswith("_in_wave"))
        out["forms_equal"] = forms_equal
        del tables, status_out, info, ap_info, mag, cands, status
        # the whole path against ft8gpu_decode_messages, and the update alone
        m0 = u8(FRAMES * ft8.MAX_MESSAGES * 64)
        m1, k0, k1 = torch.zeros_like(m0), torch.zeros_like(counts), torch.zeros_like(counts)
        nbs = torch.zeros((FRAMES, 2), dtype=torch.int32, device="cuda")
        for R, S in LAYOUTS:
            state = u8(R * ft8.HINT_STATE_DTYPE.itemsize)
            torch.cuda.synchronize()
            plain, hinted = [], []
            for _ in range(args.rounds):
                plain.append(timed(lambda: dec.decode_messages_dev(iq, FRAMES, m0, k0), dec.synchronize, args.steps))
                hinted.append(timed(lambda: dec.decode_messages_hinted_dev(iq, R, S, state, rec_tries, gates[1], hard, 0, 1, m1, k1, nbs), dec.synchronize, args.steps))
            h = nbs.cpu().numpy()
            out["whole_path"].append({"receivers": R, "slots": S, "tries": rec_tries, "max_bad_per_64": gates[1], "decode_messages_ms": [round(x, 4) for x in plain],
                                      "decode_messages_hinted_ms": [round(x, 4) for x in hinted],
                                      "best_decode_messages_ms": round(min(plain), 4), "best_decode_messages_hinted_ms": round(min(hinted), 4),
                                      "messages_after_bp": int(h[:, 0].sum()), "messages_after_hints": int(h[:, 1].sum()),
                                      "bp_counts_equal": bool(np.array_equal(h[:, 0], k0.cpu().numpy()))})
            if S == 16:
                upd = [timed(lambda: dec.hint_update_dev(m0, k0, R, S, state), dec.synchronize, args.steps) for _ in range(args.rounds)]
                out["update"] = {"receivers": R, "slots": S, "ms": [round(x, 4) for x in upd], "best_ms": round(min(upd), 4)}
            del state
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if all(w["bp_counts_equal"] for w in out["whole_path"]) and forms_equal else 1


if __name__ == "__main__":
    sys.exit(main())
