#!/usr/bin/env python3
"""What the call hints gain and what they accept wrongly (ft8gpu_decode_messages_hinted), swept over the preselection gate,
the number of tries and the hard-error gate on one GPU.

  python tools/hint_gain.py [--json profiles/hint_gain.json] [--receivers 96]

Rows (receivers x 4 slots each, the device's own synthesiser, signals at random audio frequencies and clock offsets, -24 .. 0 dB):
  qso_20, qso_30          20 / 30 QSOs per receiver that advance one step per slot (CQ, call, report, R-report, RR73; QSO k starts
                          at step k % 2), the receivers' tables start empty and are filled by the update rule alone
  qso_20_u, qso_30_u      the same frames, every table pre-filled with 236 entries from unrelated calls (all kinds, both phases)
  noise                   4 x receivers frames without signals against full tables (512 unrelated entries), one slot
Per row and parameter set: planted messages gained over BP (a gained record whose text was sent in that frame), wrong
acceptances (any other gained record), and for the last slot the tries per failing candidate (the stage entry on that slot's
frames against the state the first three slots left).  The same frames run through "CQ ? ?" a-priori decoding
(ft8gpu_decode_messages_ap, one pass, no OSD) and through matching with derive (ft8gpu_decode_messages_expected) at their
recommended gates.  "recommended" is the parameter set with the largest gain over the QSO rows among those that accept
nothing wrong on any row; ties go to fewer tries, then to the smaller gates."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SLOTS = 4
GATES = (8, 12, 16, 20, 24)
TRIES = (1, 2, 4)
HARD = (30, 40, 50, 174)
CALL_PREFIX = ("K", "W", "N", "G", "F", "DL", "JA", "VK", "EA", "OH", "SM", "PY", "ZL", "I", "VE", "LU")
LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"


def random_call(rng):
    return str(rng.choice(CALL_PREFIX)) + str(rng.integers(0, 10)) + "".join(rng.choice(list(LETTERS), size=int(rng.integers(1, 4))))


def random_grid(rng):
    return LETTERS[rng.integers(0, 18)] + LETTERS[rng.integers(0, 18)] + str(rng.integers(0, 10)) + str(rng.integers(0, 10))


def qso_step(a, b, grid, rpt, step):
    return (f"CQ {a} {grid[0]}", f"{a} {b} {grid[1]}", f"{b} {a} {rpt[0]}", f"{a} {b} R{rpt[1]}", f"{b} {a} RR73")[step]


def field_of(ft8, call):
    """the 29-bit field of a standard call in clear"""
    p = ft8.pack77(f"{call} {call} RRR")
    return (int.from_bytes(bytes(bytearray(p[:10])), "big") >> 3) >> 48


def qso_frames(ft8, workload, dec, R, nsig, seed):
    """(iq device tensor [R][SLOTS][2][48000], texts [R][SLOTS])"""
    import torch
    sig = np.zeros((R, SLOTS, nsig), ft8.SIGNAL_DTYPE)
    texts = [[None] * SLOTS for _ in range(R)]
    for r in range(R):
        rng = np.random.default_rng(seed + r)
        pairs = []
        while len(pairs) < nsig:
            a, b = random_call(rng), random_call(rng)
            if a != b:
                pairs.append((a, b))
        grids = [(random_grid(rng), random_grid(rng)) for _ in range(nsig)]
        rpts = [("%+03d" % rng.integers(-24, 10), "%+03d" % rng.integers(-24, 10)) for _ in range(nsig)]
        f0 = rng.uniform(100.0, 1450.0, nsig)
        t0 = rng.uniform(0.0, 1.8, nsig)
        for s in range(SLOTS):
            tx = [qso_step(*pairs[k], grids[k], rpts[k], (k % 2) + s) for k in range(nsig)]
            texts[r][s] = tx
            for k, t in enumerate(tx):
                sig[r, s, k]["tones"] = ft8.encode(ft8.pack77(t))
            sig[r, s]["f0_hz"], sig[r, s]["t0_s"] = f0, t0
            sig[r, s]["amplitude"] = workload.amplitude_for_snr(rng.uniform(-24.0, 0.0, nsig))
    iq = torch.empty((R * SLOTS, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
    dec.synth_frames(sig.reshape(-1), R * SLOTS, nsig, 1.0, seed, iq)
    dec.synchronize()
    return iq, texts


def unrelated_tables(ft8, R, n, seed):
    rng = np.random.default_rng(seed)
    st = ft8.hint_state(R)
    pool = [field_of(ft8, random_call(rng)) for _ in range(400)]
    for r in range(R):
        e = st[r]["entry"]
        for j in rng.permutation(ft8.HINT_ENTRIES)[:n]:
            kind = int(rng.integers(1, 4))
            a, b = (pool[int(x)] for x in rng.integers(0, len(pool), 2))
            e[j] = (a if kind & 1 else 0, b if kind & 2 else 0, 0, kind, 1, int(rng.integers(0, 2)), 0)
        st[r]["cursor"] = n
    return st


def tally(msgs, nbs, texts):
    good = bad = 0
    wrong = []
    R, S = nbs.shape[:2]
    for r in range(R):
        for s in range(S):
            for k in range(int(nbs[r, s, 0]), int(nbs[r, s, -1])):
                t = msgs[r, s, k]["text"].decode()
                if t in texts[r][s]:
                    good += 1
                else:
                    bad += 1
                    wrong.append(t)
    return good, bad, wrong


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--receivers", type=int, default=96)
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    R = args.receivers
    out = {"what": "call hints: planted messages gained over BP and wrong acceptances on one MI355X (tools/hint_gain.py)",
           "build_id": ft8.check_build_id(), "receivers": R, "slots": SLOTS, "snr_db": [-24.0, 0.0], "max_age": 0, "use_phase": 1,
           "gates": GATES, "tries": TRIES, "max_hard_errors": HARD, "rows": {}}
    with ft8.Decoder(device=0, max_frames=R * SLOTS, max_candidates=120) as dec:
        rows = []
        for nsig in (20, 30):
            iq, texts = qso_frames(ft8, workload, dec, R, nsig, 910000 + 1000 * nsig)
            rows.append((f"qso_{nsig}", iq.cpu().numpy().reshape(R, SLOTS, 2, -1), texts, None))
            rows.append((f"qso_{nsig}_u", rows[-1][1], texts, unrelated_tables(ft8, R, 236, 77 + nsig)))
        NR = R * SLOTS                                                   # as many noise frames as a QSO row has frames
        noise = torch.empty((NR, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(np.zeros(NR, ft8.SIGNAL_DTYPE), NR, 1, 1.0, 920000, noise)   # one signal of amplitude 0: noise alone
        dec.synchronize()
        rows.append(("noise", noise.cpu().numpy().reshape(NR, 1, 2, -1), [[[]] for _ in range(NR)], unrelated_tables(ft8, NR, 512, 99)))
        for name, iq, texts, st0 in rows:
            R, S = iq.shape[:2]
            row = {"frames": R * S, "sweep": []}
            plain, pn = dec.decode_messages(iq.reshape(R * S, 2, -1))
            sent = sum(len(texts[r][s]) for r in range(R) for s in range(S))
            row["sent"], row["bp_records"] = sent, int(pn.sum())
            row["bp_planted"] = int(sum(plain[f, k]["text"].decode() in texts[f // S][f % S] for f in range(R * S) for k in range(int(pn[f]))))
            if name.startswith("qso") and st0 is None:
                m, n, nbs = dec.decode_messages_ap(iq.reshape(R * S, 2, -1), 1, ("CQ ? ?",), ft8.AP_MAX_HARD_ERRORS, -1)
                g, b, _w = tally(m.reshape(R, S, 50), nbs.reshape(R, S, 3)[:, :, :2], texts)
                row["ap_cq"] = {"gained": g, "wrong": b}
                m, n, nbs, _st = dec.decode_messages_expected(iq, None, ft8.MATCH_MAX_HARD_ERRORS, 0, True)
                g, b, _w = tally(m, nbs, texts)
                row["match_derive"] = {"gained": g, "wrong": b}
            # the last slot's candidates, for the tries per failing candidate
            last = np.ascontiguousarray(iq[:, S - 1])
            mag = dec.waterfall(last)
            cands, counts = dec.find_sync(mag)
            status = dec.decode_candidates(mag, cands, counts)
            live = np.arange(cands.shape[1])[None, :] < counts[:, None]
            failing = int(((status["ok"] == 0) & (status["ldpc_errors"] != 0) & live).sum())
            row["last_slot_failing_candidates"] = failing
            for hard in HARD:
                for gate in GATES:
                    for tries in TRIES:
                        m, n, nbs, st = dec.decode_messages_hinted(iq, tries, gate, hard, st0, 0, True)
                        g, b, w = tally(m, nbs, texts)
                        rec = {"max_bad_per_64": gate, "tries": tries, "max_hard_errors": hard, "gained": g, "wrong": b, "wrong_texts": w[:8]}
                        if hard == HARD[-1]:
                            before = st0 if S == 1 else dec.decode_messages_hinted(np.ascontiguousarray(iq[:, :S - 1]), tries, gate, hard, st0, 0, True)[3]
                            if before is None:
                                before = ft8.hint_state(R)
                            _o, info = dec.hint_candidates(mag, cands, counts, status, before, tries, gate, hard, 0, True)
                            rec["last_slot_tries_per_failing_candidate"] = round(float(info["ntried"][live].sum()) / max(failing, 1), 4)
                        row["sweep"].append(rec)
            out["rows"][name] = row
            print(name, {k: v for k, v in row.items() if k != "sweep"}, file=sys.stderr)
    # the recommendation: nothing wrong on any row, the largest gain on the QSO rows
    best = None
    for hard in HARD:
        for gate in GATES:
            for tries in TRIES:
                recs = {name: next(x for x in row["sweep"] if (x["max_bad_per_64"], x["tries"], x["max_hard_errors"]) == (gate, tries, hard))
                        for name, row in out["rows"].items()}
                if any(x["wrong"] for x in recs.values()):
                    continue
                gain = sum(x["gained"] for name, x in recs.items() if name.startswith("qso"))
                key = (-gain, tries, gate, hard)
                if best is None or key < best[0]:
                    best = (key, {"max_bad_per_64": gate, "tries": tries, "max_hard_errors": hard, "gained_on_qso_rows": gain})
    out["recommended"] = best[1] if best else None
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
