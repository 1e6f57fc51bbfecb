"""What matching against expected messages gains and what it risks, on the CPU with the oracle's stages and the numpy
restatement of the rule (tests/ft8_spec_match.py).  A gate sweep (the largest number of hard errors accepted) over 30..60:
  (a) cq20, cq30  96 CQ frames (tests/synth_util.make_frame, seeds 1000.., 20 / 30 signals at U[-22, 0] dB: the frames of
                  profiles/ap_gain.json) with the frame's planted messages and 236 unrelated CQ messages in the table;
  (b) sibling     48 two-call frames (seeds 2000.., 20 signals, cq_fraction 0) whose table holds four siblings of every planted
                  message (the same calls with RRR, RR73, 73 and -10) but never the message itself: every acceptance is wrong;
  (c) noise       96 noise-only frames (seeds 5000..) against 256 unrelated CQ messages;
  (d) stream      slot sequences under the real update rule (ft8gpu_decode_messages_expected's restatement), derive 0 and 1:
                  a strong slot (20 stations at U[-12, 0] dB, half CQ), an unrelated slot, then the first slot's stations again
                  at the same frequencies 6 / 10 / 14 dB weaker with a quarter of them replaced by new stations.
Per row and gate: planted messages gained over belief propagation (unique, as the append step counts them) and every accepted
message that was not on the air; for (a) - (c) also the hard errors of the wrong best entries, so that the largest gate that
accepts nothing wrong can be read off.  Cap 120, min_score 10, 20 iterations.

  python tools/match_gain.py [--frames 96] [--procs 8] [--out profiles/match_gain.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GATES = list(range(30, 61))
UNRELATED = 236
SIBLINGS = ("RRR", "RR73", "73", "-10")
STREAM_DROPS = (6.0, 10.0, 14.0)


def table_of(payloads, seed):
    import numpy as np
    import ft8_spec_match as smt
    import match_craft as mc
    rng = np.random.default_rng(seed)
    st = smt.new_state()
    for j, p in zip(rng.permutation(smt.ENTRIES)[:len(payloads)], payloads):
        mc.put(st[0], int(j), p)
    return st


def static_frame(job):
    """rows (a) - (c): one frame against one table -> BP's planted decodes, and per failing candidate its best entry"""
    import numpy as np
    import oracle_lib
    import ft8_spec_match as smt
    import ft8_spec_messages as sm
    import match_craft as mc
    import rtlsdr_ft8d_amd as ft8
    import synth_util as S
    kind, seed, nsig, snr = job
    enc = S.oracle_encode_fn(oracle_lib)
    iq, planted = S.make_frame(seed, nsig, enc, snr_range=snr, cq_fraction=0.0 if kind == "sibling" else 1.0)
    rng = np.random.default_rng(0x7AB1E + seed)
    if kind == "sibling":
        payloads = [ft8.pack77(" ".join(t.split()[:2] + [s])) for t in planted for s in SIBLINGS]
    else:
        payloads = [ft8.pack77(t) for t in planted] + mc.unrelated_payloads(rng, UNRELATED if nsig else 256, planted)
    state = table_of(payloads, seed)
    want = set(planted)
    mag, cands, counts, status = sm.oracle_stages(oracle_lib, iq[None], 120, 10, 1)
    st = status.view(ft8.STATUS_DTYPE).reshape(1, -1)[0]
    n = int(counts[0])
    seen = []
    for i in range(n):
        if st[i]["ok"]:
            key = (int(st[i]["crc_extracted"]), bytes(st[i]["text"]))
            if key not in seen and len(seen) < 50:
                seen.append(key)
    bp_hit = sum(k[1].decode(errors="replace") in want for k in seen)
    idx, C = smt.table_codewords(state[0], 0)
    best = []                                            # (candidate, nhard, key, planted?)
    failing = 0
    for i in range(n):
        if st[i]["ok"] != 0 or st[i]["ldpc_errors"] == 0:
            continue
        failing += 1
        llr = oracle_lib.llr(mag[0], cands[0, i])
        if not np.isfinite(llr).all():
            continue
        metric, index, nhard, cw = smt.best_entry(llr, idx, C)
        code, crc, rc, text = smt.judge(oracle_lib, cw, nhard, 174)
        if code == 1:
            best.append((i, nhard, (crc, text), text.decode(errors="replace") in want))
    gates = {}
    for g in GATES:
        seen_g, new, wrong_msgs, wrong_cands = list(seen), 0, 0, 0
        for i, nhard, key, ok in best:
            if nhard > g:
                continue
            wrong_cands += not ok
            if key in seen_g or len(seen_g) >= 50:
                continue
            seen_g.append(key)
            new += ok
            wrong_msgs += not ok
        gates[g] = (new, wrong_msgs, wrong_cands)
    return dict(planted=len(want), bp_hit=bp_hit, failing=failing, gates=gates,
                wrong_nhard=sorted(nh for _i, nh, _k, ok in best if not ok), right_nhard=sorted(nh for _i, nh, _k, ok in best if ok))


def stream_sequence(job):
    """row (d): three slots of one receiver -> per gate the messages slot 2 gains over BP and what it accepts that was not on air"""
    import numpy as np
    import oracle_lib
    import ft8_spec_match as smt
    import ft8_spec_messages as sm
    import rtlsdr_ft8d_amd as ft8
    import synth_util as S
    seed, drop, derive = job
    rng = np.random.default_rng(31000 + seed)
    nsig = 20
    first = [S.random_message(rng, cq=k % 2 == 0) for k in range(nsig)]
    other = [S.random_message(rng, cq=k % 2 == 0) for k in range(nsig)]
    again = [S.random_message(rng, cq=k % 2 == 0) if k % 4 == 3 else first[k] for k in range(nsig)]       # a quarter are new stations
    f0, t0, snr = rng.uniform(100.0, 1500.0, nsig), rng.uniform(0.0, 1.8, nsig), rng.uniform(-12.0, 0.0, nsig)
    f1, t1, snr1 = rng.uniform(100.0, 1500.0, nsig), rng.uniform(0.0, 1.8, nsig), rng.uniform(-12.0, 0.0, nsig)
    iq = np.zeros((1, 3, 2, S.NSAMPLES), np.float32)
    for s, (texts, f, t, db) in enumerate(((first, f0, t0, snr), (other, f1, t1, snr1), (again, f0, t0, snr - drop))):
        noise = np.random.default_rng(41000 + 10 * seed + s)
        fi, fq = noise.normal(0.0, 1.0, S.NSAMPLES), noise.normal(0.0, 1.0, S.NSAMPLES)
        for k, text in enumerate(texts):
            si, sq = S.cpfsk(ft8.encode(ft8.pack77(text)), float(f[k]), int(round(t[k] * 3200)), S.amplitude_for_snr(float(db[k]), 1.0))
            fi += si
            fq += sq
        i32, q32 = fi.astype(np.float32), fq.astype(np.float32)
        scale = np.float32(0.5) / max(np.abs(i32).max(), np.abs(q32).max(), np.float32(1e-24))
        iq[0, s, 0], iq[0, s, 1] = i32 * scale, q32 * scale
    stages = sm.oracle_stages(oracle_lib, iq.reshape(3, 2, -1), 120, 10, 1)
    on_air = (set(first), set(other), set(again))
    out = {}
    for g in GATES:
        msgs, n, nbs, _state = smt.decode_expected(oracle_lib, iq, max_hard_errors=g, derive=bool(derive), stages=stages, nthreads=1)
        good = bad = 0
        for s in range(3):
            for k in range(int(nbs[0, s, 0]), int(n[0, s])):
                ok = msgs[0, s, k]["text"].decode(errors="replace") in on_air[s]
                good += ok
                bad += not ok
        out[g] = (good, bad)
    bp2 = sum(msgs[0, 2, k]["text"].decode(errors="replace") in on_air[2] for k in range(int(nbs[0, 2, 0])))
    return dict(gates=out, bp_slot2=bp2, repeated=sum(a == b for a, b in zip(first, again)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--sequences", type=int, default=24)
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_gain.json"))
    a = ap.parse_args()
    import multiprocessing as mp
    import oracle_lib
    oracle_lib.build()
    rows = []
    static = [("cq20", "cq", 20, (-22.0, 0.0), 1000, a.frames), ("cq30", "cq", 30, (-22.0, 0.0), 1000, a.frames),
              ("sibling", "sibling", 20, (-22.0, 0.0), 2000, a.frames // 2), ("noise", "cq", 0, (-22.0, 0.0), 5000, a.frames)]
    with mp.Pool(a.procs) as pool:
        for name, kind, nsig, snr, seed0, frames in static:
            t0 = time.time()
            per = pool.map(static_frame, [(kind, s, nsig, snr) for s in range(seed0, seed0 + frames)])
            wrong = sorted(x for p in per for x in p["wrong_nhard"])
            row = dict(name=name, signals_per_frame=nsig, snr_db=list(snr), seeds=[seed0, seed0 + frames - 1], frames=frames,
                       table="four siblings of every planted message, never the message" if kind == "sibling" else
                             ("the planted messages and %d unrelated CQ messages" % UNRELATED if nsig else "256 unrelated CQ messages"),
                       planted=sum(p["planted"] for p in per), bp_planted=sum(p["bp_hit"] for p in per),
                       failing_candidates=sum(p["failing"] for p in per),
                       smallest_wrong_nhard=wrong[0] if wrong else None, wrong_best_entries_nhard_smallest_20=wrong[:20],
                       gates={str(g): dict(new_planted=sum(p["gates"][g][0] for p in per), wrong_messages=sum(p["gates"][g][1] for p in per),
                                           wrong_candidates=sum(p["gates"][g][2] for p in per)) for g in GATES},
                       seconds=round(time.time() - t0, 1))
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "gates"}), flush=True)
            print({g: (row["gates"][str(g)]["new_planted"], row["gates"][str(g)]["wrong_candidates"]) for g in GATES[::5]}, flush=True)
        for derive in (0, 1):
            for drop in STREAM_DROPS:
                t0 = time.time()
                per = pool.map(stream_sequence, [(s, drop, derive) for s in range(a.sequences)])
                row = dict(name="stream_drop%d_derive%d" % (drop, derive), derive=derive, weaker_by_db=drop, sequences=a.sequences,
                           signals_per_slot=20, repeated_stations=sum(p["repeated"] for p in per), bp_planted_slot2=sum(p["bp_slot2"] for p in per),
                           gates={str(g): dict(gained=sum(p["gates"][g][0] for p in per), not_on_air=sum(p["gates"][g][1] for p in per))
                                  for g in GATES}, seconds=round(time.time() - t0, 1))
                rows.append(row)
                print(row["name"], {g: (row["gates"][str(g)]["gained"], row["gates"][str(g)]["not_on_air"]) for g in GATES[::5] + [49]}, flush=True)
    doc = dict(what="matching undecoded candidates against expected messages, one pass (CPU: the oracle's stages and "
                    "tests/ft8_spec_match.py); per row and gate (max hard errors): planted messages gained over BP, accepted "
                    "messages / candidates whose entry was not on the air; stream rows run the real update rule over three slots",
               command="python tools/match_gain.py --frames %d --sequences %d" % (a.frames, a.sequences), max_candidates=120, min_score=10,
               ldpc_iters=20, gates=GATES, rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
