"""What combining soft bits across slots gains and what it risks, with the numpy restatement of the rule
(tests/ft8_spec_combine.py; the oracle's stages and its C bp_decode) and, with --gpu, on the device with equal results.
Streams of 4 slots per receiver (the recipe of tests/synth_util.py: CPFSK in complex AWGN, peak-normalised):
  cq20, cq30  96 receivers, 20 / 30 CQ stations per slot at U[-24, 0] dB; one station set in slots 0 and 2, another in slots 1
              and 3, every station at its own frequency (100 .. 1500 Hz) and clock offset (0 .. 1.8 s) in both of its slots,
              fresh noise per slot;
  noise       96 receivers x 4 slots of noise only: everything accepted is wrong.
A sweep over min_agree (88 .. 130) x store_per_slot (16 .. 128), max_age 0.  Per row and point: planted messages gained over
BP alone (unique per frame, as the append step counts them), messages accepted that were not on the air in that slot, BP runs
per frame (candidates whose info.result is 1, 3, 4, 5 or 7).  The recommended FT8GPU_COMBINE_MIN_AGREE is the smallest swept
gate that accepts nothing wrong on any row at any swept store_per_slot.  For FT8GPU_COMBINE_STORE_PER_SLOT the file carries two
readings at that gate, gains summed over the CQ rows: the smallest swept value within 2 % of the gain at 128, and the smallest
within 2 % of the largest gain of the sweep.  They differ because the gain is not monotone in store_per_slot: a station's
partner lies two slots back, and a ring of 128 entries that takes 96 or 128 candidates per slot has overwritten it by then.
The constant is the second reading.  --compare N adds, on the first N receivers
of cq20, what AP ("CQ ? ?", gate 35), OSD (order 2, gate 27) and matching (gate 49, derive 0, its own table filled by its own
update rule) gain on the same frames.  Cap 120, min_score 10, 20 iterations.

  python tools/combine_gain.py [--receivers 96] [--procs 8] [--compare 24] [--gpu] [--out profiles/combine_gain.json]"""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GATES = [88, 94, 100, 106, 112, 118, 124, 130]
STORES = [16, 24, 32, 48, 64, 96, 128]
SLOTS = 4
SNR = (-24.0, 0.0)
ROWS = (("cq20", 20, 7000), ("cq30", 30, 8000), ("noise", 0, 9000))


class CachedOracle:
    """oracle_lib with the normalised soft bits of a candidate remembered across the points of the sweep"""

    def __init__(self, oracle):
        self._o, self._llr = oracle, {}

    def __getattr__(self, name):
        return getattr(self._o, name)

    def llr(self, mag, cand):
        key = (zlib.crc32(mag), cand.tobytes())                  # by content: the slices of a sweep come and go at the same addresses
        v = self._llr.get(key)
        if v is None:
            v = self._llr[key] = self._o.llr(mag, cand)
        return v


def stream(seed, nsig):
    """(iq [1][4][2][48000], texts per slot) of one receiver"""
    import numpy as np
    import rtlsdr_ft8d_amd as ft8
    import synth_util as S
    rng = np.random.default_rng(seed)
    sets = []
    for _ in range(2):
        tx = [S.random_message(rng, cq=True) for _ in range(nsig)]
        sets.append((tx, rng.uniform(100.0, 1500.0, nsig), rng.uniform(0.0, 1.8, nsig), rng.uniform(SNR[0], SNR[1], nsig)))
    iq = np.zeros((1, SLOTS, 2, S.NSAMPLES), np.float32)
    for s in range(SLOTS):
        tx, f0, t0, db = sets[s & 1]
        noise = np.random.default_rng(100000 + 10 * seed + s)
        fi, fq = noise.normal(0.0, 1.0, S.NSAMPLES), noise.normal(0.0, 1.0, S.NSAMPLES)
        for k, t in enumerate(tx):
            si, sq = S.cpfsk(ft8.encode(ft8.pack77(t)), float(f0[k]), int(round(t0[k] * 3200)), S.amplitude_for_snr(float(db[k]), 1.0))
            fi += si
            fq += sq
        i32, q32 = fi.astype(np.float32), fq.astype(np.float32)
        scale = np.float32(0.5) / max(np.abs(i32).max(), np.abs(q32).max(), np.float32(1e-24))
        iq[0, s, 0], iq[0, s, 1] = i32 * scale, q32 * scale
    return iq, [sets[s & 1][0] for s in range(SLOTS)]


def tally(msgs, nbs, texts):
    """(BP's planted messages, planted gained, not on the air) over the slots of one receiver"""
    bp = good = bad = 0
    for s in range(SLOTS):
        bp += sum(msgs[0, s, k]["text"].decode(errors="replace") in texts[s] for k in range(int(nbs[0, s, 0])))
        for k in range(int(nbs[0, s, 0]), int(nbs[0, s, 1])):
            ok = msgs[0, s, k]["text"].decode(errors="replace") in texts[s]
            good += ok
            bad += not ok
    return bp, good, bad


def receiver(job):
    import numpy as np
    import oracle_lib
    import ft8_spec_combine as sc
    import ft8_spec_messages as sm
    seed, nsig, compare = job
    iq, texts = stream(seed, nsig)
    stages = sm.oracle_stages(oracle_lib, iq.reshape(SLOTS, 2, -1), 120, 10, 1)
    o = CachedOracle(oracle_lib)
    out = dict(planted=sum(len(set(t)) for t in texts), points={})
    for g in GATES:
        for store in STORES:
            trace = []
            msgs, n, nbs, _st = sc.decode_combined(o, iq, min_agree=g, store_per_slot=store, stages=stages, nthreads=1, bp=oracle_lib.bp_decode,
                                                   trace=trace)
            bp, good, bad = tally(msgs, nbs, texts)
            runs = sum(int(np.isin(info["result"], (1, 3, 4, 5, 7)).sum()) for _s, info in trace)
            out["points"][(g, store)] = (good, bad, runs)
            out["bp"] = bp
    if compare:
        import ft8_spec_ap as sap
        import ft8_spec_match as smt
        import ft8_spec_osd as so
        frames = iq.reshape(SLOTS, 2, -1)
        flat = [t for t in texts]
        m, n, nbs = sap.decode_ap(oracle_lib, frames, 1, [sap.cq_hypothesis()], 35, -1, 27, nthreads=1)
        out["ap"] = sum(m[s, k]["text"].decode(errors="replace") in flat[s] for s in range(SLOTS) for k in range(int(nbs[s, 0, 0]), int(nbs[s, 0, 1])))
        m, n, nbs = sap.decode_ap(oracle_lib, frames, 1, [], 35, 2, 27, nthreads=1)
        out["osd"] = sum(m[s, k]["text"].decode(errors="replace") in flat[s] for s in range(SLOTS) for k in range(int(nbs[s, 0, 1]), int(nbs[s, 0, 2])))
        m, n, nbs, _st = smt.decode_expected(oracle_lib, iq, max_hard_errors=49, derive=False, stages=stages, nthreads=1)
        out["match"] = tally(m, nbs, texts)[1]
    return out


def gpu_points(a, rows, recommended):
    """the device on the same streams at a few points of the sweep: (good, bad) per row must equal the restatement's"""
    import numpy as np
    import rtlsdr_ft8d_amd as ft8
    pts = sorted({(GATES[0], 128), (recommended[0], recommended[1]), (GATES[-1], STORES[0])})
    out = []
    with ft8.Decoder(device=0, max_frames=a.receivers * SLOTS) as dec:
        for (name, nsig, seed0), row in zip(ROWS, rows):
            made = [stream(s, nsig) for s in range(seed0, seed0 + a.receivers)]
            iq = np.concatenate([m[0] for m in made])
            for g, store in pts:
                msgs, n, nbs, _st = dec.decode_messages_combined(iq, None, g, 0, store)
                good = bad = 0
                for r in range(a.receivers):
                    _bp, gd, bd = tally(msgs[r:r + 1], nbs[r:r + 1], made[r][1])
                    good, bad = good + gd, bad + bd
                want = row["points"]["%d,%d" % (g, store)]
                out.append(dict(row=name, min_agree=g, store_per_slot=store, gained=good, wrong=bad,
                                equals_restatement=(good, bad) == (want["gained"], want["wrong"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--receivers", type=int, default=96)
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--compare", type=int, default=24)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--device-only", action="store_true", help="read --out, run the device on its streams, write the 'device' key back")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine_gain.json"))
    a = ap.parse_args()
    if a.device_only:
        with open(a.out) as f:
            doc = json.load(f)
        rec = doc["recommended"]
        doc["device"] = gpu_points(a, doc["rows"], (rec["min_agree"], rec["store_per_slot"]))
        print(doc["device"], flush=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return 0 if all(d["equals_restatement"] for d in doc["device"]) else 1
    import multiprocessing as mp
    import oracle_lib
    oracle_lib.build()
    rows = []
    with mp.Pool(a.procs) as pool:
        for name, nsig, seed0 in ROWS:
            t0 = time.time()
            per = pool.map(receiver, [(s, nsig, name == "cq20" and k < a.compare) for k, s in enumerate(range(seed0, seed0 + a.receivers))], chunksize=1)
            frames = a.receivers * SLOTS
            row = dict(name=name, signals_per_slot=nsig, snr_db=list(SNR), seeds=[seed0, seed0 + a.receivers - 1], receivers=a.receivers,
                       slots=SLOTS, planted=sum(p["planted"] for p in per), bp_planted=sum(p["bp"] for p in per),
                       points={"%d,%d" % k: dict(gained=sum(p["points"][k][0] for p in per), wrong=sum(p["points"][k][1] for p in per),
                                                  bp_runs_per_frame=round(sum(p["points"][k][2] for p in per) / frames, 2))
                               for k in per[0]["points"]}, seconds=round(time.time() - t0, 1))
            cmp_ = [p for p in per if "ap" in p]
            if cmp_:
                row["comparison"] = dict(receivers=len(cmp_), bp_planted=sum(p["bp"] for p in cmp_), ap_cq_gate35=sum(p["ap"] for p in cmp_),
                                         osd_order2_gate27=sum(p["osd"] for p in cmp_), match_gate49_own_table=sum(p["match"] for p in cmp_),
                                         combine_by_point={"%d,%d" % (g, st): sum(p["points"][(g, st)][0] for p in cmp_)
                                                           for g in GATES for st in STORES})
            rows.append(row)
            print(name, "planted", row["planted"], "bp", row["bp_planted"], row.get("comparison"), row["seconds"], "s", flush=True)
            for g in GATES:
                print("  gate", g, [(s, row["points"]["%d,%d" % (g, s)]["gained"], row["points"]["%d,%d" % (g, s)]["wrong"],
                                     row["points"]["%d,%d" % (g, s)]["bp_runs_per_frame"]) for s in STORES], flush=True)
    clean = [g for g in GATES if all(r["points"]["%d,%d" % (g, s)]["wrong"] == 0 for r in rows for s in STORES)]
    gate = clean[0] if clean else None
    rec = None
    if gate is not None:
        gain = {s: sum(r["points"]["%d,%d" % (gate, s)]["gained"] for r in rows[:2]) for s in STORES}
        store = min(s for s in STORES if gain[s] >= 0.98 * max(gain.values()))
        rec = dict(min_agree=gate, store_per_slot=store, gain_by_store_at_that_gate=gain,
                   smallest_store_within_2_percent_of_gain_at_128=min(s for s in STORES if gain[s] >= 0.98 * gain[128]),
                   smallest_store_within_2_percent_of_largest_gain=store)
    doc = dict(what="soft bits of undecoded candidates combined across a receiver's slots (CPU: the oracle's stages and "
                    "tests/ft8_spec_combine.py); per row and point 'min_agree,store_per_slot': planted messages gained over BP, "
                    "messages accepted that were not on the air, BP runs per frame",
               command="python tools/combine_gain.py --receivers %d --compare %d" % (a.receivers, a.compare), max_candidates=120, min_score=10,
               ldpc_iters=20, max_age=0, gates=GATES, stores=STORES, recommended=rec, rows=rows)
    if a.gpu and rec:
        doc["device"] = gpu_points(a, rows, (rec["min_agree"], rec["store_per_slot"]))
        print(doc["device"], flush=True)
    print("recommended", rec, flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
