"""What the demodulation from the I/Q samples gains and what it risks, on the CPU with the oracle's stages and the numpy
restatement of the rule (tests/ft8_spec_demod.py).  Per row, per gate (the largest number of hard errors accepted) and per mask
of soft-bit sets (bit n - 1 = blocks of n symbols): planted messages gained over belief propagation and decodes outside the
planted set.
  cq20       the 96 crowded CQ frames of 20 signals at -22 .. 0 dB of the OSD, AP and match figures (tests/synth_util.make_frame,
             seeds 1000 ...)
  snr-24 .. snr-16   one signal per frame at that SNR, 64 frames each, start and frequency drawn uniformly (off the grid), seeds
             3000 + 100 * step ...; the decoded fraction for BP alone, for each set alone and for their union
  noise      96 frames of noise (make_frame(seed, 0), seeds 5000 ...): wrong acceptances per frame
Cap 120, min_score 10, 20 iterations, one pass, max_per_frame = the cap.  The constants are chosen here: the gate is the largest
swept one at which no row accepts a message outside its planted set under any mask; the mask is the one with the fewest sets
(then the smallest value) whose gain on cq20 at that gate is within 2 % of the largest.

  python tools/demod_gain.py [--procs 8] [--out profiles/demod_gain.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GATES = [20, 25, 30, 36, 40, 45, 50, 60, 174]
MASKS = [1, 2, 3, 4, 5, 6, 7]
SNRS = list(range(-24, -15))
ROWS = [("cq20", 20, (-22.0, 0.0), 1000, 96)] + [("snr%d" % s, 1, (float(s), float(s)), 3000 + 100 * k, 64) for k, s in enumerate(SNRS)] + \
       [("noise", 0, (-22.0, 0.0), 5000, 96)]


def one_frame(job):
    import numpy as np
    import oracle_lib
    import ft8_spec_demod as sdm
    import ft8_spec_messages as sm
    import synth_util as S
    import rtlsdr_ft8d_amd as ft8
    seed, nsig, snr = job
    iq, planted = S.make_frame(seed, nsig, S.oracle_encode_fn(oracle_lib), snr_range=snr)
    iq = np.ascontiguousarray(iq, np.float32)
    want = set(t for t in planted if t is not None)
    mag, cands, counts, status = sm.oracle_stages(oracle_lib, iq[None], 120, 10, 1)
    st = status.view(ft8.STATUS_DTYPE).reshape(1, -1)[0]
    n = int(counts[0])
    seen, bp_hit, bp_miss = [], 0, 0
    for i in range(n):
        if st[i]["ok"]:
            key = (int(st[i]["crc_extracted"]), bytes(st[i]["text"]))
            if key not in seen and len(seen) < 50:
                seen.append(key)
                if st[i]["text"].decode(errors="replace") in want:
                    bp_hit += 1
                else:
                    bp_miss += 1
    failing = [i for i in range(n) if st[i]["ok"] == 0 and st[i]["ldpc_errors"] != 0]
    w4 = sdm.twiddles()
    found = {}                                           # (candidate, set) -> (nhard, crc, text) of a word that passes every check but the gate
    for i in failing:
        _e, _d, _p, per_set = sdm.analyse(iq[0], iq[1], cands[0, i], w4, 20, oracle_lib.bp_decode)
        for s in (1, 2, 3):
            _llr, x, plain, errors = per_set[s]
            if x is None:
                continue
            code, nhard, ext, _calc, _rc, text = sdm.judge(oracle_lib, plain, errors, x, 174)
            if code == 1:
                found[(i, s)] = (nhard, ext, text)
    res = {g: {m: [0, 0] for m in MASKS} for g in GATES}
    for g in GATES:
        for m in MASKS:
            seen_g = list(seen)
            for i in failing:
                for s in (1, 2, 3):                      # the first accepted set ends the candidate
                    if not (m >> (s - 1)) & 1 or (i, s) not in found or found[(i, s)][0] > g:
                        continue
                    _nhard, ext, text = found[(i, s)]
                    if (ext, text) not in seen_g and len(seen_g) < 50:
                        seen_g.append((ext, text))
                        res[g][m][0 if text.decode(errors="replace") in want else 1] += 1
                    break
    return dict(bp_hit=bp_hit, bp_miss=bp_miss, failing=len(failing), planted=len(want), res=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--rows", default=",".join(r[0] for r in ROWS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demod_gain.json"))
    a = ap.parse_args()
    import multiprocessing as mp
    import oracle_lib
    oracle_lib.build()
    rows = []
    with mp.Pool(a.procs) as pool:
        for name, nsig, snr, seed0, frames in ROWS:
            if name not in a.rows.split(","):
                continue
            t0 = time.time()
            per = pool.map(one_frame, [(s, nsig, snr) for s in range(seed0, seed0 + frames)], chunksize=1)
            row = dict(name=name, signals_per_frame=nsig, snr_db=list(snr), seeds=[seed0, seed0 + frames - 1], frames=frames,
                       planted=sum(p["planted"] for p in per), bp_planted=sum(p["bp_hit"] for p in per),
                       bp_outside=sum(p["bp_miss"] for p in per), failing_candidates=sum(p["failing"] for p in per), gates={})
            for g in GATES:
                row["gates"][str(g)] = {str(m): dict(new_planted=sum(p["res"][g][m][0] for p in per),
                                                     outside=sum(p["res"][g][m][1] for p in per)) for m in MASKS}
            row["seconds"] = round(time.time() - t0, 1)
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "gates"}), json.dumps(row["gates"]["174"]), flush=True)
    clean = [g for g in GATES if all(r["gates"][str(g)][str(m)]["outside"] == 0 for r in rows for m in MASKS)]
    gate = max(clean) if clean else None
    choice = dict(max_hard_errors=gate, sets=None)
    cq = next((r for r in rows if r["name"] == "cq20"), None)
    if gate is not None and cq is not None:
        gains = {m: cq["gates"][str(gate)][str(m)]["new_planted"] for m in MASKS}
        best = max(gains.values())
        ok = [m for m in MASKS if gains[m] >= 0.98 * best]
        choice["sets"] = min(ok, key=lambda m: (bin(m).count("1"), m))
        choice["cq20_gain_by_mask"] = gains
        for r in rows:
            if r["name"].startswith("snr"):
                at = r["gates"][str(gate)]
                r["decoded_fraction"] = dict(bp=r["bp_planted"] / r["planted"],
                                             **{"mask%d" % m: (r["bp_planted"] + at[str(m)]["new_planted"]) / r["planted"] for m in (1, 2, 4, 7)})
    doc = dict(what="demodulation from the I/Q samples after belief propagation, one pass (CPU: the oracle's stages and "
                    "tests/ft8_spec_demod.py); per gate (max hard errors) and mask of soft-bit sets: planted messages gained, decodes "
                    "outside the planted set; decoded_fraction of the single-signal rows at the chosen gate",
               command="python tools/demod_gain.py", max_candidates=120, min_score=10, ldpc_iters=20, gates=GATES, masks=MASKS,
               chosen=choice, rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(choice))


if __name__ == "__main__":
    main()
