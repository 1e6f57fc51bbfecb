"""What a-priori decoding on the demodulated soft bits gains and what it risks, on the CPU with the oracle's stages and the
restatements (tests/ft8_spec_demod.py, tests/ft8_spec_apsoft.py).  The rows and seeds are those of tools/demod_gain.py (cq20,
snr-24 .. snr-16, noise); the demodulation runs at its recommended values (all three sets, no gate); AP then runs on the rows of
what is still undecoded, sets 7, under two hypothesis tables:
  cq       "CQ ? ?" alone
  cq+3     "CQ ? ?" and three call hypotheses that no planted message carries (the false-decode side: 29 more forced bits each)
Per row, table and AP gate (the largest number of hard errors accepted): planted messages gained over the demodulation (through
the append step: unique, up to 50 per frame) and decodes outside the planted set.  The recommended gate is chosen here by
tools/demod_gain.py's rule: the largest swept gate at which no row accepts anything outside its planted set, under either table.

  python tools/demod_ap_gain.py [--procs 8] [--out profiles/demod_ap_gain.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import demod_gain as dg                      # the rows and gates (tools/ is on the path of a script started from it)

GATES = dg.GATES
ROWS = dg.ROWS
TABLES = {"cq": ["CQ ? ?"], "cq+3": ["CQ ? ?", "VK9XQX ? ?", "ZS6ZZQ ? ?", "JA1QQY ? ?"]}


def one_frame(job):
    import numpy as np
    import oracle_lib
    import ft8_spec_ap as sa
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
    seen = []                                            # the frame's records so far: (crc, text)
    hits = [0, 0]                                        # [planted, outside] after BP, then after the demodulation

    def add(key, tally):
        if key not in seen and len(seen) < 50:
            seen.append(key)
            tally[0 if key[1].decode(errors="replace") in want else 1] += 1

    for i in range(n):
        if st[i]["ok"]:
            add((int(st[i]["crc_extracted"]), bytes(st[i]["text"])), hits)
    bp_hit, bp_miss = hits
    failing = [i for i in range(n) if st[i]["ok"] == 0 and st[i]["ldpc_errors"] != 0]
    w4 = sdm.twiddles()
    demod = [0, 0]
    left = []                                            # still undecoded: (candidate, its usable rows {set: x})
    for i in failing:
        _e, _d, _p, per_set = sdm.analyse(iq[0], iq[1], cands[0, i], w4, 20, oracle_lib.bp_decode)
        rows, won = {}, False
        for s in (1, 2, 3):
            _llr, x, plain, errors = per_set[s]
            if x is None:
                continue
            rows[s] = x
            code, _nhard, ext, _calc, _rc, text = sdm.judge(oracle_lib, plain, errors, x, sdm.MAX_HARD_ERRORS)
            if code == 1:
                add((ext, text), demod)
                won = True
                break
        if not won:
            left.append((i, rows))
    res = {}
    for name, patterns in TABLES.items():
        hyps = [sa.from_text(p) for p in patterns]
        words = []                                       # per candidate: (nhard, crc, text) of every word that passes all checks but the gate
        for i, rows in left:
            w = []
            for s in (1, 2, 3):
                if s not in rows:
                    continue
                tried = sa.attempts(oracle_lib, rows[s], hyps, 20)
                if tried is None:
                    continue
                h = (rows[s] > 0).astype(np.uint8)
                for plain, errors, _it, m, b in tried:
                    code, nhard, ext, _calc, _rc, text = sa.judge(oracle_lib, plain, errors, m, b, h, 174)
                    if code == 1:
                        w.append((nhard, ext, text))
            words.append(w)
        res[name] = {}
        for g in GATES:
            tally, mark = [0, 0], len(seen)
            for w in words:
                first = next((x for x in w if x[0] <= g), None)          # the first accepted (set, hypothesis) ends the candidate
                if first is not None:
                    add((first[1], first[2]), tally)
            del seen[mark:]
            res[name][g] = tally
    return dict(bp_hit=bp_hit, bp_miss=bp_miss, failing=len(failing), planted=len(want), demod_hit=demod[0], demod_miss=demod[1],
                left=len(left), res=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--rows", default=",".join(r[0] for r in ROWS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demod_ap_gain.json"))
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
                       bp_outside=sum(p["bp_miss"] for p in per), failing_candidates=sum(p["failing"] for p in per),
                       demod_new_planted=sum(p["demod_hit"] for p in per), demod_outside=sum(p["demod_miss"] for p in per),
                       failing_after_demod=sum(p["left"] for p in per), tables={})
            for t in TABLES:
                row["tables"][t] = {str(g): dict(new_planted=sum(p["res"][t][g][0] for p in per), outside=sum(p["res"][t][g][1] for p in per))
                                    for g in GATES}
            row["seconds"] = round(time.time() - t0, 1)
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "tables"}), json.dumps(row["tables"]), flush=True)
    clean = [g for g in GATES if all(r["tables"][t][str(g)]["outside"] == 0 for r in rows for t in TABLES)]
    gate = max(clean) if clean else None
    choice = dict(ap_max_hard_errors=gate)
    if gate is not None:
        for r in rows:
            if r["name"].startswith("snr"):
                r["decoded_fraction"] = dict(bp=r["bp_planted"] / r["planted"], demod=(r["bp_planted"] + r["demod_new_planted"]) / r["planted"],
                                             demod_ap=(r["bp_planted"] + r["demod_new_planted"] + r["tables"]["cq"][str(gate)]["new_planted"]) / r["planted"])
    doc = dict(what="a-priori decoding on the soft bits of the demodulation from the I/Q samples, behind belief propagation and the "
                    "demodulation (all sets, no gate), one pass (CPU: the oracle's stages, tests/ft8_spec_demod.py and "
                    "tests/ft8_spec_apsoft.py's rule); per hypothesis table and AP gate: planted messages gained over the demodulation, "
                    "decodes outside the planted set; decoded_fraction of the single-signal rows at the chosen gate under \"CQ ? ?\"",
               command="python tools/demod_ap_gain.py --procs %d" % a.procs, max_candidates=120, min_score=10, ldpc_iters=20, gates=GATES, tables=TABLES,
               chosen=choice, rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(choice))


if __name__ == "__main__":
    main()
