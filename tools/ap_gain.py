"""What a-priori decoding gains and what it risks, on the CPU with the oracle's stages and the restatement of the rule
(tests/ft8_spec_ap.py).  Per workload (the rows of tools/osd_gain.py), per hypothesis set ("CQ ? ?" alone; with "CQ DX ? ?")
and per gate (the largest number of hard errors accepted on the unmasked positions): planted messages gained over belief
propagation, decodes outside the planted set, and the failing candidates for which BP converges under a hypothesis, agrees
with it, lies within the gate and is NOT a planted codeword -- each of those still has to pass the CRC (2^-14) to become a
false decode.  The hard errors of the right and of the wrong words are listed, so that the gate can be read off.
The same pass measures the combination: OSD orders 1 and 2 at their recommended gate behind AP (on what AP left undecoded),
beside OSD alone.  Cap 120, min_score 10, 20 iterations, one pass.

  python tools/ap_gain.py [--frames 96] [--procs 8] [--out profiles/ap_gain.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from osd_gain import ROWS, frame_of  # noqa: E402

SETS = {"cq": ("CQ ? ?",), "cq+cqdx": ("CQ ? ?", "CQ DX ? ?")}
GATES = [15, 20, 25, 30, 35, 40, 45, 50, 60, 174]
ORDERS = [1, 2]
OSD_GATE = 27                                            # FT8GPU_OSD_MAX_HARD_ERRORS


def one_frame(job):
    import numpy as np
    import oracle_lib
    import ft8_spec_ap as sa
    import ft8_spec_messages as sm
    import ft8_spec_osd as so
    import rtlsdr_ft8d_amd as ft8
    traffic, seed, nsig, snr = job
    iq, planted, codewords = frame_of(traffic, seed, nsig, snr)
    want = set(t for t in planted if t is not None)
    cws = set(codewords)
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
    llrs = {i: oracle_lib.llr(mag[0], cands[0, i]) for i in failing}
    hyp_sets = {name: [sa.from_text(t) for t in texts] for name, texts in SETS.items()}
    # OSD's best patterns, once per candidate: (nhard, result code tuple)
    osd = {}
    for i in failing:
        if np.isfinite(llrs[i]).all():
            s = so.search(llrs[i])
            for o in ORDERS:
                metric, pat, nhard, cw = s[o]
                osd[(i, o)] = so.judge(oracle_lib, cw, nhard, OSD_GATE)

    def osd_gain(order, seen_now, skip):
        got = [0, 0]
        seen_o = list(seen_now)
        for i in failing:
            if i in skip or (i, order) not in osd or osd[(i, order)][0] != 1:
                continue
            code = osd[(i, order)]
            key = (code[1], code[4])
            if key in seen_o or len(seen_o) >= 50:
                continue
            seen_o.append(key)
            got[0 if code[4].decode(errors="replace") in want else 1] += 1
        return got

    res = {}
    hard = {name: dict(right=[], wrong=[]) for name in SETS}
    converged = {name: 0 for name in SETS}
    for name, hyps in hyp_sets.items():
        tried = {i: sa.attempts(oracle_lib, llrs[i], hyps) for i in failing}
        # every converged word that agrees with its hypothesis, with its hard errors: right (planted) or wrong
        for i in failing:
            if tried[i] is None:
                continue
            h = (llrs[i] > 0).astype(np.uint8)
            for plain, errors, it, m, b in tried[i]:
                if errors == 0:
                    converged[name] += 1
                    if (plain[m] == b[m]).all():
                        nh = int(((plain != h) & ~m).sum())
                        hard[name]["right" if bytes(plain) in cws else "wrong"].append(nh)
        res[name] = {}
        for g in GATES:
            new, outside, wrong = 0, 0, 0
            seen_g = list(seen)
            accepted = set()
            for i in failing:
                if tried[i] is None:
                    continue
                h = (llrs[i] > 0).astype(np.uint8)
                for plain, errors, it, m, b in tried[i]:
                    if errors == 0 and (plain[m] == b[m]).all() and int(((plain != h) & ~m).sum()) <= g and bytes(plain) not in cws:
                        wrong += 1
                info, win = sa.resolve(oracle_lib, llrs[i], tried[i], g)
                if win is None:
                    continue
                accepted.add(i)
                plain, ext, calc, rc, text = win
                key = (ext, text)
                if key in seen_g or len(seen_g) >= 50:
                    continue
                seen_g.append(key)
                if text.decode(errors="replace") in want:
                    new += 1
                else:
                    outside += 1
            res[name][g] = dict(new=new, outside=outside, wrong=wrong,
                                osd_after={o: osd_gain(o, seen_g, accepted) for o in ORDERS})
    return dict(bp_hit=bp_hit, bp_miss=bp_miss, failing=len(failing), planted=len(want), res=res, hard=hard, converged=converged,
                osd_alone={o: osd_gain(o, seen, set()) for o in ORDERS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--rows", default=",".join(r[0] for r in ROWS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ap_gain.json"))
    a = ap.parse_args()
    import multiprocessing as mp
    import oracle_lib
    oracle_lib.build()
    rows = []
    with mp.Pool(a.procs) as pool:
        for name, traffic, nsig, snr, seed0 in ROWS:
            if name not in a.rows.split(","):
                continue
            t0 = time.time()
            per = pool.map(one_frame, [(traffic, s, nsig, snr) for s in range(seed0, seed0 + a.frames)])
            row = dict(name=name, traffic=traffic, signals_per_frame=nsig, snr_db=list(snr), seeds=[seed0, seed0 + a.frames - 1],
                       frames=a.frames, planted=sum(p["planted"] for p in per), bp_planted=sum(p["bp_hit"] for p in per),
                       bp_outside=sum(p["bp_miss"] for p in per), failing_candidates=sum(p["failing"] for p in per),
                       osd_alone={str(o): dict(new_planted=sum(p["osd_alone"][o][0] for p in per),
                                               outside=sum(p["osd_alone"][o][1] for p in per)) for o in ORDERS},
                       sets={})
            for s in SETS:
                d = dict(hypotheses=list(SETS[s]), bp_converged=sum(p["converged"][s] for p in per),
                         hard_errors_of_planted_words=sorted(x for p in per for x in p["hard"][s]["right"]),
                         hard_errors_of_wrong_words=sorted(x for p in per for x in p["hard"][s]["wrong"]), gates={})
                for g in GATES:
                    wrong = sum(p["res"][s][g]["wrong"] for p in per)
                    d["gates"][str(g)] = dict(
                        new_planted=sum(p["res"][s][g]["new"] for p in per), outside=sum(p["res"][s][g]["outside"] for p in per),
                        wrong_within_gate=wrong, expected_false_per_frame=wrong / 16384.0 / a.frames,
                        osd_behind_ap={str(o): dict(new_planted=sum(p["res"][s][g]["osd_after"][o][0] for p in per),
                                                    outside=sum(p["res"][s][g]["osd_after"][o][1] for p in per)) for o in ORDERS})
                row["sets"][s] = d
            row["seconds"] = round(time.time() - t0, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    doc = dict(what="a-priori decoding after belief propagation, one pass (CPU: the oracle's stages and tests/ft8_spec_ap.py); per "
                    "hypothesis set and gate (max hard errors on the unmasked positions): planted messages gained, decodes outside "
                    "the planted set, converged words that agree with their hypothesis within the gate and are not planted "
                    "codewords; osd_behind_ap: what OSD (gate %d) then adds on the candidates AP left, osd_alone: OSD without AP" % OSD_GATE,
               command="python tools/ap_gain.py --frames %d" % a.frames, max_candidates=120, min_score=10, ldpc_iters=20,
               gates=GATES, osd_gate=OSD_GATE, rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
