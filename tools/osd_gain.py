"""What ordered-statistics decoding gains and what it risks, on the CPU with the oracle's stages and the numpy restatement
of the rule (tests/ft8_spec_osd.py).  Per workload, per order (1, 2) and per gate (the largest number of hard errors
accepted): planted messages gained over belief propagation, decodes outside the planted set, and the number of failing
candidates whose best pattern is within the gate and is not a planted codeword -- each of those passes the CRC with
probability 2^-14, so that number x 2^-14 / frames is the expected false-decode rate per frame.
CQ frames are tests/synth_util.make_frame, mixed frames make_mixed_frame over workload.mixed_message_pool(1024, seed=7),
noise frames make_frame(seed, 0, ...) at seeds 5000...  Cap 120, min_score 10, 20 iterations, one pass.

  python tools/osd_gain.py [--frames 96] [--procs 8] [--out profiles/osd_gain.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, traffic, signals per frame, SNR range in dB, first seed)
ROWS = [("cq20", "cq", 20, (-22.0, 0.0), 1000), ("cq1", "cq", 1, (-24.0, -14.0), 1000), ("noise", "cq", 0, (-22.0, 0.0), 5000),
        ("mixed20", "mixed", 20, (-22.0, 0.0), 1000), ("mixed30", "mixed", 30, (-22.0, 0.0), 1000),
        ("mixed45", "mixed", 45, (-22.0, 0.0), 1000)]
GATES = [20, 23, 25, 27, 29, 31, 33, 35, 40, 83]
ORDERS = [1, 2]
_pool = None


def codeword_of_tones(tones):
    """the 174 codeword bits behind 79 tones (data symbols 7..35 and 43..71, Gray map 0 1 3 2 5 6 4 7)"""
    inv = {g: b for b, g in enumerate([0, 1, 3, 2, 5, 6, 4, 7])}
    bits = []
    for k in list(range(7, 36)) + list(range(43, 72)):
        v = inv[int(tones[k])]
        bits += [(v >> 2) & 1, (v >> 1) & 1, v & 1]
    return bytes(bits)


def frame_of(traffic, seed, nsig, snr):
    """(iq, planted texts, planted codewords)"""
    import numpy as np
    import oracle_lib
    import synth_util as S
    global _pool
    if traffic == "cq":
        enc = S.oracle_encode_fn(oracle_lib)
        iq, msgs = S.make_frame(seed, nsig, enc, snr_range=snr)
        return iq, msgs, [codeword_of_tones(enc(m)) for m in msgs]
    if _pool is None:
        from rtlsdr_ft8d_amd import workload
        _pool = workload.mixed_message_pool(1024, seed=7)
    texts, tones = _pool
    iq, planted = S.make_mixed_frame(seed, nsig, snr, texts, tones)
    rng = np.random.default_rng(seed)                    # make_mixed_frame's own draws, to know WHICH pool entries it took
    rng.normal(0.0, 1.0, S.NSAMPLES), rng.normal(0.0, 1.0, S.NSAMPLES)
    picks = list(rng.integers(0, len(texts), nsig))
    assert [texts[k] for k in picks] == planted[:nsig]
    return iq, planted, [codeword_of_tones(tones[k]) for k in picks]


def one_frame(job):
    import numpy as np
    import oracle_lib
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
    res = {o: {g: [0, 0, 0] for g in GATES} for o in ORDERS}          # new planted, outside, wrong within the gate
    found = {}
    for i in failing:
        llr = oracle_lib.llr(mag[0], cands[0, i])
        if not np.isfinite(llr).all():
            continue
        s = so.search(llr)
        for o in ORDERS:
            metric, pat, nhard, cw = s[o]
            code = so.judge(oracle_lib, cw, nhard, 174)
            found[(i, o)] = (nhard, bytes(cw) in cws, code)
    for o in ORDERS:
        for g in GATES:
            seen_g = list(seen)
            for i in failing:
                if (i, o) not in found:
                    continue
                nhard, right, code = found[(i, o)]
                if nhard > g or code[0] == 5:
                    continue
                if not right:
                    res[o][g][2] += 1
                if code[0] != 1:
                    continue
                key = (code[1], code[4])
                if key in seen_g or len(seen_g) >= 50:
                    continue
                seen_g.append(key)
                res[o][g][0 if code[4].decode(errors="replace") in want else 1] += 1
    return dict(bp_hit=bp_hit, bp_miss=bp_miss, failing=len(failing), planted=len(want), res=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--rows", default=",".join(r[0] for r in ROWS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "osd_gain.json"))
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
                       bp_outside=sum(p["bp_miss"] for p in per), failing_candidates=sum(p["failing"] for p in per), orders={})
            for o in ORDERS:
                row["orders"][str(o)] = {}
                for g in GATES:
                    tot = [sum(p["res"][o][g][k] for p in per) for k in range(3)]
                    row["orders"][str(o)][str(g)] = dict(new_planted=tot[0], outside=tot[1], wrong_within_gate=tot[2],
                                                         expected_false_per_frame=tot[2] / 16384.0 / a.frames)
            row["seconds"] = round(time.time() - t0, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    doc = dict(what="ordered-statistics decoding after belief propagation, one pass (CPU: the oracle's stages and tests/ft8_spec_osd.py); "
                    "per order and gate (max hard errors): planted messages gained, decodes outside the planted set, failing "
                    "candidates whose best pattern is within the gate and not a planted codeword",
               command="python tools/osd_gain.py --frames %d" % a.frames, max_candidates=120, min_score=10, ldpc_iters=20,
               gates=GATES, rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
