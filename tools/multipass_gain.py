"""What multi-pass decoding gains, on the CPU with the oracle's stages (tests/ft8_spec_multipass.py): planted messages
decoded after 1, 2 and 3 passes, and decodes outside the planted set, over signals per frame x traffic.  CQ frames are
tests/synth_util.make_frame (CQ messages at 100..1500 Hz, dt 0..1.8 s); mixed frames are make_mixed_frame over
rtlsdr_ft8d_amd.workload.mixed_message_pool.  Cap 120, min_score 10, 20 iterations.  Writes one JSON document.

  python tools/multipass_gain.py [--frames 96] [--seed 1000] [--out profiles/multipass_gain.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (traffic, signals per frame, SNR range in dB)
ROWS = [("cq", 20, (-22.0, 0.0)), ("cq", 30, (-22.0, 0.0)), ("cq", 45, (-22.0, 0.0)), ("cq", 1, (-24.0, -14.0)),
        ("mixed", 20, (-22.0, 0.0)), ("mixed", 30, (-22.0, 0.0)), ("mixed", 45, (-22.0, 0.0))]
PASSES = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multipass_gain.json"))
    a = ap.parse_args()
    import numpy as np
    import oracle_lib
    import synth_util as S
    import ft8_spec_multipass as spec
    from rtlsdr_ft8d_amd import workload
    oracle_lib.build()
    enc = S.oracle_encode_fn(oracle_lib)
    texts, tones = workload.mixed_message_pool(1024, seed=7)
    seeds = range(a.seed, a.seed + a.frames)
    rows = []
    for traffic, nsig, snr in ROWS:
        t0 = time.time()
        if traffic == "cq":
            fr = [S.make_frame(s, nsig, enc, snr_range=snr) for s in seeds]
        else:
            fr = [S.make_mixed_frame(s, nsig, snr, texts, tones) for s in seeds]
        iq = np.stack([f[0] for f in fr])
        planted = [f[1] for f in fr]
        msgs, n, nbp = spec.decode_passes(oracle_lib, iq, PASSES, nthreads=a.threads)
        correct, outside = [], []
        for p in range(PASSES):
            hit = miss = 0
            for f in range(len(n)):
                want = set(t for t in planted[f] if t is not None)
                for r in msgs[f, :int(nbp[f, p])]:
                    if r["text"].decode(errors="replace") in want:
                        hit += 1
                    else:
                        miss += 1
            correct.append(hit)
            outside.append(miss)
        row = dict(traffic=traffic, signals_per_frame=nsig, snr_db=list(snr), frames=a.frames,
                   planted=int(sum(len(set(t for t in p if t is not None)) for p in planted)),
                   correct_by_pass=correct, outside_planted_by_pass=outside,
                   decodes_by_pass=[int(nbp[:, p].sum()) for p in range(PASSES)],
                   gain_pct_by_pass=[round(100.0 * (c / correct[0] - 1.0), 2) if correct[0] else None for c in correct],
                   frames_gaining_in_pass=[int((nbp[:, p] > nbp[:, p - 1]).sum()) for p in range(1, PASSES)],
                   seconds=round(time.time() - t0, 1))
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc = dict(what="planted messages decoded after each pass (CPU: the oracle's stages through tests/ft8_spec_multipass.py)",
               command="python tools/multipass_gain.py --frames %d --seed %d" % (a.frames, a.seed),
               seeds=[a.seed, a.seed + a.frames - 1], max_candidates=120, min_score=10, ldpc_iters=20,
               mixed_pool="workload.mixed_message_pool(1024, seed=7); a mixed frame carries nsig + 1 signals (one message twice)",
               rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
