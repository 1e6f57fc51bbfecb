"""What multi-pass decoding gains when the decoded signals are subtracted from the I/Q samples, on the CPU with the oracle's
stages (tests/ft8_spec_subtract.py): planted messages decoded after 1, 2 and 3 passes, and decodes outside the planted set, over
the rows, seeds and frame counts of tools/multipass_gain.py, with the masking path's figures from profiles/multipass_gain.json
beside each.  Writes one JSON document.
--waveform gfsk synthesises the same signals pulse-shaped (tools/gfsk_effect.waveform); --shape selects the reference the records
are subtracted with (tests/ft8_spec_subtract_gfsk.py).  Several of either give every row once per waveform and shape.

  python tools/subtract_gain.py [--frames 96] [--seed 1000] [--out profiles/subtract_gain.json]
                                [--smooth 8] [--range 2] [--tstep 8]      (other constants of the rule, for comparison only)
  python tools/subtract_gain.py --rows 0 2 --waveform gfsk cpfsk --shape 0 1 --out profiles/subtract_gfsk_gain.json"""
import argparse
import concurrent.futures as cf
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from multipass_gain import PASSES, ROWS  # noqa: E402  (tools/ is the script's directory)


def set_constants(smooth, rng, tstep):
    import numpy as np
    import ft8_spec_subtract as ss
    ss.SMOOTH, ss.RANGE, ss.TSTEP = smooth, rng, tstep
    ss.INV = np.array([0.0] + [1.0 / (32.0 * n) for n in range(1, 2 * smooth + 2)]).astype(np.float32)


def decode_chunk(job):
    """a few frames of one row through the restated path (a worker process: the numpy restatement is single-threaded)"""
    traffic, nsig, snr, seeds, consts = job[:5]
    name, shape = job[5:] if len(job) > 5 else ("cpfsk", 0)
    import numpy as np
    import oracle_lib
    import synth_util as S
    import ft8_spec_subtract_gfsk as sg
    from gfsk_effect import waveform
    from rtlsdr_ft8d_amd import workload
    oracle_lib.build()
    set_constants(*consts)
    with waveform(name):
        if traffic == "cq":
            enc = S.oracle_encode_fn(oracle_lib)
            fr = [S.make_frame(s, nsig, enc, snr_range=snr) for s in seeds]
        else:
            texts, tones = workload.mixed_message_pool(1024, seed=7)
            fr = [S.make_mixed_frame(s, nsig, snr, texts, tones) for s in seeds]
    iq = np.stack([f[0] for f in fr])
    msgs, n, nbp, _res = sg.decode_passes_subtracted(oracle_lib, iq, PASSES, shape, nthreads=1)
    return [f[1] for f in fr], msgs, n, nbp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--rows", type=int, nargs="*", help="indices into the rows of tools/multipass_gain.py (default: all)")
    ap.add_argument("--smooth", type=int, default=8)
    ap.add_argument("--range", type=int, default=2)
    ap.add_argument("--tstep", type=int, default=8)
    ap.add_argument("--waveform", choices=("cpfsk", "gfsk"), nargs="+", default=["cpfsk"])
    ap.add_argument("--shape", type=int, choices=(0, 1), nargs="+", default=[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subtract_gain.json"))
    a = ap.parse_args()
    import numpy as np
    import oracle_lib
    oracle_lib.build()
    with open(os.path.join(ROOT, "profiles", "multipass_gain.json")) as f:
        masking = {(r["traffic"], r["signals_per_frame"]): r for r in json.load(f)["rows"]}
    consts = (a.smooth, a.range, a.tstep)
    seeds = list(range(a.seed, a.seed + a.frames))
    per = max(1, (a.frames + 2 * a.threads - 1) // (2 * a.threads))
    rows = []
    plain = a.waveform == ["cpfsk"] and a.shape == [0]                  # the document this tool has always written
    cases = [(k, row, name, shape) for k, row in enumerate(ROWS) for name in a.waveform for shape in a.shape]
    with cf.ProcessPoolExecutor(max_workers=a.threads) as ex:
        for k, (traffic, nsig, snr), name, shape in cases:
            if a.rows and k not in a.rows:
                continue
            t0 = time.time()
            parts = list(ex.map(decode_chunk, [(traffic, nsig, snr, seeds[i:i + per], consts, name, shape) for i in range(0, a.frames, per)]))
            planted = [p for part in parts for p in part[0]]
            msgs = np.concatenate([part[1] for part in parts])
            nbp = np.concatenate([part[3] for part in parts])
            correct, outside = [], []
            for p in range(PASSES):
                hit = miss = 0
                for f in range(len(nbp)):
                    want = set(t for t in planted[f] if t is not None)
                    for r in msgs[f, :int(nbp[f, p])]:
                        if r["text"].decode(errors="replace") in want:
                            hit += 1
                        else:
                            miss += 1
                correct.append(hit)
                outside.append(miss)
            m = masking.get((traffic, nsig))
            same = m is not None and m["frames"] == a.frames and m["planted"] == int(sum(len(set(t for t in p if t is not None)) for p in planted))
            row = dict(traffic=traffic, signals_per_frame=nsig, snr_db=list(snr), frames=a.frames,
                       planted=int(sum(len(set(t for t in p if t is not None)) for p in planted)),
                       correct_by_pass=correct, outside_planted_by_pass=outside,
                       decodes_by_pass=[int(nbp[:, p].sum()) for p in range(PASSES)],
                       gain_pct_by_pass=[round(100.0 * (c / correct[0] - 1.0), 2) if correct[0] else None for c in correct],
                       frames_gaining_in_pass=[int((nbp[:, p] > nbp[:, p - 1]).sum()) for p in range(1, PASSES)],
                       masking_correct_by_pass=m["correct_by_pass"] if same else None,
                       masking_outside_planted_by_pass=m["outside_planted_by_pass"] if same else None,
                       masking_gain_pct_by_pass=m["gain_pct_by_pass"] if same else None,
                       seconds=round(time.time() - t0, 1))
            if not plain:
                row = dict(waveform=name, shape=shape, reference=("cpfsk", "gfsk")[shape], **row)
            rows.append(row)
            print(json.dumps(row), flush=True)
    doc = dict(what="planted messages decoded after each pass with subtraction in the I/Q samples (CPU: the oracle's stages through "
                    "tests/ft8_spec_subtract.py), beside the masking path's figures of profiles/multipass_gain.json",
               command="python tools/subtract_gain.py --frames %d --seed %d" % (a.frames, a.seed) +
                       ("" if plain else " --rows %s --waveform %s --shape %s" % (" ".join(str(k) for k in a.rows or range(len(ROWS))),
                                                                                  " ".join(a.waveform), " ".join(str(v) for v in a.shape))),
               seeds=[a.seed, a.seed + a.frames - 1], max_candidates=120, min_score=10, ldpc_iters=20,
               constants=dict(smooth=a.smooth, range=a.range, tstep=a.tstep),
               mixed_pool="workload.mixed_message_pool(1024, seed=7); a mixed frame carries nsig + 1 signals (one message twice)",
               rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
