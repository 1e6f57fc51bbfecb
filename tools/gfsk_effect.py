#!/usr/bin/env python3
"""What pulse shaping does to the I/Q stages, on the CPU (no GPU needed): the quantities of the existing tools measured twice, on
the CPFSK signals those tools synthesise and on GFSK signals (tests/ft8_spec_gfsk.py) with the same tones, frequencies, start
samples, amplitudes, noise seeds and frame counts.  The GFSK runs replace the two CPFSK synthesisers the tools call
(tests/synth_util.cpfsk and oracle_lib.synth_cpfsk) and leave everything else as it is, so the CPFSK figures are the committed
ones again.

  python tools/gfsk_effect.py [--out profiles/gfsk_effect.json] [--procs 8] [--parts decodes,refine,depth,passes]

  decodes  the 96 crowded CQ frames of 20 signals of tools/demod_gain.py: planted messages belief propagation decodes, and what the
           demodulation from the I/Q samples gains at the committed gate and mask (profiles/demod_gain.json "chosen")
  refine   tools/refine_accuracy.py: median and 90th percentile of the refined frequency and time error, 256 single-signal frames
           per set
  depth    tools/subtract_accuracy.py: 10 log10(|x' - (x - s)|^2 / |s|^2), s the noiseless waveform as synthesised (the GFSK one in
           the GFSK run), 64 frames per set
  passes   tools/subtract_gain.py, rows cq 20 and cq 45: planted messages after 1, 2 and 3 passes, 96 frames each
On the GFSK run, depth and passes are measured once more with the GFSK reference of the subtraction (shape 1 of
tests/ft8_spec_subtract_gfsk.py; "cancellation_depth_gfsk_reference", "passes_gfsk_reference"): the same frames, the other
reference.  profiles/subtract_gfsk_accuracy.json and profiles/subtract_gfsk_gain.json hold those figures from the tools themselves.
No threshold is set on any of these figures."""
import argparse
import contextlib
import json
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WAVEFORMS = ("cpfsk", "gfsk")


def gfsk_planes(tones, f0_hz, start_sample, amplitude, n=48000):
    """tests/synth_util.cpfsk's signature with the restated GFSK waveform: (i, q) float64 [n]"""
    import numpy as np
    import ft8_spec_gfsk as sg
    x = sg.contribution(np.asarray(tones, np.uint8), f0_hz, amplitude, sg.IQ).astype(np.float64)
    out = np.zeros((2, n))
    start = int(start_sample)
    lo, hi = max(start, 0), min(start + x.shape[1], n)
    if lo < hi:
        out[:, lo:hi] = x[:, lo - start:hi - start]
    return out[0], out[1]


def gfsk_synth(tones, f_tone0_hz, start_sample, amplitude):
    """oracle_lib.synth_cpfsk's signature: S signals summed, (i, q) float32 [48000]"""
    import numpy as np
    tones = np.ascontiguousarray(tones, np.uint8).reshape(-1, 79)
    total = np.zeros((2, 48000))
    for s in range(tones.shape[0]):
        i, q = gfsk_planes(tones[s], float(f_tone0_hz[s]), int(start_sample[s]), float(amplitude[s]))
        total[0] += i
        total[1] += q
    return total[0].astype(np.float32), total[1].astype(np.float32)


@contextlib.contextmanager
def waveform(name):
    """inside: the tools' synthesisers make `name`"""
    import oracle_lib
    import synth_util
    assert name in WAVEFORMS
    saved = (synth_util.cpfsk, oracle_lib.synth_cpfsk)
    if name == "gfsk":
        synth_util.cpfsk, oracle_lib.synth_cpfsk = gfsk_planes, gfsk_synth
    try:
        yield
    finally:
        synth_util.cpfsk, oracle_lib.synth_cpfsk = saved


# ---- workers (one process each: the numpy restatements are single-threaded) ----------------------------------------------------------
def demod_frame(job):
    name, inner = job
    import demod_gain
    with waveform(name):
        return demod_gain.one_frame(inner)


def passes_chunk(job):
    name, inner, shape = job
    import subtract_gain
    return subtract_gain.decode_chunk(inner + (name, shape))


def part_decodes(pool, name, chosen):
    import demod_gain
    row = next(r for r in demod_gain.ROWS if r[0] == "cq20")
    _, nsig, snr, seed0, frames = row
    per = pool.map(demod_frame, [(name, (s, nsig, snr)) for s in range(seed0, seed0 + frames)], chunksize=1)
    g, m = chosen["max_hard_errors"], chosen["sets"]
    return dict(frames=frames, seeds=[seed0, seed0 + frames - 1], planted=sum(p["planted"] for p in per),
                bp_planted=sum(p["bp_hit"] for p in per), bp_outside=sum(p["bp_miss"] for p in per),
                failing_candidates=sum(p["failing"] for p in per), demod_gate=g, demod_sets=m,
                demod_new_planted=sum(p["res"][g][m][0] for p in per), demod_outside=sum(p["res"][g][m][1] for p in per))


def part_refine(name, threads):
    import oracle_lib
    import refine_craft as rc
    out = {}
    with waveform(name):
        for label, snr, seed in (("strong", rc.STRONG_DB, 1), ("weak", rc.WEAK_DB, 2)):
            iq, f0, start, text = rc.accuracy_frames(oracle_lib, 256, snr, seed)
            s = rc.summary(rc.accuracy(oracle_lib, iq, f0, start, text, nthreads=threads))
            s["true_snr_db"] = snr
            out[label] = s
    return out


def part_depth(name, threads, shape=0):
    import numpy as np
    import oracle_lib
    import ft8_spec_subtract_gfsk as sg
    import subtract_craft as sc
    out = []
    with waveform(name):
        for label, snr, seed in (("noiseless", None, 1), ("0dB", 0.0, 2), ("-18dB", -18.0, 3)):
            iq, s, _f0, _start = sc.suppression_frames(oracle_lib, 64, snr, seed)
            with sg.rule(shape):
                db = sc.suppression_db(oracle_lib, iq, s, nthreads=threads)
            out.append({"set": label, "snr_db": snr, "decoded": int(len(db)), "median_db": round(float(np.median(db)), 2),
                        "p90_db": round(float(np.percentile(db, 90)), 2), "worst_db": round(float(db.max()), 2)})
    return out


def part_passes(pool, name, procs, shape=0):
    import numpy as np
    from multipass_gain import PASSES, ROWS
    frames, seed0 = 96, 1000
    seeds = list(range(seed0, seed0 + frames))
    per = max(1, (frames + 2 * procs - 1) // (2 * procs))
    rows = []
    for traffic, nsig, snr in (ROWS[0], ROWS[2]):
        assert (traffic, nsig) in (("cq", 20), ("cq", 45))
        parts = pool.map(passes_chunk, [(name, (traffic, nsig, snr, seeds[i:i + per], (8, 2, 8)), shape) for i in range(0, frames, per)], chunksize=1)
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
        rows.append(dict(traffic=traffic, signals_per_frame=nsig, snr_db=list(snr), frames=frames, seeds=[seed0, seed0 + frames - 1],
                         planted=int(sum(len(set(t for t in p if t is not None)) for p in planted)), correct_by_pass=correct,
                         outside_planted_by_pass=outside,
                         gain_pct_by_pass=[round(100.0 * (c / correct[0] - 1.0), 2) if correct[0] else None for c in correct]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--parts", default="decodes,refine,depth,passes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gfsk_effect.json"))
    a = ap.parse_args()
    import oracle_lib
    oracle_lib.build()
    oracle_lib.lib()
    with open(os.path.join(ROOT, "profiles", "demod_gain.json")) as f:
        chosen = json.load(f)["chosen"]
    parts = a.parts.split(",")
    doc = dict(what="the I/Q stages on CPFSK and on GFSK signals with the same tones, places, noise seeds and frame counts (CPU: the "
                    "oracle's stages and the numpy restatements; tools/gfsk_effect.py)",
               command="python tools/gfsk_effect.py", max_candidates=120, min_score=10, ldpc_iters=20)
    with mp.Pool(a.procs) as pool:
        for name in WAVEFORMS:
            t0 = time.time()
            res = {}
            if "decodes" in parts:
                res["decodes_cq20"] = part_decodes(pool, name, chosen)
            if "refine" in parts:
                res["refine"] = part_refine(name, a.procs)
            if "depth" in parts:
                res["cancellation_depth"] = part_depth(name, a.procs)
                if name == "gfsk":
                    res["cancellation_depth_gfsk_reference"] = part_depth(name, a.procs, shape=1)
            if "passes" in parts:
                res["passes"] = part_passes(pool, name, a.procs)
                if name == "gfsk":
                    res["passes_gfsk_reference"] = part_passes(pool, name, a.procs, shape=1)
            res["seconds"] = round(time.time() - t0, 1)
            doc[name] = res
            print(name, json.dumps(res), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
