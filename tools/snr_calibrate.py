"""Calibration of the SNR estimate of the messages path (CPU only, the oracle's stages): frames with one signal each at a
known SNR in 2500 Hz (the oracle's CPFSK synth + AWGN + the decoder thread's peak normalisation), the oracle's waterfall /
find_sync / decode, the estimate's continuous form 10 log10(q S / (nsym P[nb]) - 1) (tests/ft8_spec_messages.py); K is
the median of (estimate - truth), d0 the median of (dt_s - s0 / 3200) where s0 is the synthesised start sample.

  python tools/snr_calibrate.py [--frames 720] [--out profiles/snr_calibration.json]

K goes into csrc/api_messages.hip (kSnrCalibrationK), rounded to 0.01 dB; d0 is read by tests/test_gpu_messages.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 0x534E52          # "SNR"


def synth_frames(oracle, nframes, snr_lo, snr_hi, seed, traffic_texts=None):
    """[n][2][48000] frames with one CQ signal each -> (iq, truth snr, start samples, texts)"""
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    rng = np.random.default_rng(seed)
    texts, tones = workload.message_pool(256, seed=seed & 0xFFFF)
    iq = np.zeros((nframes, 2, ft8.NSAMPLES), np.float32)
    snr = rng.uniform(snr_lo, snr_hi, nframes) if snr_hi > snr_lo else np.full(nframes, float(snr_lo))
    s0 = rng.integers(0, int(1.8 * 3200), nframes)
    picks = rng.integers(0, len(texts), nframes)
    f0 = rng.uniform(100.0, 1500.0, nframes)
    for k in range(nframes):
        si, sq = oracle.synth_cpfsk(tones[picks[k]], [f0[k]], [s0[k]], [float(workload.amplitude_for_snr(snr[k]))])
        ni, nq = rng.normal(0.0, 1.0, (2, ft8.NSAMPLES))
        iq[k, 0], iq[k, 1] = oracle.normalise((si + ni).astype(np.float32), (sq + nq).astype(np.float32))
    return iq, snr, s0, [texts[p] for p in picks]


def measure(oracle, iq, snr, s0, texts, k=0.0):
    """(continuous estimate - truth, dt - s0/3200, truth) for every frame whose planted message was decoded"""
    import ft8_spec_messages as spec
    mag, cands, counts, status = spec.oracle_stages(oracle, iq)
    msgs, n = spec.collect(mag, cands, counts, status)
    base = spec.noise_baseline(mag)
    err, dt, truth, est_db = [], [], [], []
    for f in range(len(n)):
        for j in range(int(n[f])):
            m = msgs[f, j]
            if m["text"].decode() != texts[f]:
                continue
            S, nsym, nb = spec.snr_parts(mag[f], base[f], m["cand"], spec.tones_of(m["a91"]))
            e = spec.snr_continuous(S, nsym, nb, k)
            if e is None:
                continue
            err.append(e - snr[f])
            dt.append(float(m["dt_s"]) - s0[f] / 3200.0)
            truth.append(float(snr[f]))
            est_db.append(int(m["snr_db"]))
    return np.array(err), np.array(dt), np.array(truth), np.array(est_db)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=720)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snr_calibration.json"))
    a = ap.parse_args()
    import oracle_lib as oracle
    oracle.build()
    t0 = time.time()
    iq, snr, s0, texts = synth_frames(oracle, a.frames, -20.0, 20.0, SEED)
    err, dt, truth, _ = measure(oracle, iq, snr, s0, texts, 0.0)
    K = float(np.median(err))
    d0 = float(np.median(dt))
    resid = err - round(K, 2)
    bins = {}
    for lo in range(-20, 20, 5):
        sel = (truth >= lo) & (truth < lo + 5)
        if sel.any():
            bins[f"{lo}..{lo + 5}"] = dict(decodes=int(sel.sum()), median_error_db=round(float(np.median(resid[sel])), 3),
                                           max_abs_error_db=round(float(np.abs(resid[sel]).max()), 3))
    res = dict(tool="tools/snr_calibrate.py", frames=a.frames, seed=SEED, snr_range_db=[-20.0, 20.0], decodes=int(len(err)),
               K=round(K, 2), K_unrounded=K, d0_s=round(d0, 4),
               residual_db=dict(median_abs=round(float(np.median(np.abs(resid))), 3), p95_abs=round(float(np.percentile(np.abs(resid), 95)), 3),
                                max_abs=round(float(np.abs(resid).max()), 3)),
               dt_minus_start_s=dict(median=round(d0, 4), min=round(float(dt.min()), 4), max=round(float(dt.max()), 4)),
               by_truth_db=bins, seconds=round(time.time() - t0, 1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
