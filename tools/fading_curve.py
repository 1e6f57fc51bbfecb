#!/usr/bin/env python3
"""Decode probability against SNR under HF fading: one planted station per frame in 1 dB steps, in white noise alone ("awgn") and
under the four channel presets of include/ft8gpu.h ("Fading channel"), and a crowd of 20 stations per frame through three passes
of subtraction in both reference shapes.  The same tones, frequencies, start times and noise seeds under every channel.

  python tools/fading_curve.py [--out profiles/fading_curve.json] [--frames 1024] [--crowd-frames 128] [--snr -24 -8]
                               [--channels awgn quiet moderate disturbed flutter]
  python tools/fading_curve.py --cpu --frames 4 --snr -12 -10 --out /tmp/curve.json

On the GPU (the default) the frames come from ft8gpu_synth_gfsk_frames_faded (noise sigma 1 from the device's generator, peak
0.5) and stay in HBM; every SNR point of every channel goes through
  bp        ft8gpu_decode_messages
  deep      ft8gpu_decode_messages_ap with the hypothesis "CQ ? ?" and OSD of order 1 (the deep path: AP + OSD)
  demod     ft8gpu_decode_messages_demod at the recommended gate and mask
  demod_ap  ft8gpu_decode_messages_demod_ap: the same, then AP under "CQ ? ?" on the demodulated soft bits at its recommended gate
and the crowd frames (20 stations, all at the point's SNR, 70 Hz apart) through
  subtract_cpfsk, subtract_gfsk   ft8gpu_decode_messages_subtracted_shaped, three passes: planted messages after each pass.
A station counts as decoded when its text is among the frame's records.  --cpu: the restated rule (tests/ft8_spec_channel.py) with
numpy noise, and the oracle's whole path (its CQ spots) as the only stage, "bp": slow, for a handful of frames (a CPU test runs
it).  No threshold is set on any of these figures; the file records what was measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHANNELS = ("awgn", "quiet", "moderate", "disturbed", "flutter")
NCROWD, SEED = 20, 0x4654


def single_signals(ft8, workload, nframes, snr_db):
    """one station per frame: frame f sends message f of the CQ pool at 600 .. 1400 Hz from 0.3 .. 1.3 s; the draw does not depend
    on the SNR or the channel"""
    texts, tones = workload.message_pool(256, seed=11)
    rng = np.random.default_rng(SEED)
    s = np.zeros((nframes, 1), ft8.SIGNAL_DTYPE)
    pick = np.arange(nframes) % len(texts)
    s["tones"][:, 0] = tones[pick]
    s["f0_hz"][:, 0] = rng.uniform(600.0, 1400.0, nframes)
    s["t0_s"][:, 0] = rng.uniform(0.3, 1.3, nframes)
    s["amplitude"] = workload.amplitude_for_snr(snr_db, 1.0)
    return s, [texts[k] for k in pick]


def crowd_signals(ft8, workload, nframes, snr_db):
    """20 stations per frame, 70 Hz apart from 150 Hz up in a shuffled order (the top one ends at 1536 Hz, inside the decoder's band),
    from 0.2 .. 1.6 s, all at snr_db"""
    texts, tones = workload.message_pool(1024, seed=12)
    rng = np.random.default_rng(SEED + 1)
    s = np.zeros((nframes, NCROWD), ft8.SIGNAL_DTYPE)
    pick = np.stack([rng.choice(len(texts), NCROWD, replace=False) for _ in range(nframes)])
    s["tones"] = tones[pick]
    s["f0_hz"] = np.stack([rng.permutation(NCROWD) for _ in range(nframes)]) * 70.0 + 150.0 + rng.uniform(0.0, 6.25, (nframes, NCROWD))
    s["t0_s"] = rng.uniform(0.2, 1.6, (nframes, NCROWD))
    s["amplitude"] = workload.amplitude_for_snr(snr_db, 1.0)
    return s, [[texts[k] for k in row] for row in pick]


def channels_of(ft8, name, shape):
    return None if name == "awgn" else ft8.channel_preset(name, shape)


def texts_of(msgs, n):
    return [set(r["text"].decode(errors="replace") for r in msgs[f, :int(n[f])]) for f in range(len(n))]


def run_gpu(a):
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    F, FC = a.frames, a.crowd_frames
    snrs = list(range(a.snr[0], a.snr[1] + 1))
    doc = dict(mode="gpu", build_id=ft8.check_build_id(), frames=F, crowd_frames=FC, crowd_signals=NCROWD, snr_db=snrs, noise_sigma=1.0, peak=0.5,
               max_candidates=120, min_score=10, ldpc_iters=20, demod_gate=ft8.DEMOD_MAX_HARD_ERRORS, demod_sets=ft8.DEMOD_SETS,
               presets={k: list(v) for k, v in ft8.CHANNEL_PRESETS.items()}, curves={}, crowd={})
    B = max(F, FC)
    with ft8.Decoder(device=0, max_frames=B) as dec:
        iq = torch.zeros((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        msgs = torch.zeros(B * ft8.MAX_MESSAGES * ft8.MESSAGE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        n = torch.zeros(B, dtype=torch.int32, device="cuda")
        by = torch.zeros(B * 3, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def fetch(count):
            dec.synchronize()
            m = msgs.cpu().numpy().view(ft8.MESSAGE_DTYPE).reshape(B, ft8.MAX_MESSAGES)[:count]
            return m, n.cpu().numpy()[:count]

        for name in a.channels:
            t0 = time.time()
            curves = {"bp": [], "deep": [], "demod": [], "demod_ap": []}
            crowd = {"subtract_cpfsk": [], "subtract_gfsk": []}
            for k, snr in enumerate(snrs):
                sig, want = single_signals(ft8, workload, F, snr)
                dec.synth_gfsk_frames_faded_dev(sig, channels_of(ft8, name, sig.shape), F, 1, 1.0, SEED + k, 0, 0.5, iq)
                stages = {"bp": lambda: dec.decode_messages_dev(iq, F, msgs, n),
                          "deep": lambda: dec.decode_messages_ap_dev(iq, F, 1, ("CQ ? ?",), ft8.AP_MAX_HARD_ERRORS, 1, ft8.OSD_MAX_HARD_ERRORS, msgs, n),
                          "demod": lambda: dec.decode_messages_demod_dev(iq, F, ft8.DEMOD_SETS, ft8.DEMOD_MAX_HARD_ERRORS, 120, msgs, n),
                          "demod_ap": lambda: dec.decode_messages_demod_ap_dev(iq, F, ft8.DEMOD_SETS, ft8.DEMOD_MAX_HARD_ERRORS, 120, ("CQ ? ?",),
                                                                               ft8.APSOFT_MAX_HARD_ERRORS, msgs, n)}
                for stage, run in stages.items():
                    run()
                    got = texts_of(*fetch(F))
                    curves[stage].append(sum(want[f] in got[f] for f in range(F)))
                if FC < 1:                                            # --crowd-frames 0: the single-station rows only
                    continue
                sig, wantc = crowd_signals(ft8, workload, FC, snr)
                dec.synth_gfsk_frames_faded_dev(sig, channels_of(ft8, name, sig.shape), FC, NCROWD, 1.0, SEED + 100 + k, 0, 0.5, iq)
                for stage, shape in (("subtract_cpfsk", ft8.SUBTRACT_CPFSK), ("subtract_gfsk", ft8.SUBTRACT_GFSK)):
                    dec.decode_messages_subtracted_dev(iq, FC, 3, msgs, n, by, None, shape)
                    m, cnt = fetch(FC)
                    nb = by.cpu().numpy()[:FC * 3].reshape(FC, 3)
                    hits = [0, 0, 0]
                    for f in range(FC):
                        w = set(wantc[f])
                        for p in range(3):
                            hits[p] += sum(r["text"].decode(errors="replace") in w for r in m[f, :int(nb[f, p])])
                    crowd[stage].append(hits)
            doc["curves"][name] = curves
            doc["crowd"][name] = dict(planted_per_point=FC * NCROWD, decoded_after_pass=crowd)
            print(name, json.dumps(curves), json.dumps(crowd), f"{time.time() - t0:.1f} s", flush=True)
    return doc


def run_cpu(a):
    import ft8_spec_channel as sc
    import ft8_spec_gfsk as sg
    import gfsk_craft as gc
    import oracle_lib
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    oracle_lib.build()
    oracle_lib.lib()
    F = a.frames
    snrs = list(range(a.snr[0], a.snr[1] + 1))
    doc = dict(mode="cpu", frames=F, snr_db=snrs, noise_sigma=1.0, peak=0.5, presets={k: list(v) for k, v in sc.PRESETS.items()}, curves={})
    for name in a.channels:
        hits = []
        for k, snr in enumerate(snrs):
            sig, want = single_signals(ft8, workload, F, snr)
            count = 0
            for f in range(F):
                r = sig[f, 0]
                one = [(r["tones"], float(r["f0_hz"]), float(r["t0_s"]), float(r["amplitude"]))]
                x = sc.clip(one, None if name == "awgn" else [sc.PRESETS[name]], sg.IQ, None, SEED + k, f)
                noise = np.random.default_rng([SEED + k, f]).normal(0.0, 1.0, (2, sg.NSAMPLES_IQ)).astype(np.float32)
                frame = sg.normalise(x + noise, 0.5)
                count += want[f] in gc.decoded_texts(oracle_lib, frame)
            hits.append(count)
        doc["curves"][name] = {"bp": hits}
        print(name, hits, flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fading_curve.json"))
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--crowd-frames", type=int, default=128)
    ap.add_argument("--snr", type=int, nargs=2, default=[-24, -8])
    ap.add_argument("--channels", nargs="+", default=list(CHANNELS), choices=CHANNELS)
    a = ap.parse_args()
    doc = dict(what="decode probability against SNR in white noise and under the HF channel presets (tools/fading_curve.py): per channel and "
                    "stage, the number of frames (of `frames`) whose planted station was decoded at each entry of snr_db",
               command="python tools/fading_curve.py" + (" --cpu" if a.cpu else ""))
    doc.update(run_cpu(a) if a.cpu else run_gpu(a))
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
