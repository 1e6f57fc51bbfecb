"""Hand-made inputs of the second demodulation (tests/test_demod_cpu.py proves on the CPU that they are what they are named for,
tests/test_gpu_demod.py holds the device to the restatement on them).  Signals come from a CPFSK synthesiser of its own, in
float64, which may start a signal before the frame or let it run past its end."""
import numpy as np

import ft8_spec_demod as sdm

NSAMPLES = 48000
CAP = 24                                      # max_candidates of the contexts these inputs are made for
FILL = 0xA5
TEXTS = ("CQ K1ABC FN42", "CQ DL1XYZ JO62", "K1ABC W9XYZ EN37", "W9XYZ K1ABC -11", "CQ JA1ZZZ PM95", "G4ABC F5XYZ RR73",
         "CQ VK3DEF QF22", "PY2AAA LU1BBB GF05")


def tones_of(oracle, text):
    rc, payload = oracle.pack77(text)
    assert rc == 0
    return oracle.encode(payload), payload


def cpfsk(tones, f0_hz, start, amp, phase0=0.0):
    """(I, Q) float64 [48000] of one signal: 79 symbols of 512 samples from sample `start` (any integer), tone 0 at f0_hz"""
    f = f0_hz + 6.25 * np.repeat(np.asarray(tones, np.float64), 512)
    phase = phase0 + 2.0 * np.pi * (np.cumsum(f) - f) / 3200.0
    j = start + np.arange(79 * 512)
    keep = (j >= 0) & (j < NSAMPLES)
    I, Q = np.zeros(NSAMPLES), np.zeros(NSAMPLES)
    I[j[keep]] = amp * np.cos(phase[keep])
    Q[j[keep]] = amp * np.sin(phase[keep])
    return I, Q


def start_of(T, e=0, extra=0):
    return 256 * T + sdm.LEAD + sdm.TSTEP * e + extra


def place(oracle, frame, text, to, ts, fo, fs, e=0, d=0, amp=1.0, dt=0, df=0.0, phase0=0.0):
    """add the signal whose truth lies e time steps, d frequency steps (+ dt samples, df Hz) from the candidate's own place"""
    T, F = 2 * to + ts, 2 * fo + fs
    tones, _payload = tones_of(oracle, text)
    I, Q = cpfsk(tones, 0.78125 * (4 * F + d) + df, start_of(T, e, dt), amp, phase0)
    frame[0] += I
    frame[1] += Q
    return tones


def failing_status(ft8, n, errors=5):
    st = np.zeros(n, ft8.STATUS_DTYPE)
    st["ldpc_errors"], st["iters"] = errors, 20
    return st


def constructed(ft8, oracle):
    """iq [4][2][48000], cands [4][CAP], counts [4], status_in [4][CAP], where {name: (frame, index)}"""
    rng = np.random.default_rng(20260)
    iq = np.zeros((4, 2, NSAMPLES))
    cands = np.zeros((4, CAP), ft8.CAND_DTYPE)
    status = np.zeros((4, CAP), ft8.STATUS_DTYPE)
    counts = np.array([10, 3, CAP, 0], np.int32)
    where = {}

    def cand(f, i, name, to, ts, fo, fs, score=20):
        cands[f, i] = (score, to, fo, ts, fs)
        where[name] = (f, i)

    # frame 0: the edges of the candidate grid and of the search, every sub-step, records that do not qualify
    rows = [("before_the_frame", 0, -12, 0, 0, 0, 0, 0, 1.2), ("past_the_frame", 1, 23, 1, 248, 1, 0, 0, 1.2),
            ("truth_at_e+4_d+2", 2, 5, 0, 60, 0, 4, 2, 1.0), ("truth_at_e-4_d-2", 3, 5, 1, 100, 1, -4, -2, 1.0),
            ("truth_at_e+4_d-2", 4, 8, 0, 140, 1, 4, -2, 1.0), ("truth_at_e-4_d+2", 5, 8, 1, 180, 0, -4, 2, 1.0),
            ("weak", 9, 2, 0, 30, 0, 1, -1, 0.55)]
    for k, (name, i, to, ts, fo, fs, e, d, amp) in enumerate(rows):
        cand(0, i, name, to, ts, fo, fs)
        place(oracle, iq[0], TEXTS[k], to, ts, fo, fs, e, d, amp, phase0=0.7 * k)
    cand(0, 6, "already_decoded", 5, 0, 60, 0)
    cand(0, 7, "bp_left_no_errors", 5, 1, 100, 1)
    cand(0, 8, "noise_only", 10, 0, 220, 0)
    status[0] = failing_status(ft8, CAP)
    status[0, 6]["ok"], status[0, 6]["ldpc_errors"], status[0, 6]["text"] = 1, 0, b"CQ K1ABC FN42"
    status[0, 7]["ldpc_errors"] = 0
    iq[0] += rng.normal(0.0, 3.0, (2, NSAMPLES))
    # frame 1: zeros
    for i, (to, ts, fo, fs) in enumerate([(-12, 0, 0, 0), (6, 1, 90, 1), (23, 1, 248, 1)]):
        cand(1, i, f"zeros_{i}", to, ts, fo, fs)
    status[1] = failing_status(ft8, CAP)
    # frame 2: a full list; an infinite sample that only the late candidates' windows reach
    for i in range(CAP):
        to, fo = (-3 + i if i < 12 else i), 8 + 10 * i
        cand(2, i, f"full_{i}", to, i & 1, fo, (i >> 1) & 1, score=40 - i)
        if i % 3 == 0:
            place(oracle, iq[2], TEXTS[(i // 3) % len(TEXTS)], to, i & 1, fo, (i >> 1) & 1, (i % 5) - 2, (i % 4) - 2, 0.5 + 0.05 * i, dt=3, df=0.2)
    status[2] = failing_status(ft8, CAP, errors=9)
    status[2, 5]["ok"], status[2, 5]["ldpc_errors"] = 1, 0
    iq[2] += rng.normal(0.0, 3.0, (2, NSAMPLES))
    iq[2, 0, 47000] = np.inf
    # frame 3: no candidates; its list holds the fill pattern
    cands[3] = np.frombuffer(bytes([FILL]) * (8 * CAP), ft8.CAND_DTYPE)
    status[3] = np.frombuffer(bytes([FILL]) * (48 * CAP), ft8.STATUS_DTYPE)
    return iq.astype(np.float32), cands, counts, status, where


def radio(ft8, oracle, seed=7, frames=5, signals=6, sigma=3.0, amps=(0.36, 0.62)):
    """frames of off-grid signals near BP's threshold -> (iq [frames][2][48000] float32, the planted texts per frame)"""
    rng = np.random.default_rng(seed)
    iq = np.zeros((frames, 2, NSAMPLES))
    planted = []
    for f in range(frames):
        texts = []
        for s in range(signals):
            text = TEXTS[(f + s) % len(TEXTS)]
            tones, _payload = tones_of(oracle, text)
            f0 = 200.0 + 220.0 * s + rng.uniform(0.0, 100.0)
            start = int(rng.integers(1500, 7500))
            I, Q = cpfsk(tones, f0, start, rng.uniform(*amps), rng.uniform(0.0, 2.0 * np.pi))
            iq[f, 0] += I
            iq[f, 1] += Q
            texts.append(text)
        iq[f] += rng.normal(0.0, sigma, (2, NSAMPLES))
        planted.append(texts)
    return iq.astype(np.float32), planted
