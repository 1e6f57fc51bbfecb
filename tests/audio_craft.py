"""Constructed 12 kHz clips for the audio front end (tests only): the five-signal clip of tests/test_audio_cpu.py and
tests/test_gpu_audio.py, and the edge clips of the stage parity test."""
import numpy as np

import ft8_spec_audio as sa

RATE, N = sa.RATE, sa.NSAMPLES_AUDIO
AMPLITUDE = 0.02
# message, frequency of tone 0 (Hz), start (s)
PLANTED = (("CQ K1ABC FN42", 700.0, 0.5), ("CQ DL1XYZ JO62", 2300.0, 0.8), ("CQ JA1AAA PM95", 1525.0, 0.3),
           ("CQ VK2BBB QF56", 1562.5, 1.0), ("CQ W9XYZ EN52", 3040.0, 0.0))
BANDS = (0, 240)
# what each band can hold: band 0 ends at 1600 Hz and a candidate needs freq_offset + 7 < 256, so 1562.5 Hz is out of its reach
IN_BAND = {0: ("CQ K1ABC FN42", "CQ JA1AAA PM95"), 240: ("CQ JA1AAA PM95", "CQ DL1XYZ JO62", "CQ W9XYZ EN52", "CQ VK2BBB QF56")}


def cpfsk(tones, f0_hz, start_s, amplitude=AMPLITUDE):
    """cos of the cumulative phase at 12 kHz, 1920 samples per symbol, float64 [180000]"""
    f = np.repeat(f0_hz + 6.25 * np.asarray(tones, np.float64), 1920)
    x = amplitude * np.cos(np.cumsum(2.0 * np.pi * f / RATE))
    out = np.zeros(N)
    s = int(round(start_s * RATE))
    n = min(x.size, N - s)
    out[s:s + n] = x[:n]
    return out


def noise(seed=5):
    """white noise at 0 dB in 2500 Hz against a signal of AMPLITUDE"""
    sigma = np.sqrt((AMPLITUDE ** 2 / 2) * 6000 / 2500)
    return np.random.default_rng(seed).normal(0, sigma, N)


def to_s16(x):
    return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)


def five_signal_clip(oracle):
    """int16 [180000]: the five planted signals in noise"""
    x = noise(5)
    for text, f0, t0 in PLANTED:
        rc, payload = oracle.pack77(text)
        assert rc == 0
        x = x + cpfsk(oracle.encode(payload[:10]), f0, t0)
    return to_s16(x)


def planted_hz(text):
    return {t: f for t, f, _ in PLANTED}[text]


def text_of(rec):
    return bytes(rec["text"]).split(b"\0")[0].decode()


# ---- the stage parity inputs: three clips per (format, nsamples) ------------------------------------------------------------------
def s16_clips(nsamples):
    """seeded Gaussian noise; zero but for -32768 at sample 0 and +32767 at the last sample; all zeros"""
    pcm = np.zeros((3, nsamples), np.int16)
    pcm[0] = to_s16(np.random.default_rng(11).normal(0, 0.2, nsamples))
    pcm[1, 0] = -32768
    pcm[1, -1] = 32767                                     # (nsamples = 1: the one sample is the last)
    return pcm


NAN_BITS = 0xFFC00001                                       # a quiet NaN with its sign set and a payload


def f32_clips(nsamples):
    """seeded Gaussian noise; a NaN, both infinities, a subnormal and 1e30 at known samples (as many as fit); all zeros"""
    pcm = np.zeros((3, nsamples), np.float32)
    pcm[0] = np.random.default_rng(12).normal(0, 0.2, nsamples).astype(np.float32)
    pcm[1] = np.random.default_rng(13).normal(0, 0.01, nsamples).astype(np.float32)
    special = ((0, np.array([NAN_BITS], np.uint32).view(np.float32)[0]), (3, np.float32(np.inf)), (5, np.float32(-np.inf)),
               (6, np.float32(1e-41)), (1000, np.float32(1e30)), (90001, np.float32(np.inf)), (179000, np.float32(1e-45)))
    for at, v in special:
        if at < nsamples:
            pcm[1, at] = v
    return pcm
