"""Constructed inputs of the GFSK synthesiser's tests (tests only): signal records from plain tuples, the five-signal clip of
tests/audio_craft.py built as GFSK, the eight -16 dB I/Q frames, and the byte-identity cases of tests/test_gpu_gfsk.py."""
import numpy as np

import audio_craft as ac
import ft8_spec_gfsk as sg
import synth_util as S

F = np.float32
SIGNAL_DTYPE = np.dtype([("tones", "u1", (79,)), ("pad", "u1"), ("f0_hz", "<f4"), ("t0_s", "<f4"), ("amplitude", "<f4")])


def records(clips):
    """clips: a list (clips) of lists of (tones, f0_hz, t0_s, amplitude), the same number in every clip -> SIGNAL_DTYPE [nclips][nsig]"""
    nsig = len(clips[0])
    out = np.zeros((len(clips), nsig), SIGNAL_DTYPE)
    for c, sigs in enumerate(clips):
        assert len(sigs) == nsig
        for s, (tones, f0, t0, amp) in enumerate(sigs):
            out[c, s]["tones"] = tones
            out[c, s]["f0_hz"], out[c, s]["t0_s"], out[c, s]["amplitude"] = F(f0), F(t0), F(amp)
    return out


def tones_of(oracle, text):
    rc, payload = oracle.pack77(text)
    assert rc == 0
    return np.asarray(oracle.encode(payload[:10]), np.uint8)


def random_tones(seed):
    return np.random.default_rng(seed).integers(0, 8, 79).astype(np.uint8)


# ---- the five signals of audio_craft.five_signal_clip as GFSK audio -----------------------------------------------------------------
def five_signals(oracle):
    return [(tones_of(oracle, text), f0, t0, ac.AMPLITUDE) for text, f0, t0 in ac.PLANTED]


def five_signal_clip_gfsk(oracle):
    """int16 [180000]: the restated GFSK signals in audio_craft's noise, rounded as audio_craft rounds"""
    x = sg.clip(five_signals(oracle), sg.AUDIO, ac.N).astype(np.float64) + ac.noise(5)
    return ac.to_s16(x)


FIVE_SIGMA = float(np.sqrt((ac.AMPLITUDE ** 2 / 2) * 6000 / 2500))     # audio_craft.noise's sigma, for the device's generator


# ---- eight I/Q frames of one GFSK signal each at -16 dB --------------------------------------------------------------------------------
EIGHT_TEXT, EIGHT_SNR_DB = "CQ K1ABC FN42", -16.0


def eight_signals(oracle):
    """[frame] -> [(tones, f0, t0_s, amplitude)]: f0 = 700 + 3.1 s, start = 1600 + 37 s samples, noise sigma 1"""
    tones = tones_of(oracle, EIGHT_TEXT)
    amp = S.amplitude_for_snr(EIGHT_SNR_DB, 1.0)
    return [[(tones, 700.0 + 3.1 * s, (1600 + 37 * s) / 3200.0, amp)] for s in range(8)]


def eight_frames(oracle):
    """float32 [8][2][48000]: restated signal + numpy noise of seeds 100 .. 107, peak-normalised to 0.5"""
    out = np.zeros((8, 2, sg.NSAMPLES_IQ), F)
    for s, sigs in enumerate(eight_signals(oracle)):
        assert sg.start_of(sigs[0][2], sg.IQ) == 1600 + 37 * s
        noise = np.random.default_rng(100 + s).normal(0.0, 1.0, (2, sg.NSAMPLES_IQ)).astype(F)
        out[s] = sg.normalise(sg.clip(sigs, sg.IQ) + noise, 0.5)
    return out


def decoded_texts(oracle, frame):
    dec, n = oracle.subsystem(frame[0], frame[1])
    return [f"CQ {dec[k]['call'].decode()} {dec[k]['loc'].decode()}" for k in range(n)]


# ---- byte-identity cases -----------------------------------------------------------------------------------------------------------------
def case_signals(mode, nsig):
    """nsig signals that between them start before 0, at 0, across tile seams and end behind the clip, with f0 at 0, at multiples
    of 6.25, at an arbitrary float, just under the rate and (I/Q) negative; amplitudes include 2^-130 and 2^100"""
    rate = sg.RATE[mode]
    f0s = [0.0, 6.25 * 160, 1234.5677490234375, float(np.nextafter(F(rate), F(0))), 6.25 * 300, 2718.28]
    if mode == sg.IQ:
        f0s += [-431.7, -6.25 * 40]
    t0s = [-0.5, 0.0, (2048 - 100) / rate, 14.0, 0.64, 2.0 + 1.0 / 3.0, 8.5, -12.0]
    amps = [1.0, 0.25, 2.0 ** -130, 2.0 ** 100, 0.7, 3.0]
    out = []
    for s in range(nsig):
        out.append((random_tones(1000 + s), f0s[s % len(f0s)], t0s[(s * 3 + s // 8) % len(t0s)], amps[s % len(amps)] if nsig <= 8 else amps[s % 2]))
    return out
