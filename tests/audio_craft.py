"""Constructed 12 kHz clips for the audio front end (tests only): the five-signal clip of tests/test_audio_cpu.py and
tests/test_gpu_audio.py, the edge clips of the stage parity test, the stage in double from its definition with its rounding
bound, impulse clips and their closed form, the clip lengths at the kernel's seams, and the twelve-signal clip of the merge test."""
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


# ---- the stage from its definition, in double -------------------------------------------------------------------------------------
U = 2.0 ** -24                                              # unit roundoff of float32
_J = np.array([1, 1j, -1, -1j])
_M = np.arange(sa.NSAMPLES, dtype=np.int64)


def _at_outputs(up, h):
    """(up * h)[15 m + 79], m = 0 .. 47999; zero where the convolution has ended"""
    full = np.convolve(up, h)
    full = np.concatenate([full, np.zeros(max(0, 15 * sa.NSAMPLES + 79 - full.size))])
    return full[15 * _M + 79]


def ref64(a, base_bin):
    """The stage as it is defined, not as include/ft8gpu.h restates it: mix, zero-stuff by 4, the 159-tap FIR at 48 kHz, every
    15th sample, rotate by j^m.  a: the samples [nsamples] (as float32 holds them) -> (x float64 [2][48000], bound [48000]).
    bound: what one component of the float32 rule may differ from x by.  A component is 40 products summed one after the other:
    the table entry, a * c, h * z and each of the 39 adds after the first are one rounding each, at most U relative to the sum of
    the magnitudes S[m] = sum |h[k]| |a[n]| over the window (the same convolution on absolute values), so 44 U S[m] in first
    order; 40 * 2^-149 more for products that underflow."""
    a = np.asarray(a, np.float64)
    h = sa.taps().astype(np.float64)
    n = np.arange(a.size, dtype=np.int64)
    z = a * np.exp(-2j * np.pi * ((n * (base_bin + 128)) % 1920) / 1920.0)
    up = np.zeros(4 * a.size, np.complex128)
    up[0::4] = z
    y = _at_outputs(up.real, h) + 1j * _at_outputs(up.imag, h)
    x = y * _J[_M % 4]                                      # (a multiplication by 1, j, -1 or -j is exact)
    S = _at_outputs(np.abs(up), np.abs(h))
    return np.stack([x.real, x.imag]), 44.0 * U * S + 40.0 * 2.0 ** -149


def worst_ratio(got, a, base_bin):
    """max over both components of |got - ref64| / (U S): at most 44 by the bound; the bound itself is asserted"""
    x, bound = ref64(a, base_bin)
    err = np.abs(np.asarray(got, np.float64) - x)
    assert np.isfinite(err).all()
    over = np.argwhere(err > bound[None])
    assert len(over) == 0, f"base {base_bin}: {len(over)} components beyond the bound, the first at {over[0].tolist()}: " \
                           f"error {err[tuple(over[0])]:.3e}, bound {bound[over[0][1]]:.3e}"
    S = (bound - 40.0 * 2.0 ** -149) / (44.0 * U)
    return float((err[:, S > 0] / (U * S[S > 0])).max())


REF64_BASES, REF64_LENGTHS = (3, 701, 704), (180000, 2857)


def noise_clip(fmt, nsamples):
    """the dense noise clip of the stage parity test, alone"""
    return (s16_clips(nsamples) if fmt == sa.S16 else f32_clips(nsamples))[0]


# ---- the rotation and the outputs past a clip's end -------------------------------------------------------------------------------
def rotate(y):
    """x[m] = y[m] * j^m as the rule spells it: a negation flips the sign bit, also that of a zero.  float32 [2][48000]"""
    yr, yi = np.asarray(y, np.float32)
    q = _M % 4
    return np.stack([np.where(q == 0, yr, np.where(q == 1, -yi, np.where(q == 2, -yr, yi))),
                     np.where(q == 0, yi, np.where(q == 1, yr, np.where(q == 2, -yi, -yr)))]).astype(np.float32)


SILENCE = rotate(np.zeros((2, sa.NSAMPLES), np.float32))    # y = +0 under the rotation: (+0, +0), (-0, +0), (-0, -0), (+0, -0)


def first_silent_output(nsamples):
    """The first m all of whose taps meet samples at or past nsamples (48000 if there is none): output m reads a[N - j] with tap
    h[r + 4 j], j = 0 .. 39, and h[159] = 0, so its earliest sample is N - 39, or N - 38 where r = 3.  That sample moves forward
    with every m (N by 3 or 4, the span by at most 1), so the silent outputs are a tail of the frame."""
    T = 15 * _M + 79
    lo = T // 4 - np.where(T % 4 == 3, 38, 39)
    assert (np.diff(lo) > 0).all()
    return int(np.searchsorted(lo, nsamples))


# ---- impulse clips: one tap per output ---------------------------------------------------------------------------------------------
IMPULSE_STEP = 41                                           # longer than a window (40 samples), coprime to 4 and to 15


def impulse_clip(fmt, nsamples=N):
    """unit impulses (16384 in int16) every 41 samples from sample 0 on"""
    pcm = np.zeros(nsamples, np.int16 if fmt == sa.S16 else np.float32)
    pcm[::IMPULSE_STEP] = 16384 if fmt == sa.S16 else 1.0
    return pcm


def impulse_taps(nsamples=N):
    """per output m: (n0, k, hit): the one impulse its window can hold, the tap k = 15 m + 79 - 4 n0 that meets it, and whether
    it does (0 <= k < 159 and n0 inside the clip)"""
    T = 15 * _M + 79
    n0 = (T // 4) // IMPULSE_STEP * IMPULSE_STEP            # the last impulse at or before N; the one before it is 41 > 39 back
    k = T - 4 * n0
    return n0, k, (k < 159) & (n0 < nsamples)


def impulse_frame(pcm, fmt, base_bin):
    """the frame of an impulse clip in closed form, from the tables alone: where a tap meets an impulse the sum is +0 plus one
    product, F(h[k] * F(a * wm[(n0 f) mod 1920])); elsewhere it is +0.  float32 [2][48000]"""
    h, wm = sa.taps(), sa.mixer()
    a = sa.samples(pcm, fmt)
    n0, k, hit = impulse_taps(a.size)
    n0, k = np.where(hit, n0, 0), np.where(hit, k, 159)
    c = wm[(n0 * (base_bin + 128)) % 1920]
    y = np.zeros((2, sa.NSAMPLES), np.float32)
    for p in range(2):
        y[p] = np.where(hit, np.float32(0) + h[k] * (a[n0] * c[:, p]), np.float32(0))
    return rotate(y)


# ---- which mixer entries a band list reads ------------------------------------------------------------------------------------------
def entries_read(base_bins, nsamples=N):
    """the set of wm[] indices (n f) mod 1920, n < nsamples, over the bands of a list"""
    n = np.arange(nsamples, dtype=np.int64)
    return set(np.unique(np.concatenate([(n * (b + 128)) % 1920 for b in base_bins])).tolist())


OLD_BAND_LISTS = ((0,), (0, 240), (704,), (0, 240, 480, 704))
WIDE_BAND_LISTS = ((3,), (701, 1, 36, 127), (704, 0), (240, 240))

# ---- clip ends at the kernel's seams (bands SEAM_BANDS, two dense clips) ---------------------------------------------------------
SEAM_BANDS = (3, 704)
SEAM_LENGTHS = {"groups": (8, 9, 15, 16, 17, 39, 40, 41),                     # 16-byte groups and the 40-sample window
                "tile1": (2855, 2856, 2857, 2860, 2863, 2864),                # tile 1 stages from sample 2880 - 24
                "stage0": (3047, 3048, 3049),                                 # tile 0 stages 3072 samples from sample -24
                "workgroup": (8615, 8616, 8617),                              # three tiles per workgroup: 3 * 2880 - 24
                "last_tile": (178535, 178536, 178537),                        # 62 * 2880 - 24
                "last_group": (179993, 179994, 179995, 179996, 179997, 179998)}


def seam_clips(fmt, nsamples):
    """two clips of dense seeded noise: the second starts 16-byte aligned only if nsamples * sizeof(sample) is a multiple of 16"""
    x = np.random.default_rng(21).normal(0, 0.2, (2, nsamples))
    return to_s16(x) if fmt == sa.S16 else x.astype(np.float32)


# ---- a dozen signals for the merge: every one in reach of bands 96, 100 and 0 ------------------------------------------------------
DOZEN = (("CQ K1ABC FN42", 700.0, 0.5), ("CQ DL1XYZ JO62", 771.875, 0.0), ("CQ JA1AAA PM95", 843.75, 0.9), ("CQ VK2BBB QF56", 918.75, 0.2),
         ("CQ W9XYZ EN52", 990.625, 1.1), ("CQ G4ABC IO91", 1062.5, 0.4), ("CQ F5DEF JN18", 1137.5, 0.7), ("CQ EA3GHI JN11", 1209.375, 0.1),
         ("CQ I2JKL JN45", 1281.25, 1.0), ("CQ OH6MNO KP20", 1356.25, 0.3), ("CQ SM5PQR JO89", 1428.125, 0.8), ("CQ PY2STU GG66", 1500.0, 0.6))
DOZEN_BANDS = (96, 100, 0, 100)                             # overlapping, not ascending, one base twice
DOZEN_SEED = 7


def dozen_signal_clip(oracle, seed=DOZEN_SEED):
    """int16 [180000]: the twelve signals of DOZEN in the noise of five_signal_clip"""
    x = noise(seed)
    for text, f0, t0 in DOZEN:
        rc, payload = oracle.pack77(text)
        assert rc == 0
        x = x + cpfsk(oracle.encode(payload[:10]), f0, t0)
    return to_s16(x)


def dozen_hz(text):
    return {t: f for t, f, _ in DOZEN}[text]
