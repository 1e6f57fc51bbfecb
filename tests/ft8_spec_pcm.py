"""The PCM front end of include/ft8gpu.h ("PCM front end"), restated in numpy: the tables, the two float32 stages (one IEEE
operation per step, sums sequential from +0, taps ascending), the frames of a capture's channels and the merge of the channels'
records.  The tables come from libm through python's math module, in double, as the C code forms them.  Outputs whose windows
hold no sample are +0 by the rule, so a short capture costs little here."""
import math

import numpy as np

S16, F32FMT, COMPLEX = 0, 1, 2                   # FT8GPU_PCM_S16 / _F32 / _COMPLEX
DS = (15, 30, 60, 120, 240)
MIX2, TAPS_B, NTAPS_B, MAX_CHANNELS = 1536, 48, 47, 16
NSAMPLES, NPLANE = 48000, 144000                 # outputs of stage B and of stage A
BETA = 9.0
F = np.float32


def rate_of(D):
    return 3200 * D


def max_samples(D):
    return 48000 * D


def mixer1(D):
    """w1 [16 D][2] = (cos, -sin)(2 pi i / (16 D))"""
    n = 16 * D
    out = np.zeros((n, 2), F)
    for i in range(n):
        a = 2.0 * math.pi * float(i) / float(n)
        out[i] = (F(math.cos(a)), F(-math.sin(a)))
    return out


def mixer2():
    """w2 [1536][2] = (cos, -sin)(2 pi i / 1536)"""
    out = np.zeros((MIX2, 2), F)
    for i in range(MIX2):
        a = 2.0 * math.pi * float(i) / float(MIX2)
        out[i] = (F(math.cos(a)), F(-math.sin(a)))
    return out


def _i0(x):
    s = term = 1.0
    for k in range(1, 40):
        q = x / (2.0 * float(k))
        term = term * (q * q)
        s = s + term
    return s


def kaiser_lowpass_double(half, cutoff, rate):
    """t[k] / s in double, k = 0 .. 2 half: the taps before their rounding to float"""
    t = []
    for k in range(2 * half + 1):
        d = float(k - half)
        pu = math.pi * (((2.0 * cutoff) * d) / rate)
        sinc = 1.0 if d == 0.0 else math.sin(pu) / pu
        w = d / float(half)
        x = BETA * math.sqrt(1.0 - w * w)
        t.append((sinc * _i0(x)) / _i0(BETA))
    s = 0.0
    for v in t:
        s = s + v
    return [v / s for v in t]


def taps_a(D):
    """hA [8 M + 1], M = D / 3: Kaiser (beta 9) low-pass at 3200 D sps, cutoff 4000 Hz, centred on 4 M, sum 1"""
    return np.array(kaiser_lowpass_double(4 * (D // 3), 4000.0, 3200.0 * float(D)), np.float64).astype(F)


def taps_b():
    """hB [48]: Kaiser (beta 9) low-pass at 9600 sps, cutoff 1600 Hz, 47 taps centred on 23, sum 1; hB[47] = 0"""
    out = np.zeros(TAPS_B, F)
    out[:NTAPS_B] = np.array(kaiser_lowpass_double(23, 1600.0, 9600.0), np.float64).astype(F)
    return out


_TABLES = {}


def tables(D):
    """(w1, hA) of D, computed once"""
    if D not in _TABLES:
        _TABLES[D] = (mixer1(D), taps_a(D))
    return _TABLES[D]


_W2, _HB = mixer2(), taps_b()


def channel(freq_bin):
    """(c, q): the two mixer steps of a channel"""
    f = int(freq_bin) + 128
    c = (f + 16) // 32
    return c, f - 32 * c


def bin_range(D, fmt):
    return (-256 * D if fmt & COMPLEX else 0), 256 * D - 256


def last_m(D, nsamples):
    """the last m whose window holds a sample, M m - 4 M <= nsamples - 1, at most 143999"""
    M = D // 3
    return min((nsamples - 1 + 4 * M) // M, NPLANE - 1)


def samples(pcm, fmt):
    """one capture's elements -> (xr, xi) float32; xi is None for real input"""
    a = np.asarray(pcm)
    if fmt & F32FMT:
        assert a.dtype == F
    else:
        assert a.dtype == np.int16
        a = a.astype(F) * F(2.0 ** -15)
    if fmt & COMPLEX:
        return a[0::2], a[1::2]
    return a, None


def stage_a(xr, xi, D, c):
    """v[m], m = 0 .. last_m -> float32 [2][last_m + 1]"""
    M = D // 3
    w1, h = tables(D)
    n = xr.shape[0]
    ml = last_m(D, n)
    idx = (np.arange(n, dtype=np.int64) * c) % (16 * D)
    wr, wi = w1[idx, 0], w1[idx, 1]
    with np.errstate(all="ignore"):
        if xi is None:
            ur, ui = xr * wr, xr * wi
        else:
            ur, ui = xr * wr - xi * wi, xr * wi + xi * wr
        u = np.zeros((2, M * ml + 8 * M + 1), F)             # sample s lies at s + 4 M
        k = min(n, u.shape[1] - 4 * M)
        u[0, 4 * M:4 * M + k], u[1, 4 * M:4 * M + k] = ur[:k], ui[:k]
        at = M * np.arange(ml + 1, dtype=np.int64) + 8 * M
        v = np.zeros((2, ml + 1), F)
        for k in range(8 * M + 1):
            v[0] = v[0] + h[k] * u[0, at - k]
            v[1] = v[1] + h[k] * u[1, at - k]
    return v


def stage_b(v, q):
    """v float32 [2][last_m + 1] -> the frame float32 [2][48000]"""
    m = np.arange(v.shape[1], dtype=np.int64)
    idx = (m * q) % MIX2
    wr, wi = _W2[idx, 0], _W2[idx, 1]
    with np.errstate(all="ignore"):
        z = np.zeros((2, 3 * NSAMPLES + 64), F)              # z[m] lies at m + 23: the windows reach from -23 to 144020
        z[0, 23:23 + v.shape[1]] = v[0] * wr - v[1] * wi
        z[1, 23:23 + v.shape[1]] = v[0] * wi + v[1] * wr
        live = min(NSAMPLES, (v.shape[1] - 1 + 23) // 3 + 1)  # behind it the windows hold no sample: +0
        at = 3 * np.arange(live, dtype=np.int64) + 46
        y = np.zeros((2, NSAMPLES), F)
        for k in range(NTAPS_B):
            y[0, :live] = y[0, :live] + _HB[k] * z[0, at - k]
            y[1, :live] = y[1, :live] + _HB[k] * z[1, at - k]
        zero = F(0)
        x = np.empty((2, NSAMPLES), F)
        yr, yi = y
        x[0, 0::4], x[1, 0::4] = yr[0::4], yi[0::4]
        x[0, 1::4], x[1, 1::4] = zero - yi[1::4], yr[1::4]
        x[0, 2::4], x[1, 2::4] = zero - yr[2::4], zero - yi[2::4]
        x[0, 3::4], x[1, 3::4] = yi[3::4], zero - yr[3::4]
    return x


def normalised(x):
    """the peak normalisation of ft8gpu_rx_decimate on one frame"""
    with np.errstate(all="ignore"):
        pk = F(np.abs(x).max())
        max_sig = pk if pk > F(1e-24) else F(1e-24)
        return x * F(0.5 / float(max_sig))


def frame(pcm, fmt, D, freq_bin, normalise=False):
    """one channel of one capture -> float32 [2][48000]"""
    xr, xi = samples(pcm, fmt)
    lo, hi = bin_range(D, fmt)
    assert D in DS and 1 <= xr.shape[0] <= max_samples(D) and lo <= int(freq_bin) <= hi
    c, q = channel(freq_bin)
    x = stage_b(stage_a(xr, xi, D, c), q)
    return normalised(x) if normalise else x


def frames(pcm, fmt, D, freq_bins, normalise=False):
    """pcm [ncaptures][elements] -> [ncaptures][nchannels][2][48000]"""
    out = np.zeros((len(pcm), len(freq_bins), 2, NSAMPLES), F)
    for k in range(len(pcm)):
        for b, fb in enumerate(freq_bins):
            out[k, b] = frame(pcm[k], fmt, D, int(fb), normalise)
    return out


def merge(chan_msgs, chan_n, freq_bins, msgs, n_msgs):
    """chan_msgs [ncaptures][nchannels][50] records, chan_n [ncaptures][nchannels] -> msgs [ncaptures][50 * nchannels] (written in
    place below the count only), n_msgs [ncaptures]"""
    ncap, nch = chan_n.shape
    for c in range(ncap):
        kept, seen = 0, []
        for b in range(nch):
            for k in range(min(max(int(chan_n[c, b]), 0), 50)):
                if kept >= 50 * nch:
                    break
                rec = chan_msgs[c, b, k].copy()
                key = rec["a91"].tobytes()
                if any(key == s and abs(int(freq_bins[b]) - int(freq_bins[sb])) < 256 for s, sb in seen):
                    continue
                seen.append((key, b))
                cand = rec["cand"]
                rec["freq_hz"] = (F(int(cand["freq_offset"]) + int(freq_bins[b])) + F(cand["freq_sub"]) / F(2)) * F(6.25)
                rec["pad"][0] = b
                msgs[c, kept] = rec
                kept += 1
        n_msgs[c] = kept
    return msgs, n_msgs
