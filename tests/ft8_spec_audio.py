"""The audio front end of include/ft8gpu.h ("12 kHz audio"), restated in numpy: the tables, the frames of a clip's bands and the
merge of the bands' records.  float32 throughout, one IEEE operation per step, the sums sequential from +0 in the stated order;
the tables come from libm through python's math module, in double, as the C code forms them."""
import math

import numpy as np

RATE, NSAMPLES_AUDIO, TAPS, MIX, MAX_BANDS, MAX_BASE = 12000, 180000, 160, 1920, 4, 704
NSAMPLES = 48000
S16, F32 = 0, 1
F = np.float32


def mixer():
    """wm [1920][2] = (cos, -sin)(2 pi i / 1920)"""
    out = np.zeros((MIX, 2), F)
    for i in range(MIX):
        a = 2.0 * math.pi * float(i) / float(MIX)
        out[i] = (F(math.cos(a)), F(-math.sin(a)))
    return out


def _i0(x):
    s = term = 1.0
    for k in range(1, 40):
        q = x / (2.0 * float(k))
        term = term * (q * q)
        s = s + term
    return s


def taps():
    """h [160]: the Kaiser low-pass, h[159] = 0"""
    out = np.zeros(TAPS, F)
    i0_8 = _i0(8.0)
    for k in range(TAPS - 1):
        d = float(k - 79)
        pu = math.pi * ((3200.0 * d) / 48000.0)
        sinc = 1.0 if k == 79 else math.sin(pu) / pu
        w = d / 80.0
        x = 8.0 * math.sqrt(1.0 - w * w)
        out[k] = F((((8.0 * (3200.0 / 48000.0)) * sinc) * _i0(x)) / i0_8)
    return out


_H, _WM = taps(), mixer()
_M = np.arange(NSAMPLES, dtype=np.int64)
_T = 15 * _M + 79
_R, _N = _T % 4, _T // 4
_PAD = 64                                        # zeros in front of z: N - j >= 19 - 39


def samples(pcm, fmt):
    """a[n] of one clip as float32"""
    if fmt == S16:
        return np.asarray(pcm, np.int16).astype(F) * F(2.0 ** -15)
    assert fmt == F32
    return np.asarray(pcm, F)


def frame(a, base_bin):
    """one band of one clip: a float32 [nsamples] -> x float32 [2][48000]"""
    a = np.asarray(a, F)
    n = a.shape[0]
    assert 1 <= n <= NSAMPLES_AUDIO and 0 <= base_bin <= MAX_BASE
    idx = (np.arange(n, dtype=np.int64) * (base_bin + 128)) % MIX
    z = np.zeros((2, _PAD + NSAMPLES_AUDIO + 64), F)
    with np.errstate(all="ignore"):
        z[0, _PAD:_PAD + n] = a * _WM[idx, 0]
        z[1, _PAD:_PAD + n] = a * _WM[idx, 1]
        y = np.zeros((2, NSAMPLES), F)
        for j in range(40):
            h = _H[_R + 4 * j]
            y[0] = y[0] + h * z[0, _PAD + _N - j]
            y[1] = y[1] + h * z[1, _PAD + _N - j]
    x = np.empty((2, NSAMPLES), F)
    yr, yi = y
    x[0, 0::4], x[1, 0::4] = yr[0::4], yi[0::4]
    x[0, 1::4], x[1, 1::4] = -yi[1::4], yr[1::4]
    x[0, 2::4], x[1, 2::4] = -yr[2::4], -yi[2::4]
    x[0, 3::4], x[1, 3::4] = yi[3::4], -yr[3::4]
    return x


def frames(pcm, fmt, base_bins):
    """pcm [nclips][nsamples] -> [nclips][nbands][2][48000]"""
    pcm = np.asarray(pcm)
    out = np.zeros((pcm.shape[0], len(base_bins), 2, NSAMPLES), F)
    for c in range(pcm.shape[0]):
        a = samples(pcm[c], fmt)
        for b, base in enumerate(base_bins):
            out[c, b] = frame(a, int(base))
    return out


def merge(band_msgs, band_n, base_bins, msgs, n_msgs):
    """band_msgs [nclips][nbands][50] records, band_n [nclips][nbands] -> msgs [nclips][50 * nbands] (written in place below the
    count only), n_msgs [nclips]"""
    nclips, nbands = band_n.shape
    for c in range(nclips):
        kept, seen = 0, []
        for b in range(nbands):
            for k in range(min(max(int(band_n[c, b]), 0), 50)):
                if kept >= 50 * nbands:
                    break
                rec = band_msgs[c, b, k].copy()
                key = rec["a91"].tobytes()
                if key in seen:
                    continue
                seen.append(key)
                cand = rec["cand"]
                rec["freq_hz"] = (F(int(cand["freq_offset"]) + int(base_bins[b])) + F(cand["freq_sub"]) / F(2)) * F(6.25)
                rec["pad"][0] = b
                msgs[c, kept] = rec
                kept += 1
        n_msgs[c] = kept
    return msgs, n_msgs


def same(got, want):
    """byte for byte, except that a NaN of `want` asks for a NaN only (include/ft8gpu.h: sign and payload unspecified).  Returns
    (number of NaNs compared as NaN, None or a description of the first difference)."""
    g = np.ascontiguousarray(got, F)
    w = np.ascontiguousarray(want, F)
    if g.shape != w.shape:
        return 0, f"shapes {g.shape} != {w.shape}"
    wn = np.isnan(w)
    bad = np.where(wn, ~np.isnan(g), g.view(np.uint32) != w.view(np.uint32))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        return int(wn.sum()), f"{int(bad.sum())} values differ, the first at {list(map(int, at))}: {g[at]!r} != {w[at]!r}"
    return int(wn.sum()), None
