"""The wideband RX front end of include/ft8gpu.h ("wideband RX"), restated in numpy: the tables, the integer stage A in its
direct 497-tap form and in its fast form (four int64 cumulative sums, decimated, fourth differences), the float32 stage B (one
IEEE operation per step, sums sequential from +0, taps ascending), the frames of a capture's channels and the merge of the
channels' records.  The tables come from libm through python's math module, in double, as the C code forms them."""
import math

import numpy as np

RATE, MAX_PAIRS, MIX1, MIX2, TAPS, MAX_CHANNELS, MAX_BIN = 2400000, 36000000, 6000, 3072, 96, 16, 176000
NSAMPLES = 48000
R1, R2 = 125, 6                                  # 2.4 Msps -> 19 200 sps -> 3200 sps
NTAPS = 95                                       # h[0 .. 94], centred on 47; h[95] = 0
KAISER, BETA, DROOP = 93, 9.0, 0.1685
F = np.float32


def mixer1():
    """w1 [6000][2] int16 = (lrint(32767 cos), -lrint(32767 sin))(2 pi i / 6000)"""
    out = np.zeros((MIX1, 2), np.int16)
    for i in range(MIX1):
        a = 2.0 * math.pi * float(i) / float(MIX1)
        out[i] = (round(32767.0 * math.cos(a)), -round(32767.0 * math.sin(a)))      # round half even = lrint
    return out


def mixer2():
    """w2 [3072][2] = (cos, -sin)(2 pi i / 3072)"""
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


def _kaiser_sinc(k):
    """t[k], k = 0 .. 92, and 0 outside"""
    if k < 0 or k >= KAISER:
        return 0.0
    d = float(k - (KAISER - 1) // 2)
    pu = math.pi * ((3200.0 * d) / 19200.0)
    sinc = 1.0 if d == 0.0 else math.sin(pu) / pu
    w = d / float((KAISER - 1) // 2)
    x = BETA * math.sqrt(1.0 - w * w)
    return (sinc * _i0(x)) / _i0(BETA)


def taps():
    """h [96]: the Kaiser low-pass convolved with the droop compensator [-a, 1 + 2a, -a], normalised to sum 1; h[95] = 0"""
    hh = [((1.0 + 2.0 * DROOP) * _kaiser_sinc(i - 1) - DROOP * _kaiser_sinc(i)) - DROOP * _kaiser_sinc(i - 2) for i in range(NTAPS)]
    s = 0.0
    for v in hh:
        s = s + v
    out = np.zeros(TAPS, F)
    for i in range(NTAPS):
        out[i] = F(hh[i] / s)
    return out


def cic_taps():
    """g [497] int64: the four-fold convolution of a 125-sample boxcar"""
    box = np.ones(R1, np.int64)
    g = box
    for _ in range(3):
        g = np.convolve(g, box)
    return g


C0 = F(1.0 / (32767.0 * float(R1) ** 4 * 128.0))
_W1, _W2, _H = mixer1().astype(np.int32), mixer2(), taps()


def channel(freq_bin):
    """(c, q): the two mixer steps of a channel"""
    f = int(freq_bin) + 128
    c = (f + 32) // 64
    return c, f - 64 * c


def last_m(npairs):
    """the last m whose window holds a sample: 125 m - 248 <= npairs - 1"""
    return (npairs - 1 + 248) // R1


def mixed(raw, c):
    """u[n] = x[n] * w1[(n c) mod 6000], 0 <= n < npairs -> (re, im) int32"""
    x = (np.asarray(raw, np.uint8) ^ np.uint8(0x80)).view(np.int8).astype(np.int32)
    xr, xi = x[0::2], x[1::2]
    idx = (np.arange(xr.shape[0], dtype=np.int64) * c) % MIX1
    wr, wi = _W1[idx, 0], _W1[idx, 1]
    return xr * wr - xi * wi, xr * wi + xi * wr


def stage_a_direct(raw, c, ms):
    """v[m] for the given m by the 497-tap definition, int64 -> (re, im)"""
    ur, ui = mixed(raw, c)
    n = ur.shape[0]
    g = cic_taps()
    out = np.zeros((2, len(ms)), np.int64)
    j = np.arange(497)
    for o, m in enumerate(ms):
        at = R1 * int(m) + 248 - j
        ok = (at >= 0) & (at < n)
        out[0, o] = (g[ok] * ur[at[ok]].astype(np.int64)).sum()
        out[1, o] = (g[ok] * ui[at[ok]].astype(np.int64)).sum()
    return out


def stage_a(raw, c):
    """v[m], m = -1 .. last_m, in the fast form: four int64 cumulative sums of u (they wrap, the result does not), every 125th
    value from sample 123 on, then four first differences -> int64 [2][last_m + 2], column m + 1"""
    npairs = len(raw) // 2
    ml = last_m(npairs)
    out = np.zeros((2, ml + 2), np.int64)
    for part, u in enumerate(mixed(raw, c)):
        s = np.zeros(R1 * (ml + 2), np.int64)
        s[:npairs] = u
        for _ in range(4):
            np.cumsum(s, out=s)
        d = np.zeros(ml + 2 + 4, np.int64)                   # D[k] = S4[125 k + 123], k = -4 .. last_m + 1
        d[4:] = s[123::R1]
        for _ in range(4):
            d = d[1:] - d[:-1]
        out[part] = d
    return out


def stage_b(v, q):
    """v int64 [2][M] (column m + 1) -> the frame float32 [2][48000]"""
    m = np.arange(-1, v.shape[1] - 1, dtype=np.int64)
    idx = (m * q) % MIX2
    wr, wi = _W2[idx, 0], _W2[idx, 1]
    with np.errstate(all="ignore"):
        vr, vi = v[0].astype(F) * C0, v[1].astype(F) * C0
        pad = 48                                             # z[m] lies at pad + m: the windows reach from -47 to 288041
        z = np.zeros((2, pad + R2 * NSAMPLES + 64), F)
        n = min(v.shape[1], z.shape[1] - pad + 1)
        z[0, pad - 1:pad - 1 + n] = (vr * wr - vi * wi)[:n]
        z[1, pad - 1:pad - 1 + n] = (vr * wi + vi * wr)[:n]
        at = pad + R2 * np.arange(NSAMPLES, dtype=np.int64) + 47
        y = np.zeros((2, NSAMPLES), F)
        for k in range(NTAPS):
            y[0] = y[0] + _H[k] * z[0, at - k]
            y[1] = y[1] + _H[k] * z[1, at - k]
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
    pk = F(np.abs(x).max())
    max_sig = pk if pk > F(1e-24) else F(1e-24)
    return x * F(0.5 / float(max_sig))


def frame(raw, freq_bin, normalise=False):
    """one channel of one capture: raw uint8 [2 npairs] -> float32 [2][48000]"""
    raw = np.asarray(raw, np.uint8)
    npairs = raw.shape[0] // 2
    assert raw.shape[0] == 2 * npairs and npairs >= 8 and npairs % 8 == 0 and npairs <= MAX_PAIRS and abs(int(freq_bin)) <= MAX_BIN
    c, q = channel(freq_bin)
    x = stage_b(stage_a(raw, c), q)
    return normalised(x) if normalise else x


def frames(raw, freq_bins, normalise=False):
    """raw [ncaptures][2 npairs] -> [ncaptures][nchannels][2][48000]"""
    raw = np.asarray(raw, np.uint8)
    out = np.zeros((raw.shape[0], len(freq_bins), 2, NSAMPLES), F)
    for k in range(raw.shape[0]):
        for b, fb in enumerate(freq_bins):
            out[k, b] = frame(raw[k], int(fb), normalise)
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
