"""The fading channel of include/ft8gpu.h ("Fading channel"), restated in numpy on top of tests/ft8_spec_gfsk.py: the taps, the path
amplitudes and the delay, a path's grid values, the per-sample gain, a path's contribution and a clip's sum.  Phases are wrapping
uint32 arithmetic, everything else float32, one IEEE operation per step, the sums sequential from +0.  gain64() is the same process
in float64 without tables or interpolation: the model the statistics tests look at."""
import math

import numpy as np

import ft8_spec_gfsk as sg

F = np.float32
NONE, FADED = 0, 1
TAPS, GRID = 16, 1265
STEP = {sg.IQ: 32, sg.AUDIO: 120}
# the standard normal quantiles at (m + 0.5) / 16, as include/ft8gpu.h commits them (FT8GPU_CHANNEL_QUANTILES)
QUANTILES = [-1.862731867421651, -1.318010897303537, -1.009990169249582, -0.776421761147928, -0.579132162255556, -0.402250065321725,
             -0.237202109328788, -0.078412412733112, 0.078412412733112, 0.237202109328788, 0.402250065321725, 0.579132162255556,
             0.776421761147928, 1.009990169249582, 1.318010897303537, 1.862731867421651]
PRESETS = {"quiet": (0.1, 0.5, 1.0, FADED), "moderate": (0.5, 1.0, 1.0, FADED), "disturbed": (1.0, 2.0, 1.0, FADED),
           "flutter": (10.0, 0.5, 1.0, FADED)}
CHANNEL_DTYPE = np.dtype([("spread_hz", "<f4"), ("delay_ms", "<f4"), ("path2_gain", "<f4"), ("mode", "<u4")])
_M64 = (1 << 64) - 1
_M32 = 0xFFFFFFFF


def mix(x):
    """splitmix64's step on a python int"""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def taps(seed, clip, signal, path, spread_hz):
    """(gstep, theta), uint32 [16] each"""
    key = mix((seed & _M64) ^ 0x4641444531)
    gstep, theta = np.zeros(TAPS, np.uint32), np.zeros(TAPS, np.uint32)
    for m in range(TAPS):
        f = (float(F(spread_hz)) / 2.0) * QUANTILES[m]
        gstep[m] = int(np.rint(f / 100.0 * 4294967296.0)) & _M32          # llrint of a double: half to even; negative wraps
        theta[m] = mix(key ^ mix(((clip << 12) + (signal << 5) + (path << 4) + m) & _M64)) >> 32
    return gstep, theta


def path_amplitudes(path2_gain):
    """(w_0, w_1): r = sqrtf(1 + g2 * g2); 1 / r, g2 / r"""
    g2 = F(path2_gain)
    r = np.sqrt(F(1.0) + g2 * g2, dtype=F)
    return F(1.0) / r, g2 / r


def delay_of(delay_ms, mode):
    """lrintf(delay_ms * (float)rate / 1000.0f), left to right"""
    return int(np.rint(F(delay_ms) * F(sg.RATE[mode]) / F(1000.0)))


def grid(gstep, theta, w):
    """G[0 .. 1264]: float32 [1265][2]"""
    _, _, gc, gf = sg.tables(sg.IQ)
    j = np.arange(GRID, dtype=np.uint64)
    sc, ss = np.zeros(GRID, F), np.zeros(GRID, F)
    for m in range(TAPS):
        ph = ((np.uint64(theta[m]) + np.uint64(gstep[m]) * j) & np.uint64(_M32)).astype(np.uint32)
        c, f = gc[ph >> 20], gf[(ph >> 8) & 4095]
        sc = sc + (c[:, 0] * f[:, 0] - c[:, 1] * f[:, 1])
        ss = ss + (c[:, 1] * f[:, 0] + c[:, 0] * f[:, 1])
    return np.stack([F(w) * (F(0.25) * sc), F(w) * (F(0.25) * ss)], axis=1).astype(F)


def gain(G, mode):
    """the interpolated gain at the local samples n' in [0, 79 sps): float32 [2][79 sps]"""
    S = STEP[mode]
    n = np.arange(sg.NN * sg.SPS[mode])
    j, k = n // S, n % S
    t = k.astype(F) / F(S)
    return np.stack([G[j, p] + (G[j + 1, p] - G[j, p]) * t for p in range(2)]).astype(F)


def path_contribution(x, G, mode):
    """x: the unfaded contribution [2][79 sps] -> (xr Gr - xi Gi, xr Gi + xi Gr)"""
    g = gain(G, mode)
    with np.errstate(all="ignore"):
        return np.stack([x[0] * g[0] - x[1] * g[1], x[0] * g[1] + x[1] * g[0]]).astype(F)


def _add(out, x, start):
    n = out.shape[1]
    lo, hi = max(start, 0), min(start + x.shape[1], n)
    if lo < hi:
        with np.errstate(all="ignore"):
            out[:, lo:hi] = out[:, lo:hi] + x[:, lo - start:hi - start]


def clip(signals, channels, mode, nsamples=None, seed=0, clip_index=0):
    """the sum before noise and normalisation.  signals = [(tones, f0_hz, t0_s, amplitude), ...], channels = None or
    [(spread_hz, delay_ms, path2_gain, mode), ...] -> float32 [2][48000] (IQ) or [nsamples] (AUDIO)"""
    n = sg.NSAMPLES_IQ if mode == sg.IQ else int(nsamples)
    out = np.zeros((2, n), F)
    for s, (tones, f0_hz, t0_s, amplitude) in enumerate(signals):
        x = sg.contribution(tones, f0_hz, amplitude, mode)
        start = sg.start_of(t0_s, mode)
        ch = None if channels is None else channels[s]
        if ch is None or int(ch[3]) == NONE:
            _add(out, x, start)
            continue
        w = path_amplitudes(ch[2])
        d = delay_of(ch[1], mode)
        for p in range(1 if F(ch[2]) == 0 else 2):
            gstep, theta = taps(seed, clip_index, s, p, ch[0])
            _add(out, path_contribution(x, grid(gstep, theta, w[p]), mode), start + (d if p else 0))
    return out if mode == sg.IQ else out[0]


def channel_records(clips):
    """a list (clips) of lists of (spread_hz, delay_ms, path2_gain, mode) -> CHANNEL_DTYPE [nclips][nsig]"""
    out = np.zeros((len(clips), len(clips[0])), CHANNEL_DTYPE)
    for c, chs in enumerate(clips):
        for s, ch in enumerate(chs):
            out[c, s] = tuple(ch)
    return out


# ---- the model in double ---------------------------------------------------------------------------------------------------------------
def gain64(seed, clip, signal, path, spread_hz, t):
    """the gain process at the times t (seconds) in float64: 0.25 sum exp(2 pi i (theta_m / 2^32 + f_m t)), f_m as quantised"""
    gstep, theta = taps(seed, clip, signal, path, spread_hz)
    f = ((gstep.astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)) * (100.0 / 4294967296.0)
    ph = theta.astype(np.float64)[:, None] / 4294967296.0 + f[:, None] * np.asarray(t, np.float64)[None, :]
    return 0.25 * np.exp(2j * math.pi * ph).sum(axis=0)
