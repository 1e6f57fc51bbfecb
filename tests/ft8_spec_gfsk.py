"""The GFSK synthesiser of include/ft8gpu.h ("GFSK synthesis"), restated in numpy: the tables, one signal's contribution, a clip's
sum, peak normalisation and the int16 form.  The phase is wrapping uint32 arithmetic; everything else float32, one IEEE operation
per step, the sums sequential from +0 in signal order; the tables come from libm through python's math module, in double, as the
C code forms them.  Noise is not restated: it is outside the exact contract."""
import math

import numpy as np

IQ, AUDIO = 0, 1
S16, F32 = 0, 1
RATE = {IQ: 3200, AUDIO: 12000}
SPS = {IQ: 512, AUDIO: 1920}
NSAMPLES_IQ, NSAMPLES_AUDIO = 48000, 180000
NN, MAX_SIGNALS = 79, 64
F = np.float32
_MASK = 0xFFFFFFFF


def pulse_p(sps):
    """p_i, i = 0 .. 3 sps - 1, in double"""
    c = math.pi * math.sqrt(2.0 / math.log(2.0))
    out = np.zeros(3 * sps)
    for i in range(3 * sps):
        t = (float(i) - 1.5 * float(sps)) / float(sps)
        out[i] = 0.5 * (math.erf((2.0 * c) * (t + 0.5)) - math.erf((2.0 * c) * (t - 0.5)))
    return out


def pulse(sps, unreduced=False):
    """Q_sps[0 .. 3 sps] as uint32 (unreduced: python ints before the mod)"""
    p = pulse_p(sps)
    s, raw = 0.0, []
    for k in range(3 * sps + 1):
        raw.append(int(round((4294967296.0 * s) / float(sps))))   # round-half-even on a double: llrint in the default mode
        if k < 3 * sps:
            s = s + float(p[k])
    return raw if unreduced else np.array([r & _MASK for r in raw], np.uint32)


def twiddles():
    """(gc, gf), float32 [4096][2] each"""
    gc, gf = np.zeros((4096, 2), F), np.zeros((4096, 2), F)
    for i in range(4096):
        a = 2.0 * math.pi * float(i) / 4096.0
        gc[i] = (F(math.cos(a)), F(math.sin(a)))
        a = 2.0 * math.pi * float(i) / 16777216.0
        gf[i] = (F(math.cos(a)), F(math.sin(a)))
    return gc, gf


def ramp(sps):
    nr = sps // 8
    return np.array([F(0.5 * (1.0 - math.cos(math.pi * float(k) / float(nr)))) for k in range(nr)], F)


_TAB = {}


def tables(mode):
    if mode not in _TAB:
        if "tw" not in _TAB:
            _TAB["tw"] = twiddles()
        _TAB[mode] = (pulse(SPS[mode]).astype(np.uint64), ramp(SPS[mode]))
    return _TAB[mode] + _TAB["tw"]


def start_of(t0_s, mode):
    """lrintf(t0_s * (float)rate): the float product, rounded half to even"""
    return int(np.rint(F(t0_s) * F(RATE[mode])))


def step_of(f0_hz, mode):
    """(uint32_t)llrint((double)f0_hz * 4294967296.0 / (double)rate)"""
    return int(np.rint(float(F(f0_hz)) * 4294967296.0 / float(RATE[mode]))) & _MASK


def phase(tones, step, mode):
    """phi[n'] for n' in [0, 79 sps), uint32"""
    sps = SPS[mode]
    Q = tables(mode)[0]
    tones = np.asarray(tones, np.uint64)
    e = np.concatenate([tones[:1], tones, tones[-1:]])
    n = np.arange(NN * sps, dtype=np.uint64)
    m, k = (n // sps).astype(np.int64), (n % sps).astype(np.int64)
    phi = np.uint64(step) * n + e[m] * Q[k + 2 * sps] + e[m + 1] * Q[k + sps] + e[m + 2] * Q[k]
    return (phi & np.uint64(_MASK)).astype(np.uint32)


def envelope(mode):
    sps = SPS[mode]
    r = tables(mode)[1]
    env = np.ones(NN * sps, F)
    env[:r.size] = r
    env[NN * sps - r.size:] = r[::-1]
    return env


def contribution(tones, f0_hz, amplitude, mode):
    """one signal's (a * co, a * si) for n' in [0, 79 sps): float32 [2][79 sps]"""
    _, _, gc, gf = tables(mode)
    phi = phase(tones, step_of(f0_hz, mode), mode)
    c, f = gc[phi >> 20], gf[(phi >> 8) & 4095]
    with np.errstate(all="ignore"):
        co = c[:, 0] * f[:, 0] - c[:, 1] * f[:, 1]
        si = c[:, 1] * f[:, 0] + c[:, 0] * f[:, 1]
        a = F(amplitude) * envelope(mode)
        return np.stack([a * co, a * si]).astype(F)


def clip(signals, mode, nsamples=None):
    """the sum before noise and normalisation: signals = [(tones, f0_hz, t0_s, amplitude), ...] in order -> float32 [2][48000]
    (IQ) or [nsamples] (AUDIO)"""
    n = NSAMPLES_IQ if mode == IQ else int(nsamples)
    out = np.zeros((2, n), F)
    for tones, f0_hz, t0_s, amplitude in signals:
        x = contribution(tones, f0_hz, amplitude, mode)
        start = start_of(t0_s, mode)
        lo, hi = max(start, 0), min(start + x.shape[1], n)
        if lo < hi:
            with np.errstate(all="ignore"):
                out[:, lo:hi] = out[:, lo:hi] + x[:, lo - start:hi - start]
    return out if mode == IQ else out[0]


def normalise(x, peak):
    """m = max |x| (a NaN skipped), m = max(m, 1e-24f), x * (peak / m)"""
    x = np.asarray(x, F)
    if not peak > 0:
        return x
    with np.errstate(all="ignore"):
        m = np.fmax(np.fmax.reduce(np.abs(x).reshape(-1), initial=F(0)), F(1e-24))
        return (x * (F(peak) / F(m))).astype(F)


def to_s16(x):
    """rintf(x * 32768.0f) clamped to [-32768, 32767]; a NaN gives 0"""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(x, F) * F(32768.0))
    r = np.where(np.isnan(r), F(0), np.clip(r, F(-32768.0), F(32767.0)))
    return r.astype(np.int16)


def synth(signals, mode, nsamples=None, peak=0.0, fmt=F32):
    x = normalise(clip(signals, mode, nsamples), peak)
    return to_s16(x) if fmt == S16 else x


# ---- the definition in double, with none of the table arithmetic ---------------------------------------------------------------------
def definition(tones, f0_hz, mode):
    """exp(2 pi j theta) of the float64 model: theta = running sum of f0q / rate + (sum over symbols j of e_j p(n' - j sps)) / sps,
    f0q = step * rate / 2^32 the frequency as quantised.  complex128 [79 sps]; its phase is defined up to a constant."""
    sps, rate = SPS[mode], RATE[mode]
    p = pulse_p(sps)
    tones = np.asarray(tones, np.float64)
    e = np.concatenate([tones[:1], tones, tones[-1:]])                     # symbols -1 .. 79
    dphi = np.zeros((NN + 5) * sps)                                        # index i is local sample i - 2 sps
    for j in range(NN + 2):                                                # symbol j - 1 starts at (j - 1) sps, its pulse a symbol earlier
        dphi[j * sps:(j + 3) * sps] += e[j] * p
    dphi /= sps
    before = np.cumsum(dphi) - dphi                                        # the turns before a sample
    step = step_of(f0_hz, mode)
    step = step - (1 << 32) if f0_hz < 0 else step
    f0q = step * float(rate) / 4294967296.0
    theta = before[2 * sps:(NN + 2) * sps] + (f0q / rate) * np.arange(NN * sps, dtype=np.float64)
    return np.exp(2j * np.pi * (theta - np.floor(theta)))
