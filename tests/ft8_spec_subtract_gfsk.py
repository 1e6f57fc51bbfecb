"""CPU restatement of the subtraction in the I/Q samples with a shaped reference (ft8gpu_subtract_messages_shaped,
ft8gpu_decode_messages_subtracted_shaped; include/ft8gpu.h "GFSK reference") in numpy.  Shape 0 is tests/ft8_spec_subtract.py,
called as it is.  Shape 1 differs from it in two places and in nothing else, so it runs that module's own functions with those two
places exchanged for the length of a call and put back behind it (the module's globals are left as they were found; other tests
import it in the same process):

  (b') theta(j) = ((phi + 2^19) >> 20) & 4095,  phi = (k4 << 20) n' + e[m] Q[k + 1024] + e[m + 1] Q[k + 512] + e[m + 2] Q[k]
       in wrapping uint32, n' = j - S = 512 m + k, e = (tone[0], tone[0 .. 78], tone[78]), Q = ft8gpu_gfsk_pulse(512, .)
  (e') the amplitude is (Ar env, Ai env) where env(n') != 1: the ramp of ft8gpu_gfsk_ramp(512, .) over the first 64 samples of a
       record and, mirrored, over its last 64; the estimate does not see the ramp

Q and the ramp come from the library's host helpers, as w4 does."""
import contextlib

import numpy as np

import ft8_spec_subtract as ss

CPFSK, GFSK = 0, 1
SPS, NRAMP = 512, 64
SPAN = ss.SPAN
F32 = np.float32
_MASK = np.uint64(0xFFFFFFFF)
_TABLES = []


def tables():
    """(Q uint32 [1537], ramp float32 [64]) from the library's host helpers"""
    if not _TABLES:
        import rtlsdr_ft8d_amd as ft8
        q, r = ft8.gfsk_pulse(SPS), ft8.gfsk_ramp(SPS)
        assert q.dtype == np.uint32 and q.shape == (3 * SPS + 1,) and r.dtype == F32 and r.shape == (NRAMP,)
        q.setflags(write=False)
        r.setflags(write=False)
        _TABLES.append((q, r))
    return _TABLES[0]


def check_shape(shape):
    if shape not in (CPFSK, GFSK):
        raise ValueError(f"shape {shape!r} is neither CPFSK (0) nor GFSK (1)")


def extended(tones):
    """e[0 .. 80]"""
    t = np.asarray(tones, np.uint64)
    assert t.shape == (79,)
    return np.concatenate([t[:1], t, t[-1:]])


def phi(k4, tones, Q):
    """phi[n'] for n' in [0, 40448): uint32, every product and sum reduced modulo 2^32 (none reaches 2^64 before that)"""
    Q = np.asarray(Q, np.uint64)
    e = extended(tones)
    n = np.arange(SPAN, dtype=np.uint64)
    m, k = (n // SPS).astype(np.int64), (n % SPS).astype(np.int64)
    step = np.uint64((int(k4) << 20) & 0xFFFFFFFF)
    return ((step * n + e[m] * Q[k + 2 * SPS] + e[m + 1] * Q[k + SPS] + e[m + 2] * Q[k]) & _MASK).astype(np.uint32)


def theta(S, k4, tones, Q=None):
    """ft8_spec_subtract.theta's result under (b'): (j, theta(j)) as int64 [79][512]"""
    Q = tables()[0] if Q is None else Q
    th = (((phi(k4, tones, Q).astype(np.uint64) + np.uint64(1 << 19)) & _MASK) >> np.uint64(20)) & np.uint64(4095)
    j = int(S) + np.arange(SPAN, dtype=np.int64)
    return j.reshape(79, SPS), th.astype(np.int64).reshape(79, SPS)


def envelope(ramp=None):
    """env(n') for n' in [0, 40448): float32"""
    r = tables()[1] if ramp is None else np.asarray(ramp, F32)
    env = np.ones(SPAN, F32)
    env[:NRAMP] = r
    env[SPAN - NRAMP:] = r[::-1]                        # env(n') = r[40447 - n']
    return env


def apply_gfsk(xr, xi, info, tones, A, w4, Q=None, ramp=None):
    """(e) with (e'): x' = x' - (A env) conj(w4[theta]) over the record's samples inside the frame, in place; where env is 1 the
    amplitude is A itself"""
    j, th = theta(int(info["s_best"]), int(info["k4"]), tones, Q)
    j, th = j.reshape(-1), th.reshape(-1)
    q = np.arange(SPAN) >> 5
    env = envelope(ramp)
    ok = (j >= 0) & (j < ss.NSAMPLES)
    j, th, q, env = j[ok], th[ok], q[ok], env[ok]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        ar, ai = A[0][q], A[1][q]
        ramped = env != F32(1)
        ar = np.where(ramped, ar * env, ar).astype(F32)
        ai = np.where(ramped, ai * env, ai).astype(F32)
        wr, wi = w4[th, 0], w4[th, 1]
        xr[j] = xr[j] - (ar * wr + ai * wi)
        xi[j] = xi[j] - (ai * wr - ar * wi)
    assert xr.dtype == F32 and ar.dtype == F32


@contextlib.contextmanager
def rule(shape, Q=None, ramp=None):
    """inside: ft8_spec_subtract's functions follow `shape`; behind it the module is as it was"""
    check_shape(shape)
    saved = (ss.theta, ss.apply_record)
    if shape == GFSK:
        ss.theta = lambda S, k4, tones: theta(S, k4, tones, Q)
        ss.apply_record = lambda xr, xi, info, tones, A, w4: apply_gfsk(xr, xi, info, tones, A, w4, Q, ramp)
    try:
        yield
    finally:
        ss.theta, ss.apply_record = saved


def estimate_record(I, Q_samples, cand, a91, R, w4, shape):
    """ft8_spec_subtract.estimate_record under `shape`"""
    with rule(shape):
        return ss.estimate_record(I, Q_samples, cand, a91, R, w4)


def apply_record(xr, xi, info, tones, A, w4, shape):
    with rule(shape):
        return ss.apply_record(xr, xi, info, tones, A, w4)


def subtract(iq, msgs, refined, first, n_msgs, w4, shape, info=None, order=None):
    """the restatement of ft8gpu_subtract_messages_shaped; the arguments of ft8_spec_subtract.subtract with the shape"""
    with rule(shape):
        return ss.subtract(iq, msgs, refined, first, n_msgs, w4, info=info, order=order)


def decode_passes_subtracted(oracle, iq, passes, shape, **kw):
    """the restatement of ft8gpu_decode_messages_subtracted_shaped; the arguments of ft8_spec_subtract.decode_passes_subtracted
    with the shape (the refine stage is the same for both shapes)"""
    with rule(shape):
        return ss.decode_passes_subtracted(oracle, iq, passes, **kw)
