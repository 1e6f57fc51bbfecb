"""CPU restatement of the subtraction in the I/Q samples (ft8gpu_subtract_messages, ft8gpu_decode_messages_subtracted;
include/ft8gpu.h "subtraction in the I/Q samples", DESIGN.md "Subtraction in the I/Q samples") in numpy.  float32 throughout,
every sum formed in the stated order by an explicit loop (np.sum is pairwise), products and sums as separate numpy operations
(nothing fused), every phase an exact integer index, so the device compares byte for byte.

  T, F, tone[m]: those of tests/ft8_spec_refine.py;  u* = the first largest of R.pf[1 .. 3]
  w4 = (cos, -sin)(2 pi i / 4096) from ft8gpu_subtract_twiddles, an input here as the oracle's table is to the refine restatement
  K_m = k4 + 8 tone[m];  Theta_0 = 0, Theta_(m+1) = (Theta_m + 512 K_m) mod 4096;  theta(j) = (Theta_m + K_m (j - s_m)) mod 4096
  z(j) = x[j] * w4[theta(j)];  seg(S, k4, q) = z summed over j = S + 32 q .. S + 32 q + 31, ascending from +0
  P(S, k4) = sum over m ascending of |seg(16 m) + ... + seg(16 m + 15)|^2
  S_0 = 256 T + 256 + 32 R.e_best;  pf[d + 2] = P(S_0, 4 (F + u* - 2) + d);  pt[t + 2] = P(S_0 + 8 t, k4*);  first strict maxima
  A(q) = (G(p_lo) + ... + G(p_hi)) * inv[n], G = seg(S*, k4*, .), p_lo = max(0, q - 8), p_hi = min(1263, q + 8)
  x'[j] = x'[j] - A(q) conj(w4[theta(j)]) for the records in order"""
import numpy as np

import ft8_spec_refine as sr

NSAMPLES = sr.NSAMPLES
MAX_MESSAGES = sr.MAX_MESSAGES
TABLE, SMOOTH, RANGE, TSTEP = 4096, 8, 2, 8
NSEG = 16 * 79
SPAN = 512 * 79
INFO_DTYPE = np.dtype([("k4", "<i4"), ("s_best", "<i4"), ("d_best", "i1"), ("t_best", "i1"), ("valid", "u1"), ("pad0", "u1"),
                       ("pf", "<f4", (5,)), ("pt", "<f4", (5,)), ("pad", "u1", (12,))])
assert INFO_DTYPE.itemsize == 64
F32 = np.float32
INV = np.array([0.0] + [1.0 / (32.0 * n) for n in range(1, 2 * SMOOTH + 2)]).astype(F32)     # (float)(1.0 / (32 n))


def twiddles():
    """w4 from the library's host helper, float32 [4096][2]"""
    import rtlsdr_ft8d_amd as ft8
    return ft8.subtract_twiddles()


def big_theta(k4, tones):
    """Theta_m, m = 0 .. 78, by the recurrence of the rule"""
    th = np.zeros(79, np.int64)
    for m in range(78):
        th[m + 1] = (th[m] + 512 * (int(k4) + 8 * int(tones[m]))) % TABLE
    return th


def theta(S, k4, tones):
    """(j, theta(j)) for the 40448 samples of a record that starts at S: int64 arrays [79][512]"""
    K = int(k4) + 8 * np.asarray(tones, np.int64)
    r = np.arange(512, dtype=np.int64)
    th = (big_theta(k4, tones)[:, None] + K[:, None] * r[None, :]) % TABLE
    j = int(S) + 512 * np.arange(79, dtype=np.int64)[:, None] + r[None, :]
    return j, th


def segment_sums(I, Q, w4, tones, S, k4):
    """seg(S, k4, q) as (re, im) float32 [79][16]"""
    j, th = theta(S, k4, tones)
    inside = (j >= 0) & (j < NSAMPLES)
    jc = np.clip(j, 0, NSAMPLES - 1)
    xr = np.where(inside, I[jc], F32(0)).astype(F32).reshape(79, 16, 32)
    xi = np.where(inside, Q[jc], F32(0)).astype(F32).reshape(79, 16, 32)
    wr, wi = w4[th, 0].reshape(79, 16, 32), w4[th, 1].reshape(79, 16, 32)
    zr = xr * wr - xi * wi
    zi = xr * wi + xi * wr
    assert zr.dtype == F32 and zi.dtype == F32
    gr = np.zeros((79, 16), F32)
    gi = np.zeros((79, 16), F32)
    for i in range(32):
        gr = gr + zr[:, :, i]
        gi = gi + zi[:, :, i]
    return gr, gi


def power(gr, gi):
    """P of one (S, k4): float32"""
    cr = np.zeros(79, F32)
    ci = np.zeros(79, F32)
    for t in range(16):
        cr = cr + gr[:, t]
        ci = ci + gi[:, t]
    p = cr * cr + ci * ci
    P = F32(0)
    for m in range(79):
        P = F32(P + p[m])
    return P


def first_max(v):
    at, best = 0, v[0]
    for i in range(1, len(v)):
        if v[i] > best:
            at, best = i, v[i]
    return at


def estimate_record(I, Q, cand, a91, R, w4):
    """(info INFO_DTYPE record, tones, A (re, im) float32 [1264]) or (all-zero info, None, None) when R.valid == 0"""
    info = np.zeros(1, INFO_DTYPE)[0]
    if int(R["valid"]) == 0:
        return info, None, None
    I = np.ascontiguousarray(I, F32)
    Q = np.ascontiguousarray(Q, F32)
    T = 2 * int(cand["time_offset"]) + int(cand["time_sub"])
    Fq = 2 * int(cand["freq_offset"]) + int(cand["freq_sub"])
    tones = sr.tones_of_a91(a91)
    us = 1
    for u in (2, 3):
        if R["pf"][u] > R["pf"][us]:
            us = u
    S0 = 256 * T + sr.LEAD + 32 * int(R["e_best"])
    k4_0 = 4 * (Fq + us - 2)
    pf = np.array([power(*segment_sums(I, Q, w4, tones, S0, k4_0 + d)) for d in range(-RANGE, RANGE + 1)], F32)
    k4 = k4_0 + first_max(pf) - RANGE
    pt = np.array([power(*segment_sums(I, Q, w4, tones, S0 + TSTEP * t, k4)) for t in range(-RANGE, RANGE + 1)], F32)
    S = S0 + TSTEP * (first_max(pt) - RANGE)
    gr, gi = segment_sums(I, Q, w4, tones, S, k4)
    gr, gi = gr.reshape(-1), gi.reshape(-1)
    # A(q): 17 shifted copies added in ascending p; a term outside 0 .. 1263 is skipped, not added as a zero
    ar = np.zeros(NSEG, F32)
    ai = np.zeros(NSEG, F32)
    q = np.arange(NSEG)
    for o in range(-SMOOTH, SMOOTH + 1):
        ok = (q + o >= 0) & (q + o < NSEG)
        p = np.clip(q + o, 0, NSEG - 1)
        ar = np.where(ok, ar + gr[p], ar).astype(F32)
        ai = np.where(ok, ai + gi[p], ai).astype(F32)
    n = np.minimum(q + SMOOTH, NSEG - 1) - np.maximum(q - SMOOTH, 0) + 1
    ar = ar * INV[n]
    ai = ai * INV[n]
    assert ar.dtype == F32
    info["k4"], info["s_best"], info["d_best"], info["t_best"], info["valid"] = k4, S, k4 - k4_0, (S - S0) // TSTEP, 1
    info["pf"], info["pt"] = pf, pt
    return info, tones, (ar, ai)


def apply_record(xr, xi, info, tones, A, w4):
    """x' = x' - A conj(w4[theta]) over the record's samples inside the frame, in place"""
    j, th = theta(int(info["s_best"]), int(info["k4"]), tones)
    j, th = j.reshape(-1), th.reshape(-1)
    q = np.arange(SPAN) >> 5
    ok = (j >= 0) & (j < NSAMPLES)
    j, th, q = j[ok], th[ok], q[ok]
    ar, ai = A[0][q], A[1][q]
    wr, wi = w4[th, 0], w4[th, 1]
    xr[j] = xr[j] - (ar * wr + ai * wi)
    xi[j] = xi[j] - (ai * wr - ar * wi)


def subtract(iq, msgs, refined, first, n_msgs, w4, info=None, order=None):
    """the restatement of ft8gpu_subtract_messages: iq [B][2][48000], msgs / refined [B][50], first / n_msgs [B]; info: the
    caller's array before the call (zeros if None).  order: a function mapping the list of a frame's record indices to the order
    they are applied in (tests only; the rule is ascending).  Returns (iq_out, info)."""
    iq = np.ascontiguousarray(iq, F32)
    B = iq.shape[0]
    out = iq.copy()
    info = np.zeros((B, MAX_MESSAGES), INFO_DTYPE) if info is None else np.array(info, copy=True)
    clamp = lambda v: min(max(int(v), 0), MAX_MESSAGES)
    for f in range(B):
        recs = list(range(clamp(first[f]), clamp(n_msgs[f])))
        est = {}
        for i in recs:                                   # every estimate from the input frame
            est[i] = estimate_record(iq[f, 0], iq[f, 1], msgs[f, i]["cand"], msgs[f, i]["a91"].tobytes(), refined[f, i], w4)
            info[f, i] = est[i][0]
        for i in (order(recs) if order else recs):
            if est[i][1] is not None:
                apply_record(out[f, 0], out[f, 1], *est[i], w4)
    return out, info


def decode_passes_subtracted(oracle, iq, passes, w4=None, max_candidates=120, min_score=10, nthreads=8, msgs=None, stages=None, iters=20):
    """the whole path for B frames [B][2][48000] -> (msgs [B][50], n [B], n_by_pass [B][passes], residual [B][2][48000]), built
    like ft8_spec_multipass.decode_passes from the oracle's stages, ft8_spec_refine and ft8_spec_multipass.append.
    stages: the first pass's oracle stages (mag, cands, counts, status) when the caller has them already."""
    import ft8_spec_messages as sm
    import ft8_spec_multipass as mp
    import rtlsdr_ft8d_amd as ft8
    iq = np.ascontiguousarray(iq, F32)
    w4 = twiddles() if w4 is None else w4
    tw = sr.twiddles(oracle)
    mag, cands, counts, status = stages if stages is not None else sm.oracle_stages(oracle, iq, max_candidates, min_score, nthreads, iters)
    B = mag.shape[0]
    out, n = sm.collect(mag, cands, counts, status, min_score=min_score,
                        msgs=np.zeros((B, MAX_MESSAGES), ft8.MESSAGE_DTYPE) if msgs is None else msgs)
    base = sm.noise_baseline(mag)
    nbp = np.zeros((B, passes), np.int32)
    nbp[:, 0] = n
    x = iq.copy()
    prev = np.zeros(B, np.int32)                       # counts before the last pass
    for p in range(1, passes):
        active = [f for f in range(B) if prev[f] < n[f] < MAX_MESSAGES]
        if active:
            a = np.array(active)
            ref = np.zeros((len(a), MAX_MESSAGES), sr.REFINED_DTYPE)
            for k, f in enumerate(active):             # the device refines [0, n); only [prev, n) is read
                for i in range(int(prev[f]), int(n[f])):
                    ref[k, i] = sr.refine_record(x[f, 0], x[f, 1], out[f, i]["cand"], out[f, i]["a91"].tobytes(), tw)
            x[a], _info = subtract(x[a], out[a], ref, prev[a], n[a], w4)
            W = oracle.waterfall_batch(x[a], nthreads=nthreads)
            c2, k2 = oracle.find_sync_batch(W, max_candidates, min_score, nthreads=nthreads)
            s2 = oracle.decode_candidates_batch(W, c2, k2, iters=iters, nthreads=nthreads)
            prev = n.copy()
            o2, n2 = mp.append(W, base[a], c2, k2, s2, out[a], n[a], min_score=min_score)
            out[a], n[a] = o2, n2
        else:
            prev = n.copy()
        nbp[:, p] = n
    return out, n, nbp, x
