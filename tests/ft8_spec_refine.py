"""CPU restatement of the refined time and frequency (ft8gpu_refine_messages, ft8gpu_refined_estimate; include/ft8gpu.h
"refined time and frequency", DESIGN.md "Refined time and frequency") in numpy.  float32 throughout, every sum formed in the
stated order by an explicit loop (np.sum is pairwise), products and sums as separate numpy operations (nothing fused), so the
device compares byte for byte.

  T = 2 time_offset + time_sub, F = 2 freq_offset + freq_sub, tone[m] from the 91 stored bits of a91 (generator parities,
  Gray map, Costas arrays), w = the oracle's twiddle table (cos, -sin)(2 pi i / 1024)
  y(k, j) = x[j] * w[(k j) mod 1024];  g(k, q) = sum of y over j = 32 q .. 32 q + 31, ascending, from +0
  s_m(e) = 256 T + 256 + 512 m + 32 e;  c(m, k, e) = sum of g(k, q0 .. q0 + 15), ascending, q0 = s_m(e) / 32
  P(u, e) = sum over m ascending of re(c)^2 + im(c)^2 with k = F + 2 tone[m] + u
  pt_all[e + 16] = P(0, e), e = -16 .. 16; e_best = the first strict maximum; pf[u + 2] = P(u, e_best);
  noise = the same with k = F + 2 ((tone[m] + 4) & 7)"""
import math

import numpy as np

import ft8_spec_osd as so

NSAMPLES = 48000
MAX_MESSAGES = 50
LEAD, STEP, RANGE = 256, 32, 16
NOFF = 2 * RANGE + 1
SYM_SEGS = 512 // STEP
COSTAS = (3, 1, 4, 0, 6, 5, 2)
GRAY = (0, 1, 3, 2, 5, 6, 4, 7)
REFINED_DTYPE = np.dtype([("e_best", "<i2"), ("valid", "u1"), ("pad0", "u1"), ("pt", "<f4", (3,)), ("pf", "<f4", (5,)),
                          ("noise", "<f4"), ("pad", "u1", (8,))])
assert REFINED_DTYPE.itemsize == 48
F32 = np.float32


def twiddles(oracle):
    """the oracle's FFT twiddle table, float32 [1024][2]"""
    return np.ctypeslib.as_array(oracle.lib().ft8o_twiddles(), (1024, 2)).copy()


def tones_of_a91(a91):
    """79 tones from the 91 bits of a91 as stored: codeword = bits x generator, Gray map, Costas arrays"""
    bits = np.unpackbits(np.frombuffer(bytes(a91)[:12], np.uint8))[:91].astype(np.int64)
    cw = (bits @ so.generator_matrix().astype(np.int64)) & 1
    tones = np.zeros(79, np.int64)
    for m in range(79):
        if m < 7 or 36 <= m < 43 or m >= 72:
            tones[m] = COSTAS[m % 36]                    # the arrays start at 0, 36 and 72
        else:
            d = m - 7 if m < 36 else m - 14
            tones[m] = GRAY[int(cw[3 * d]) << 2 | int(cw[3 * d + 1]) << 1 | int(cw[3 * d + 2])]
    return tones


def segment_sums(I, Q, tw, k, j0, nseg):
    """g(k[m], q) for the nseg segments from sample j0[m] (a multiple of 32) of each symbol m -> (re, im) float32 [79][nseg]"""
    k = np.asarray(k, np.int64)
    j0 = np.asarray(j0, np.int64)
    j = j0[:, None, None] + STEP * np.arange(nseg, dtype=np.int64)[None, :, None] + np.arange(STEP, dtype=np.int64)[None, None, :]
    inside = (j >= 0) & (j < NSAMPLES)
    jc = np.clip(j, 0, NSAMPLES - 1)
    xr = np.where(inside, I[jc], F32(0)).astype(F32)
    xi = np.where(inside, Q[jc], F32(0)).astype(F32)
    idx = (k[:, None, None] * j) & 1023
    wr, wi = tw[idx, 0], tw[idx, 1]
    yr = xr * wr - xi * wi
    yi = xr * wi + xi * wr
    assert yr.dtype == F32 and yi.dtype == F32
    gr = np.zeros((len(k), nseg), F32)
    gi = np.zeros((len(k), nseg), F32)
    for i in range(STEP):
        gr = gr + yr[:, :, i]
        gi = gi + yi[:, :, i]
    return gr, gi


def powers(gr, gi):
    """P for every window of 16 consecutive segments: float32 [nseg - 15]"""
    nwin = gr.shape[1] - SYM_SEGS + 1
    cr = np.zeros((gr.shape[0], nwin), F32)
    ci = np.zeros((gr.shape[0], nwin), F32)
    for t in range(SYM_SEGS):
        cr = cr + gr[:, t:t + nwin]
        ci = ci + gi[:, t:t + nwin]
    p = cr * cr + ci * ci
    P = np.zeros(nwin, F32)
    for m in range(gr.shape[0]):
        P = P + p[m]
    return P


def refine_record(I, Q, cand, a91, tw):
    """one REFINED_DTYPE record"""
    I = np.ascontiguousarray(I, F32)
    Q = np.ascontiguousarray(Q, F32)
    T = 2 * int(cand["time_offset"]) + int(cand["time_sub"])
    Fq = 2 * int(cand["freq_offset"]) + int(cand["freq_sub"])
    tones = tones_of_a91(a91)
    sym = 256 * T + LEAD + 512 * np.arange(79, dtype=np.int64)
    pt_all = powers(*segment_sums(I, Q, tw, Fq + 2 * tones, sym - STEP * RANGE, SYM_SEGS + 2 * RANGE))
    assert pt_all.shape == (NOFF,)
    eb, best = 0, pt_all[0]
    for e in range(1, NOFF):
        if pt_all[e] > best:
            eb, best = e, pt_all[e]
    rec = np.zeros(1, REFINED_DTYPE)[0]
    rec["e_best"] = eb - RANGE
    rec["valid"] = 1
    rec["pt"] = [pt_all[eb - 1] if eb >= 1 else F32(0), pt_all[eb], pt_all[eb + 1] if eb + 1 < NOFF else F32(0)]
    at = sym + STEP * (eb - RANGE)
    pf = np.zeros(5, F32)
    for u in (-2, -1, 1, 2):
        pf[u + 2] = powers(*segment_sums(I, Q, tw, Fq + 2 * tones + u, at, SYM_SEGS))[0]
    pf[2] = pt_all[eb]
    rec["pf"] = pf
    rec["noise"] = powers(*segment_sums(I, Q, tw, Fq + 2 * ((tones + 4) & 7), at, SYM_SEGS))[0]
    return rec


def refine(iq, msgs, n_msgs, tw, refined=None):
    """the restatement of ft8gpu_refine_messages: iq [B][2][48000], msgs [B][50], n_msgs [B]; refined: the caller's array before
    the call (zeros if None).  Returns refined [B][50] REFINED_DTYPE."""
    iq = np.ascontiguousarray(iq, F32)
    B = iq.shape[0]
    out = np.zeros((B, MAX_MESSAGES), REFINED_DTYPE) if refined is None else np.array(refined, copy=True)
    for f in range(B):
        for i in range(min(max(int(n_msgs[f]), 0), MAX_MESSAGES)):
            out[f, i] = refine_record(iq[f, 0], iq[f, 1], msgs[f, i]["cand"], msgs[f, i]["a91"].tobytes(), tw)
    return out


# ---- the host helper (ft8gpu_refined_estimate), in Python doubles ---------------------------------------------------------

def vertex(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return 0.0
    den = a - 2.0 * b + c
    if not den < 0.0:
        return 0.0
    return min(0.5, max(-0.5, 0.5 * (a - c) / den))


FLT_MIN = float(np.finfo(np.float32).tiny)


def estimate(cand, rec):
    """(dt_s, freq_hz, snr_db) as float32, or None when the record is not valid"""
    if int(rec["valid"]) == 0:
        return None
    T = 2 * int(cand["time_offset"]) + int(cand["time_sub"])
    Fq = 2 * int(cand["freq_offset"]) + int(cand["freq_sub"])
    e = int(rec["e_best"])
    pt, pf = [float(v) for v in rec["pt"]], [float(v) for v in rec["pf"]]
    vt = 0.0 if (e - 1 < -RANGE or e + 1 > RANGE) else vertex(*pt)
    dt = (256.0 * T + LEAD + STEP * (e + vt)) / 3200.0
    us = 1
    for u in (2, 3):
        if pf[u] > pf[us]:
            us = u
    freq = 3.125 * (Fq + (us - 2) + vertex(pf[us - 1], pf[us], pf[us + 1]))
    noise, sig = float(rec["noise"]), pf[2]
    if not noise > 0.0 or not math.isfinite(noise):
        snr = 49.0 if sig > 0.0 else -30.0
    else:
        s = sig - noise
        if not s > FLT_MIN:
            s = FLT_MIN
        snr = 10.0 * math.log10(s / noise * 6.25 / 2500.0)
        if not snr > -30.0:
            snr = -30.0
        snr = min(snr, 49.0)
    return F32(dt), F32(freq), F32(snr)
