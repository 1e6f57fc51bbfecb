"""CPU restatement of the second demodulation (ft8gpu_demod_candidates, ft8gpu_decode_messages_demod; include/ft8gpu.h
"demodulation from the I/Q samples", DESIGN.md "Demodulation from the I/Q samples") in numpy.  float32 throughout, every
product and sum a separate numpy operation (nothing fused), every phase an exact integer table index, every sum in the order
the rule states: the eight strided products of a lane, the 8-point DFT as written out below, the lane twiddle, and the xor
butterfly over the 64 lanes as a loop over its six levels.  The device compares byte for byte.

  T = 2 time_offset + time_sub, F = 2 freq_offset + freq_sub, w4 = (cos, -sin)(2 pi i / 4096) (ft8gpu_subtract_twiddles)
  C(m, t; S, k4): lane l < 64, a < 8, n = 512 m + l + 64 a:  y_a = x[S + n] * w4[(k4 n) mod 4096];  U_t = DFT8(y)_t;
    V_t = U_t * w4[(8 t l) mod 4096];  C = the butterfly sum of V_t over the lanes
  S(e) = 256 T + 256 + 32 e;  Psync(e, d) = the sum over the 21 Costas symbols, ascending from +0, of re^2 + im^2 of
    C(m, costas[m]; S(e), 4 F + d);  e* = first strict maximum over e = -4 .. 4 at d = 0, then d* over d = -2 .. 2 at e*
  Z[m][t] = C(m, t; S(e*), 4 F + d*);  sets n = 1, 2, 3: blocks of n data symbols per half, A = sqrtf(re^2 + im^2) of the sum
    of the block's Z entries, llr = max(A | bit set) - max(A | bit clear), x = ftx_normalize_logl(llr), bp_decode(x)"""
import numpy as np

import ft8_spec_combine as sc
import ft8_spec_osd as so

F32 = np.float32
NSAMPLES = 48000
MAX_MESSAGES = 50
LEAD = 256
TSTEP, TRANGE, FRANGE = 32, 4, 2
TAB = 4096
COSTAS = (3, 1, 4, 0, 6, 5, 2)
GRAY = (0, 1, 3, 2, 5, 6, 4, 7)
COSTAS_SYMS = tuple(list(range(0, 7)) + list(range(36, 43)) + list(range(72, 79)))
INFO_DTYPE = np.dtype([("result", "u1"), ("set", "u1"), ("nhard", "u1"), ("e_best", "i1"), ("d_best", "i1"), ("pad0", "u1", (3,)),
                       ("psync", "<f4"), ("pad", "u1", (4,))])
assert INFO_DTYPE.itemsize == 16 and INFO_DTYPE.fields["psync"][1] == 8
C8 = F32(np.sqrt(0.5))                       # 0x3F3504F3, the float of cos(pi / 4)
CANONICAL_NAN = np.uint32(0x7FC00000)
MAX_HARD_ERRORS = 174                        # FT8GPU_DEMOD_MAX_HARD_ERRORS
SETS = 7                                     # FT8GPU_DEMOD_SETS


def twiddles():
    import rtlsdr_ft8d_amd as ft8
    return ft8.subtract_twiddles()


def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def _dft4(v0, v1, v2, v3):
    """the 4-point DFT of the rule: four complex (re, im) pairs in, outputs 0 .. 3"""
    e0 = (v0[0] + v2[0], v0[1] + v2[1])
    e1 = (v0[0] - v2[0], v0[1] - v2[1])
    o0 = (v1[0] + v3[0], v1[1] + v3[1])
    o1 = (v1[0] - v3[0], v1[1] - v3[1])
    return ((e0[0] + o0[0], e0[1] + o0[1]), (e1[0] + o1[1], e1[1] - o1[0]),
            (e0[0] - o0[0], e0[1] - o0[1]), (e1[0] - o1[1], e1[1] + o1[0]))


def dft8(yr, yi):
    """U_t = sum over a of y_a exp(-2 pi i t a / 8) in the rule's operation order; yr, yi [..., 8] -> [..., 8]"""
    p = [(yr[..., a] + yr[..., a + 4], yi[..., a] + yi[..., a + 4]) for a in range(4)]
    q = [(yr[..., a] - yr[..., a + 4], yi[..., a] - yi[..., a + 4]) for a in range(4)]
    q1 = ((q[1][0] + q[1][1]) * C8, (q[1][1] - q[1][0]) * C8)
    q2 = (q[2][1], -q[2][0])
    q3 = ((q[3][1] - q[3][0]) * C8, -((q[3][0] + q[3][1]) * C8))
    ev = _dft4(p[0], p[1], p[2], p[3])
    od = _dft4(q[0], q1, q2, q3)
    order = (ev[0], od[0], ev[1], od[1], ev[2], od[2], ev[3], od[3])
    return np.stack([u[0] for u in order], axis=-1), np.stack([u[1] for u in order], axis=-1)


def butterfly(v):
    """the xor butterfly over the last axis (64 lanes), levels 1, 2, 4, 8, 16, 32; every lane ends with the same sum"""
    lanes = np.arange(64)
    for mask in (1, 2, 4, 8, 16, 32):
        v = v + v[..., lanes ^ mask]
    return v[..., 0]


def correlate(I, Q, w4, S, k4, ms):
    """C(m, t; S[h], k4[h]) for hypotheses h and the symbols ms -> (re, im) float32 [H][len(ms)][8]"""
    S = np.atleast_1d(np.asarray(S, np.int64))
    k4 = np.atleast_1d(np.asarray(k4, np.int64))
    ms = np.asarray(ms, np.int64)
    lane = np.arange(64, dtype=np.int64)
    a = np.arange(8, dtype=np.int64)
    n = 512 * ms[:, None, None] + lane[None, :, None] + 64 * a[None, None, :]             # [M][64][8]
    j = S[:, None, None, None] + n[None]
    inside = (j >= 0) & (j < NSAMPLES)
    jc = np.clip(j, 0, NSAMPLES - 1)
    xr = np.where(inside, I[jc], F32(0)).astype(F32)
    xi = np.where(inside, Q[jc], F32(0)).astype(F32)
    idx = (k4[:, None, None, None] * n[None]) & (TAB - 1)
    with np.errstate(all="ignore"):
        yr, yi = _cmul(xr, xi, w4[idx, 0], w4[idx, 1])
        ur, ui = dft8(yr, yi)                                                            # [H][M][64][8]
        lt = (8 * np.arange(8, dtype=np.int64)[None, :] * lane[:, None]) & (TAB - 1)        # [64][8]
        vr, vi = _cmul(ur, ui, w4[lt, 0][None, None], w4[lt, 1][None, None])
        assert vr.dtype == F32 and vi.dtype == F32
        return butterfly(np.moveaxis(vr, 2, -1)), butterfly(np.moveaxis(vi, 2, -1))


def sync_powers(I, Q, w4, S, k4):
    """Psync for the hypotheses (S[h], k4[h]) -> float32 [H]"""
    cr, ci = correlate(I, Q, w4, S, k4, COSTAS_SYMS)
    P = np.zeros(cr.shape[0], F32)
    with np.errstate(all="ignore"):
        for i, m in enumerate(COSTAS_SYMS):
            t = COSTAS[m % 36]
            P = P + (cr[:, i, t] * cr[:, i, t] + ci[:, i, t] * ci[:, i, t])
    return P


def first_strict_max(p):
    at, best = 0, p[0]
    for h in range(1, len(p)):
        if p[h] > best:
            at, best = h, p[h]
    return at


def fine_sync(I, Q, w4, T, Fq):
    """(e*, d*, Psync(e*, d*), the nine time powers, the five frequency powers)"""
    S0 = 256 * T + LEAD
    es = np.arange(-TRANGE, TRANGE + 1)
    pt = sync_powers(I, Q, w4, S0 + TSTEP * es, np.full(len(es), 4 * Fq))
    e = int(es[first_strict_max(pt)])
    ds = np.arange(-FRANGE, FRANGE + 1)
    pf = sync_powers(I, Q, w4, np.full(len(ds), S0 + TSTEP * e), 4 * Fq + ds)
    assert pf[FRANGE].tobytes() == pt[e + TRANGE].tobytes()        # d = 0 is the time search's best: the device does not form it again
    d = int(ds[first_strict_max(pf)])
    return e, d, pf[d + FRANGE], pt, pf


def spectra(I, Q, w4, T, Fq, e, d):
    """Z [79][8] as (re, im)"""
    zr, zi = correlate(I, Q, w4, [256 * T + LEAD + TSTEP * e], [4 * Fq + d], np.arange(79))
    return zr[0], zi[0]


def blocks(n):
    """the blocks of set n: lists of symbol indices m, first half then second half"""
    out = []
    for first in (7, 43):
        for i in range(0, 29, n):
            out.append([first + k for k in range(i, min(i + n, 29))])
    return out


def data_index(m):
    return m - 7 if m < 36 else m - 14


def soft_bits(zr, zi, n):
    """the 174 max-log soft bits of set n, or None when a magnitude is not finite"""
    llr = np.zeros(174, F32)
    gray = np.array(GRAY)
    with np.errstate(all="ignore"):
        for blk in blocks(n):
            b = len(blk)
            re = zr[blk[0]][gray].reshape((8,) + (1,) * (b - 1))
            im = zi[blk[0]][gray].reshape((8,) + (1,) * (b - 1))
            for s in range(1, b):                                   # added in symbol order
                shape = (1,) * s + (8,) + (1,) * (b - 1 - s)
                re = re + zr[blk[s]][gray].reshape(shape)
                im = im + zi[blk[s]][gray].reshape(shape)
            A = np.sqrt(re * re + im * im)
            assert A.dtype == F32 and A.shape == (8,) * b
            if not np.isfinite(A).all():
                return None
            for s, m in enumerate(blk):
                As = np.moveaxis(A, s, 0).reshape(8, -1)
                for k in range(3):
                    bit = ((np.arange(8) >> (2 - k)) & 1).astype(bool)
                    llr[3 * data_index(m) + k] = As[bit].max() - As[~bit].max()
    return llr


def judge(oracle, plain, errors, x, gate):
    """combine's checks with the hard-error gate between the all-zero test and the CRC"""
    plain = np.asarray(plain, np.uint8)
    if errors != 0:
        return 7, 0, 0, 0, 0, b""
    nhard = int((plain != (x > 0)).sum())
    if not plain.any():
        return 5, nhard, 0, 0, 0, b""
    if nhard > gate:
        return 2, nhard, 0, 0, 0, b""
    return sc.judge(oracle, plain, errors, x)


def analyse(I, Q, cand, w4, iters=20, bp=None):
    """everything of a candidate that does not depend on the parameters: (e*, d*, psync, {n: (llr, x, plain, errors)}), x None
    for a set that is not finite (llr None when a magnitude is not)"""
    T, Fq = sc.position(cand)
    e, d, psync, _pt, _pf = fine_sync(I, Q, w4, T, Fq)
    zr, zi = spectra(I, Q, w4, T, Fq, e, d)
    per_set = {}
    for n in (1, 2, 3):
        llr = soft_bits(zr, zi, n)
        x = sc.normalized(llr) if llr is not None else None
        if x is None or not np.isfinite(x).all():
            per_set[n] = (llr, None, None, None)
            continue
        plain, errors, _it = (bp or sc.numpy_bp())(x, iters)
        per_set[n] = (llr, x, np.array(plain, np.uint8), errors)
    return e, d, psync, per_set


def demod_one(oracle, I, Q, cand, w4, sets, gate, iters=20, bp=None, analysis=None):
    """one attempted candidate -> (info record, None or (plain, ext, calc, rc, text))"""
    info = np.zeros(1, INFO_DTYPE)[0]
    e, d, psync, per_set = analysis if analysis is not None else analyse(I, Q, cand, w4, iters, bp)
    info["e_best"], info["d_best"] = e, d
    info["psync"] = psync if not np.isnan(psync) else CANONICAL_NAN.view(F32)
    for n in (1, 2, 3):
        if not (sets >> (n - 1)) & 1:
            continue
        info["set"], info["nhard"] = n, 0
        _llr, x, plain, errors = per_set[n]
        if x is None:
            info["result"] = 6
            continue
        code, nhard, ext, calc, rc, text = judge(oracle, plain, errors, x, gate)
        info["result"], info["nhard"] = code, nhard
        if code == 1:
            return info, (plain, ext, calc, rc, text)
    return info, None


def demod_candidates(oracle, iq, cands, counts, status_in, sets=SETS, gate=MAX_HARD_ERRORS, max_per_frame=None, status_out=None,
                     info=None, iters=20, bp=None, w4=None, cache=None):
    """ft8gpu_demod_candidates: iq [B][2][48000], cands [B][cap], counts [B], status_in uint8 [B][cap][48] (or STATUS_DTYPE) ->
    (status_out uint8 [B][cap][48], info INFO_DTYPE [B][cap]).  Records at and behind counts[f] keep what status_out / info held
    (zeros when None).  cache: a dict that keeps analyse() of (frame, candidate bytes) between calls on the same frames with the
    same iters."""
    import rtlsdr_ft8d_amd as ft8
    iq = np.ascontiguousarray(iq, F32).reshape(-1, 2, NSAMPLES)
    B = iq.shape[0]
    w4 = twiddles() if w4 is None else w4
    sin = np.ascontiguousarray(status_in).view(np.uint8).reshape(B, -1, 48)
    cap = sin.shape[1]
    max_per_frame = cap if max_per_frame is None else max_per_frame
    out = np.zeros((B, cap, 48), np.uint8) if status_out is None else np.array(status_out, copy=True).view(np.uint8).reshape(B, cap, 48)
    inf = np.zeros((B, cap), INFO_DTYPE) if info is None else np.array(info, copy=True).view(INFO_DTYPE).reshape(B, cap)
    st = sin.view(ft8.STATUS_DTYPE).reshape(B, cap)
    for f in range(B):
        attempted = 0
        for i in range(int(counts[f])):
            out[f, i] = sin[f, i]
            inf[f, i] = np.zeros(1, INFO_DTYPE)[0]
            if not (st[f, i]["ok"] == 0 and st[f, i]["ldpc_errors"] != 0) or attempted >= max_per_frame:
                continue
            attempted += 1
            key = (f, cands[f, i].tobytes())                         # the analysis is the frame's and the record's, wherever it stands
            if cache is None or key not in cache:
                analysis = analyse(iq[f, 0], iq[f, 1], cands[f, i], w4, iters, bp)
                if cache is not None:
                    cache[key] = analysis
            else:
                analysis = cache[key]
            rec_info, win = demod_one(oracle, iq[f, 0], iq[f, 1], cands[f, i], w4, sets, gate, iters, bp, analysis)
            inf[f, i] = rec_info
            if win is not None:
                plain, ext, calc, rc, text = win
                rec = np.zeros(1, ft8.STATUS_DTYPE)[0]
                rec["ldpc_errors"] = 0
                rec["iters"] = st[f, i]["iters"]
                rec["crc_extracted"], rec["crc_calculated"] = ext, calc
                rec["unpack_status"], rec["ok"] = rc, 1
                rec["a91"] = so.a91_of(plain)
                rec["text"] = text
                out[f, i] = np.frombuffer(rec.tobytes(), np.uint8)
    return out, inf


def decode_demod(oracle, iq, sets=SETS, gate=MAX_HARD_ERRORS, max_per_frame=None, msgs=None, max_candidates=120, min_score=10,
                 nthreads=8, iters=20, stages=None, bp=None, trace=None, cache=None):
    """ft8gpu_decode_messages_demod for iq [B][2][48000] -> (msgs [B][50], n [B], n_by_stage [B][2]): the records of
    ft8gpu_decode_messages, the stage in place on the BP status records, the append step on what it accepted (pad[3] = the
    accepted set).  stages: the oracle's (mag, cands, counts, status), to spare recomputing them.  trace: receives info [B][cap]."""
    import rtlsdr_ft8d_amd as ft8
    import ft8_spec_messages as sm
    import ft8_spec_multipass as mp
    iq = np.ascontiguousarray(iq, F32).reshape(-1, 2, NSAMPLES)
    B = iq.shape[0]
    mag, cands, counts, status = stages if stages is not None else sm.oracle_stages(oracle, iq, max_candidates, min_score, nthreads, iters)
    out, n = sm.collect(mag, cands, counts, status, min_score=min_score,
                        msgs=np.zeros((B, MAX_MESSAGES), ft8.MESSAGE_DTYPE) if msgs is None else np.array(msgs).reshape(B, MAX_MESSAGES))
    nbs = np.zeros((B, 2), np.int32)
    nbs[:, 0] = n
    st2, info = demod_candidates(oracle, iq, cands, counts, status, sets, gate, max_per_frame, iters=iters, bp=bp, cache=cache)
    o2, n2 = mp.append(mag, sm.noise_baseline(mag), cands, counts, st2, out, n, min_score=min_score)
    for f in range(B):
        for r in range(int(n[f]), int(n2[f])):
            o2[f, r]["pad"][3] = info[f, int(o2[f, r]["cand_index"])]["set"]
    nbs[:, 1] = n2
    if trace is not None:
        trace.append(info)
    return o2, n2, nbs
