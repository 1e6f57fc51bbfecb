"""CPU restatement of ordered-statistics decoding (ft8gpu_osd_candidates, DESIGN.md "Ordered-statistics decoding") in
numpy.  It is fed by the oracle's normalised soft bits (oracle_lib.llr) and takes the generator from the project's tables
(csrc/ft8_tables.h).  Integers and float32 comparisons only, so the device compares byte for byte.

The rule.  A candidate whose status record has ok == 0 and ldpc_errors != 0 is decoded again:
  h[i] = llr[i] > 0;  w[i] = 255 if |llr[i]| >= 32 else int(|llr[i]| * 8)
  positions sorted by the bit pattern of |llr[i]| (uint32) descending, ties by ascending i
  the 91 first independent columns of G in that order are the basis; R_k = the row of the reduced echelon form with its
  1 in the k-th basis column (k = 0 the most reliable)
  pattern 0 = c0 = XOR of the R_k with h = 1 at their basis position; 1 + k = c0 ^ R_k (order >= 1);
  92 + rank(i, j) = c0 ^ R_i ^ R_j, i < j in lexicographic order (order 2)
  metric = sum of w where the pattern differs from h, nhard = the number of those positions; best = smallest
  (metric, index)
  result of the best pattern, first failing check: 5 all-zero, 2 nhard > max_hard_errors, 3 CRC mismatch, 4 unpack77
  fails, 1 accepted; 6 = a non-finite soft bit (nothing searched), 0 = not attempted.
Info record: uint8 result, uint8 nhard, uint16 pattern, int32 metric."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, M = 174, 91, 83
NPAT = (1, 1 + K, 1 + K + K * (K - 1) // 2)           # patterns searched at order 0 / 1 / 2
INFO_DTYPE = np.dtype([("result", "u1"), ("nhard", "u1"), ("pattern", "<u2"), ("metric", "<i4")])
assert INFO_DTYPE.itemsize == 8


def _table(name):
    src = open(os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc", "ft8_tables.h")).read()
    m = re.search(r"%s\[[^=]*=\s*\{(.*?)\};" % name, src, re.S)
    return [int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", m.group(1))]


@functools.lru_cache(None)
def generator_matrix():
    """G uint8 [91][174]: row k = the codeword of the message whose only set bit is k (identity, then the 83 parity bits
    from kFT8_generator: parity m covers message bit k when bit k, MSB first, of generator row m is set)"""
    gen = np.array(_table("kFT8_generator"), np.uint8).reshape(M, 12)
    bits = np.unpackbits(gen, axis=1)[:, :K]             # [83][91]
    G = np.zeros((K, N), np.uint8)
    G[:, :K] = np.eye(K, dtype=np.uint8)
    G[:, K:] = bits.T
    G.setflags(write=False)
    return G


@functools.lru_cache(None)
def parity_check_matrix():
    """H uint8 [83][174] from kFT8_Nm (1-based variable indices, 0 = unused slot)"""
    nm = np.array(_table("kFT8_Nm"), np.int32).reshape(M, 7)
    H = np.zeros((M, N), np.uint8)
    for m in range(M):
        for n in nm[m]:
            if n > 0:
                H[m, n - 1] = 1
    H.setflags(write=False)
    return H


def crc14(bits77):
    """CRC-14 (polynomial 0x2757, zero start, no final XOR) over the 77 payload bits followed by five zero bits"""
    rem = 0
    for b in list(bits77)[:77] + [0] * 5:
        rem ^= int(b) << 13
        rem = ((rem << 1) ^ 0x2757) & 0x3FFF if rem & 0x2000 else (rem << 1) & 0x3FFF
    return rem


def hard_and_weights(llr):
    llr = np.asarray(llr, np.float32)
    a = np.abs(llr)
    h = (llr > 0).astype(np.uint8)
    w = np.where(a >= np.float32(32.0), 255, (np.minimum(a, np.float32(32.0)) * np.float32(8.0)).astype(np.int32)).astype(np.int32)
    return h, w


def sort_order(llr):
    key = np.abs(np.asarray(llr, np.float32)).view(np.uint32).astype(np.int64)
    return np.lexsort((np.arange(N), -key))              # primary: key descending; ties: index ascending


def eliminate(order_idx):
    """full reduction over the columns in sorted order, the free row with the smallest index as pivot -> (pivot rows [91],
    their sorted positions [91], the reduced matrix with its columns in sorted order)"""
    A = np.array(generator_matrix()[:, order_idx], copy=True)          # columns in sorted order
    used = np.zeros(K, bool)
    piv_row, piv_col = [], []
    for c in range(N):
        col = A[:, c].astype(bool)
        free = np.flatnonzero(col & ~used)
        if free.size == 0:
            continue
        p = int(free[0])
        col[p] = False
        A[col] ^= A[p]
        used[p] = True
        piv_row.append(p)
        piv_col.append(c)
        if len(piv_row) == K:
            break
    assert len(piv_row) == K
    return piv_row, piv_col, A


def reduced_basis(order_idx):
    """(basis positions in reliability order [91], R uint8 [91][174] with R[k] the reduced row of basis position k)"""
    piv_row, piv_col, A = eliminate(order_idx)
    R = np.zeros((K, N), np.uint8)
    R[:, order_idx] = A[piv_row]                         # back to codeword order
    return np.asarray(order_idx)[piv_col], R


@functools.lru_cache(None)
def _pairs():
    return np.triu_indices(K, 1)                         # lexicographic i < j


def search(llr):
    """the best pattern at orders 0, 1, 2 -> list of three (metric, pattern, nhard, codeword uint8 [174])"""
    h, w = hard_and_weights(llr)
    basis, R = reduced_basis(sort_order(llr))
    c0 = (h[basis].astype(np.int32) @ R.astype(np.int32) & 1).astype(np.uint8)
    d0 = c0 ^ h
    D1 = d0[None, :] ^ R                                 # [91][174] difference of pattern 1 + k
    m0 = int(w[d0 == 1].sum())
    m1 = D1.astype(np.int32) @ w                         # [91]
    out = []
    best = (m0, 0)
    out.append(best)
    k1 = int(np.argmin(m1))                              # first minimum = smallest index
    if (int(m1[k1]), 1 + k1) < best:
        best = (int(m1[k1]), 1 + k1)
    out.append(best)
    iu, ju = _pairs()
    # metric of d0 ^ R_i ^ R_j = m0 + S_i + S_j - 2 T_ij with s = w where d0 = 0, -w where d0 = 1 (what a flip there costs),
    # S_i = the sum of s over R_i, T_ij = the sum of s over R_i & R_j: exact in int64, without the 4095 x 174 differences
    Rs = R.astype(np.int64) * np.where(d0 == 1, -w, w).astype(np.int64)[None, :]
    S1 = Rs.sum(axis=1)
    T = Rs @ R.astype(np.int64).T
    m2 = m0 + S1[iu] + S1[ju] - 2 * T[iu, ju]             # [4095]
    k2 = int(np.argmin(m2))
    if (int(m2[k2]), 1 + K + k2) < best:
        best = (int(m2[k2]), 1 + K + k2)
    out.append(best)
    res = []
    for metric, pat in out:
        if pat == 0:
            d = d0
        elif pat <= K:
            d = D1[pat - 1]
        else:
            d = D1[iu[pat - 1 - K]] ^ R[ju[pat - 1 - K]]
        res.append((metric, pat, int(d.sum()), d ^ h))
    return res


def a91_of(codeword):
    return np.packbits(np.concatenate([np.asarray(codeword[:K], np.uint8), np.zeros(5, np.uint8)]))


def judge(oracle, codeword, nhard, max_hard_errors):
    """(result code, crc_extracted, crc_calculated, unpack status, text) of a best pattern"""
    cw = np.asarray(codeword, np.uint8)
    if not cw.any():
        return 5, 0, 0, 0, b""
    if nhard > max_hard_errors:
        return 2, 0, 0, 0, b""
    ext = int("".join(map(str, cw[77:91])), 2)
    calc = crc14(cw[:77])
    if ext != calc:
        return 3, ext, calc, 0, b""
    a77 = a91_of(cw).copy()
    a77[9] &= 0xF8
    a77[10] = a77[11] = 0
    rc, text = oracle.unpack77(a77[:10].tobytes())
    if rc < 0:
        return 4, ext, calc, rc, b""
    return 1, ext, calc, rc, text.encode()


def osd_candidates(oracle, mag, cands, counts, status_in, order, max_hard_errors, status_out=None, info=None, searches=None):
    """ft8gpu_osd_candidates: mag [B][94208], cands [B][cap], counts [B], status_in uint8 [B][cap][48] (or STATUS_DTYPE)
    -> (status_out uint8 [B][cap][48], info INFO_DTYPE [B][cap]).  Records at and behind counts[f] keep what status_out /
    info held (zeros when None).  searches: an optional dict (f, i) -> search(llr) result, filled and reused."""
    import rtlsdr_ft8d_amd as ft8
    mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, 94208)
    B = mag.shape[0]
    sin = np.ascontiguousarray(status_in).view(np.uint8).reshape(B, -1, 48)
    cap = sin.shape[1]
    out = np.zeros((B, cap, 48), np.uint8) if status_out is None else np.array(status_out, copy=True).view(np.uint8).reshape(B, cap, 48)
    inf = np.zeros((B, cap), INFO_DTYPE) if info is None else np.array(info, copy=True).view(INFO_DTYPE).reshape(B, cap)
    st = sin.view(ft8.STATUS_DTYPE).reshape(B, cap)
    for f in range(B):
        for i in range(int(counts[f])):
            out[f, i] = sin[f, i]
            inf[f, i] = np.zeros(1, INFO_DTYPE)[0]
            if st[f, i]["ok"] != 0 or st[f, i]["ldpc_errors"] == 0:
                continue
            if searches is not None and (f, i) in searches:
                s = searches[(f, i)]
            else:
                llr = oracle.llr(mag[f], cands[f, i])
                s = search(llr) if np.isfinite(llr).all() else None
                if searches is not None:
                    searches[(f, i)] = s
            if s is None:
                inf[f, i]["result"] = 6
                continue
            metric, pat, nhard, cw = s[order]
            code, ext, calc, rc, text = judge(oracle, cw, nhard, max_hard_errors)
            inf[f, i] = (code, nhard, pat, metric)
            if code == 1:
                rec = np.zeros(1, ft8.STATUS_DTYPE)[0]
                rec["ldpc_errors"] = 0
                rec["iters"] = st[f, i]["iters"]
                rec["crc_extracted"], rec["crc_calculated"] = ext, calc
                rec["unpack_status"], rec["ok"] = rc, 1
                rec["a91"] = a91_of(cw)
                rec["text"] = text
                out[f, i] = np.frombuffer(rec.tobytes(), np.uint8)
    return out, inf


def decode_deep(oracle, iq, passes, order, max_hard_errors, max_candidates=120, min_score=10, nthreads=8, msgs=None, searches=None,
                iters=20):
    """ft8gpu_decode_messages_deep for B frames [B][2][48000] -> (msgs [B][50], n [B], n_by_stage [B][passes][2]): the pass
    loop of tests/ft8_spec_multipass.py with OSD behind every pass -- OSD on the pass's status records, the append step on
    what it accepted, pad[0] of a gained record = the pattern's nhard.  order -1: no OSD.  searches: a dict that carries the
    first pass's pattern searches from one call to the next on the same frames."""
    import rtlsdr_ft8d_amd as ft8
    import ft8_spec_messages as sm
    import ft8_spec_multipass as mp
    mag, cands, counts, status = sm.oracle_stages(oracle, iq, max_candidates, min_score, nthreads, iters)
    B = mag.shape[0]
    out, n = sm.collect(mag, cands, counts, status, min_score=min_score,
                        msgs=np.zeros((B, mp.MAX_MESSAGES), ft8.MESSAGE_DTYPE) if msgs is None else msgs)
    base = sm.noise_baseline(mag)
    nbs = np.zeros((B, passes, 2), np.int32)
    flat = nbs.reshape(B, 2 * passes)

    def osd_stage(W, c, k, s, a, cache=None):
        if order < 0:
            return
        so, info = osd_candidates(oracle, W, c, k, s, order, max_hard_errors, searches=cache)
        before = n[a].copy()
        o2, n2 = mp.append(W, base[a], c, k, so, out[a], n[a], min_score=min_score)
        for j in range(len(a)):
            for r in range(int(before[j]), int(n2[j])):
                o2[j, r]["pad"][0] = info[j, int(o2[j, r]["cand_index"])]["nhard"]
        out[a], n[a] = o2, n2

    everyone = np.arange(B)
    flat[:, 0:] = n[:, None]
    osd_stage(mag, cands, counts, status, everyone, searches)
    flat[:, 1:] = n[:, None]
    W = np.array(mag, copy=True)
    prev = np.zeros(B, np.int32)
    for p in range(1, passes):
        active = [f for f in range(B) if prev[f] < n[f] < mp.MAX_MESSAGES]
        prev_next = n.copy()
        if not active:
            break
        a = np.array(active)
        W[a] = mp.mask(W[a], base[a], out[a], prev[a], n[a])
        c2, k2 = oracle.find_sync_batch(W[a], max_candidates, min_score, nthreads=nthreads)
        s2 = oracle.decode_candidates_batch(W[a], c2, k2, iters=iters, nthreads=nthreads)
        prev = prev_next
        o2, n2 = mp.append(W[a], base[a], c2, k2, s2, out[a], n[a], min_score=min_score)
        out[a], n[a] = o2, n2
        flat[:, 2 * p:] = n[:, None]
        osd_stage(W[a], c2, k2, s2, a)
        flat[:, 2 * p + 1:] = n[:, None]
    return out, n, nbs
