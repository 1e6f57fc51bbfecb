"""CPU restatement of a-priori decoding (ft8gpu_ap_candidates, ft8gpu_decode_messages_ap; DESIGN.md "A-priori decoding").
It is fed by the oracle's normalised soft bits (oracle_lib.llr) and runs the oracle's bp_decode; crc14 and unpack77 judge the
word.  float32 values and integers only, so the device compares byte for byte.

The rule.  A hypothesis is 77 payload bits with a mask (a91 numbering, MSB first; codeword positions 0..76 are the payload).
A candidate whose status record has ok == 0 and ldpc_errors != 0 is decoded again:
  llr = the normalised soft bits BP starts from; h[i] = llr[i] > 0; apmag = max |llr[i]|
  a non-finite llr[i] or apmag == 0: nothing is tried, result 6
  per hypothesis k, in table order: llr_k = +-apmag on the masked positions (by the hypothesis's bit), llr elsewhere;
  (plain, errors, iters) = bp_decode(llr_k, ldpc_iters); nhard = the unmasked positions where plain differs from h
  first failing check: 7 errors != 0, 8 plain differs from the hypothesis on a masked position, 5 plain all-zero,
  2 nhard > max_hard_errors, 3 CRC-14 mismatch, 4 unpack77 < 0, else 1 = accepted; the first accepted hypothesis wins
(bp_decode leaves at an all-zero word BEFORE it checks it and reports the errors seen so far, which are not 0: such a word
is result 7, and 5 is unreachable with this decoder.)
Info record: uint8 result, nhard, hyp, iters (255 for more), results[4]."""
import numpy as np

import ft8_spec_osd as so

N, K = so.N, so.K
MAX_HYPOTHESES = 4
INFO_DTYPE = np.dtype([("result", "u1"), ("nhard", "u1"), ("hyp", "u1"), ("iters", "u1"), ("results", "u1", (4,))])
HYP_DTYPE = np.dtype([("mask", "u1", (10,)), ("bits", "u1", (10,))])
assert INFO_DTYPE.itemsize == 8 and HYP_DTYPE.itemsize == 20


def hypothesis(mask77, bits77):
    """HYP_DTYPE record from two 0/1 vectors of 77"""
    m = np.zeros(80, np.uint8)
    b = np.zeros(80, np.uint8)
    m[:77] = np.asarray(mask77, np.uint8)[:77]
    b[:77] = np.asarray(bits77, np.uint8)[:77] & m[:77]
    h = np.zeros(1, HYP_DTYPE)
    h["mask"], h["bits"] = np.packbits(m), np.packbits(b)
    return h[0]


def mask_and_bits(hyp):
    """(mask bool [174], bits uint8 [174]) over the codeword positions"""
    m = np.zeros(N, bool)
    b = np.zeros(N, np.uint8)
    m[:77] = np.unpackbits(np.asarray(hyp["mask"], np.uint8))[:77] != 0
    b[:77] = np.unpackbits(np.asarray(hyp["bits"], np.uint8))[:77]
    return m, b


def validate(hyps):
    """the refusals of the entry: 1..4 hypotheses, bits inside the mask, nothing past bit 76, at least one masked bit"""
    if not 1 <= len(hyps) <= MAX_HYPOTHESES:
        return False
    for h in hyps:
        m, b = np.asarray(h["mask"], np.uint8), np.asarray(h["bits"], np.uint8)
        if (b & ~m).any() or (m[9] & 7) or not m.any():
            return False
    return True


def cq_hypothesis():
    """"CQ ? ?": the 28-bit first call field = 2, its /R flag = 0 (bits 0..28) and i3 = 1 (bits 74..76)"""
    m = np.zeros(77, np.uint8)
    b = np.zeros(77, np.uint8)
    m[0:29] = 1
    m[74:77] = 1
    b[26] = 1                                            # value 2 in bits 0..27
    b[76] = 1                                            # i3 = 1
    return hypothesis(m, b)


def from_text(pattern):
    """ft8gpu_ap_from_text restated with tests/ft8_spec_pack.py: "FIELD1 CALL2 THIRD" with `?` for unknown tokens, FIELD1 may
    be "CQ nnn" / "CQ aaaa"; well-formed patterns only (the refusals are the library's)"""
    import ft8_spec_pack as sp
    tok = pattern.split()
    if len(tok) == 4:
        assert tok[0] == "CQ"
        tok = [tok[0] + " " + tok[1]] + tok[2:]
    assert len(tok) == 3
    known = [t != "?" for t in tok]
    payload = sp.pack_standard(tok[0] if known[0] else "K1ABC", tok[1] if known[1] else "K1ABC", tok[2] if known[2] else "")
    m = np.zeros(77, np.uint8)
    for on, (a, b) in zip(known + [True], ((0, 29), (29, 58), (58, 74), (74, 77))):
        if on:
            m[a:b] = 1
    return hypothesis(m, np.unpackbits(np.frombuffer(payload, np.uint8))[:77])


def judge(oracle, plain, errors, mask, bits, h, max_hard_errors):
    """(result code, nhard, crc_extracted, crc_calculated, unpack status, text) of what bp_decode left"""
    plain = np.asarray(plain, np.uint8)
    nhard = int(((plain != h) & ~mask).sum())
    if errors != 0:
        return 7, nhard, 0, 0, 0, b""
    if (plain[mask] != bits[mask]).any():
        return 8, nhard, 0, 0, 0, b""
    if not plain.any():
        return 5, nhard, 0, 0, 0, b""
    if nhard > max_hard_errors:
        return 2, nhard, 0, 0, 0, b""
    ext = int("".join(map(str, plain[77:91])), 2)
    calc = so.crc14(plain[:77])
    if ext != calc:
        return 3, nhard, ext, calc, 0, b""
    a77 = so.a91_of(plain).copy()
    a77[9] &= 0xF8
    a77[10] = a77[11] = 0
    rc, text = oracle.unpack77(a77[:10].tobytes())
    if rc < 0:
        return 4, nhard, ext, calc, rc, b""
    return 1, nhard, ext, calc, rc, text.encode()


def attempts(oracle, llr, hyps, iters=20, bp=None):
    """bp_decode under every hypothesis -> None (result 6) or a list of (plain, errors, iterations, mask, bits) per
    hypothesis, independent of the gate and of which hypothesis wins.  bp: another bp_decode(llr, iters) ->
    (plain, errors, iterations), e.g. the numpy writing of tests/ft8_spec_decode.py"""
    llr = np.asarray(llr, np.float32)
    if not np.isfinite(llr).all():
        return None
    apmag = np.abs(llr).max()
    if apmag == 0:
        return None
    out = []
    for hyp in hyps:
        m, b = mask_and_bits(hyp)
        x = np.where(m, np.where(b == 1, apmag, -apmag), llr).astype(np.float32)
        plain, errors, it = (bp or oracle.bp_decode)(x, iters)
        out.append((np.array(plain, np.uint8), int(errors), int(it), m, b))
    return out


def numpy_bp():
    """bp_decode in numpy (tests/ft8_spec_decode.py), in the argument order of oracle_lib.bp_decode"""
    import ft8_spec_decode as sd
    bp = sd.BP()

    def run(llr, iters):
        errors, it, plain = bp.decode(llr, iters)
        return plain, errors, it
    return run


def resolve(oracle, llr, tried, max_hard_errors):
    """the info record and, when a hypothesis is accepted, (plain, ext, calc, rc, text) from attempts()' list"""
    info = np.zeros(1, INFO_DTYPE)[0]
    if tried is None:
        info["result"] = 6
        return info, None
    h = (np.asarray(llr, np.float32) > 0).astype(np.uint8)
    for k, (plain, errors, it, m, b) in enumerate(tried):
        code, nhard, ext, calc, rc, text = judge(oracle, plain, errors, m, b, h, max_hard_errors)
        info["result"], info["nhard"], info["hyp"], info["iters"] = code, nhard, k, min(it, 255)
        info["results"][k] = code
        if code == 1:
            return info, (plain, ext, calc, rc, text)
    return info, None


def ap_candidates(oracle, mag, cands, counts, status_in, hyps, max_hard_errors, status_out=None, info=None, iters=20, cache=None,
                  bp=None):
    """ft8gpu_ap_candidates: mag [B][94208], cands [B][cap], counts [B], status_in uint8 [B][cap][48] (or STATUS_DTYPE)
    -> (status_out uint8 [B][cap][48], info INFO_DTYPE [B][cap]).  Records at and behind counts[f] keep what status_out /
    info held (zeros when None).  cache: an optional dict (f, i) -> (llr, attempts), filled and reused (same hyps, iters)."""
    import rtlsdr_ft8d_amd as ft8
    assert validate(hyps)
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
            if cache is not None and (f, i) in cache:
                llr, tried = cache[(f, i)]
            else:
                llr = oracle.llr(mag[f], cands[f, i])
                tried = attempts(oracle, llr, hyps, iters, bp)
                if cache is not None:
                    cache[(f, i)] = (llr, tried)
            rec_info, win = resolve(oracle, llr, tried, max_hard_errors)
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


def decode_ap(oracle, iq, passes, hyps, ap_max_hard_errors, osd_order, osd_max_hard_errors, max_candidates=120, min_score=10,
              nthreads=8, msgs=None, iters=20, searches=None, cache=None):
    """ft8gpu_decode_messages_ap for B frames [B][2][48000] -> (msgs [B][50], n [B], n_by_stage [B][passes][3]): the pass loop
    of tests/ft8_spec_multipass.py with AP and then OSD behind every pass, both in place on the pass's status records, each
    followed by the append step; pad[1] of a record AP gained = 1 + hyp, pad[0] of one OSD gained = nhard.  hyps empty: no
    AP; osd_order -1: no OSD.  searches / cache: dicts that carry the first pass's OSD pattern searches / AP attempts from one call
    to the next on the same frames (same hyps and iters)."""
    import rtlsdr_ft8d_amd as ft8
    import ft8_spec_messages as sm
    import ft8_spec_multipass as mp
    mag, cands, counts, status = sm.oracle_stages(oracle, iq, max_candidates, min_score, nthreads, iters)
    B = mag.shape[0]
    out, n = sm.collect(mag, cands, counts, status, min_score=min_score,
                        msgs=np.zeros((B, mp.MAX_MESSAGES), ft8.MESSAGE_DTYPE) if msgs is None else msgs)
    base = sm.noise_baseline(mag)
    nbs = np.zeros((B, passes, 3), np.int32)
    flat = nbs.reshape(B, 3 * passes)

    def gained(W, c, k, s, a, info, pad, field, plus):
        before = n[a].copy()
        o2, n2 = mp.append(W, base[a], c, k, s, out[a], n[a], min_score=min_score)
        for j in range(len(a)):
            for r in range(int(before[j]), int(n2[j])):
                o2[j, r]["pad"][pad] = int(info[j, int(o2[j, r]["cand_index"])][field]) + plus
        out[a], n[a] = o2, n2

    def stages(W, c, k, s, a, col, searches=None, cache=None):
        flat[:, col:] = n[:, None]
        if len(hyps):
            s, info = ap_candidates(oracle, W, c, k, s, hyps, ap_max_hard_errors, iters=iters, cache=cache)
            gained(W, c, k, s, a, info, 1, "hyp", 1)
            flat[:, col + 1:] = n[:, None]
        if osd_order >= 0:
            s, info = so.osd_candidates(oracle, W, c, k, s, osd_order, osd_max_hard_errors, searches=searches)
            gained(W, c, k, s, a, info, 0, "nhard", 0)
        flat[:, col + 2:] = n[:, None]

    stages(mag, cands, counts, status, np.arange(B), 0, searches, cache)
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
        stages(W[a], c2, k2, s2, a, 3 * p)
    return out, n, nbs
