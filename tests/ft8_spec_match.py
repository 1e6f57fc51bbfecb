"""CPU restatement of the expected messages (ft8gpu_match_candidates, ft8gpu_expect_update,
ft8gpu_decode_messages_expected; include/ft8gpu.h "expected messages", DESIGN.md "Expected messages") in numpy.  It is fed
by the oracle's normalised soft bits (oracle_lib.llr) and takes the generator and the CRC from tests/ft8_spec_osd.py.
Integers and float32 comparisons only, so the device compares byte for byte.

Matching.  A candidate whose status record has ok == 0 and ldpc_errors != 0 is compared with the receiver's table:
  h[i] = llr[i] > 0;  w[i] = 255 if |llr[i]| >= 32 else int(|llr[i]| * 8)          (OSD's); a non-finite llr: result 6
  live entries: used != 0 and not (max_age != 0 and uint32(slot - stamp) > max_age); none: result 0
  c_j = payload bits 0..76, their CRC-14, the 83 parities; nhard_j = |c_j ^ h|, metric_j = sum of w over c_j ^ h
  best = smallest (metric, table index); judged: 5 all-zero payload, 2 nhard > max_hard_errors, 4 unpack77 < 0, 1 accepted
Info record: uint8 result, uint8 nhard, uint16 index, int32 metric.

Update.  insert(P, kind): the first used entry with the same 77 bits gets stamp = slot, kind &= kind; else entry[cursor % 512]
= (P with bits 77..79 zero, 1, kind, slot), cursor = cursor % 512 + 1.  A record inserts its payload as kind 0 and, with
derive, a type 1 message with two standard calls in clear inserts calls-swapped RRR / RR73 / 73 as kind 1."""
import numpy as np

import ft8_spec_osd as so

ENTRIES = 512
MAX_MESSAGES = 50
NTOKENS, MAX22 = 2063592, 4194304
ENTRY_DTYPE = np.dtype([("payload", "u1", (10,)), ("used", "u1"), ("kind", "u1"), ("stamp", "<u4")])
STATE_DTYPE = np.dtype([("entry", ENTRY_DTYPE, (ENTRIES,)), ("cursor", "<u4"), ("slot", "<u4"), ("pad", "<u4", (2,))])
INFO_DTYPE = np.dtype([("result", "u1"), ("nhard", "u1"), ("index", "<u2"), ("metric", "<i4")])
assert ENTRY_DTYPE.itemsize == 16 and STATE_DTYPE.itemsize == 8208 and INFO_DTYPE.itemsize == 8
DERIVED_GRIDS = (32402, 32403, 32404)                    # RRR, RR73, 73


def new_state(n=1):
    return np.zeros(n, STATE_DTYPE)


# ---- codewords -----------------------------------------------------------------------------------------------------------

_cw_cache = {}


def payload77(payload):
    """the 10 payload bytes with bits 77..79 cleared, as bytes"""
    p = bytearray(bytes(payload)[:10])
    p[9] &= 0xF8
    return bytes(p)


def codeword(payload):
    """uint8 [174]: the 77 bits, the CRC-14 ft8_lib's encoder appends, the 83 generator parities"""
    key = payload77(payload)
    cw = _cw_cache.get(key)
    if cw is None:
        bits = np.unpackbits(np.frombuffer(key, np.uint8))[:77]
        crc = so.crc14(bits)
        m = np.concatenate([bits, [(crc >> (13 - i)) & 1 for i in range(14)]]).astype(np.int64)
        cw = ((m @ so.generator_matrix().astype(np.int64)) & 1).astype(np.uint8)
        cw.setflags(write=False)
        _cw_cache[key] = cw
    return cw


def live_entries(st, max_age):
    """table indices of the live entries of one state at its slot"""
    e = st["entry"]
    age = (np.uint32(st["slot"]) - e["stamp"].astype(np.uint32)).astype(np.uint32)      # wraps modulo 2^32
    expired = (age > np.uint32(max_age)) if max_age != 0 else np.zeros(ENTRIES, bool)
    return np.flatnonzero((e["used"] != 0) & ~expired)


def table_codewords(st, max_age):
    """(indices [L], codewords uint8 [L][174]) of the live entries"""
    idx = live_entries(st, max_age)
    if idx.size == 0:
        return idx, np.zeros((0, so.N), np.uint8)
    return idx, np.stack([codeword(st["entry"]["payload"][j].tobytes()) for j in idx])


def best_entry(llr, idx, C):
    """(metric, table index, nhard, codeword) of the best live entry: the smallest (metric, index)"""
    h, w = so.hard_and_weights(llr)
    D = C ^ h[None, :]
    metric = D.astype(np.int64) @ w.astype(np.int64)
    k = int(np.lexsort((idx, metric))[0])
    return int(metric[k]), int(idx[k]), int(D[k].sum()), C[k]


def judge(oracle, cw, nhard, max_hard_errors):
    """(result, crc, unpack status, text): 5 all-zero payload, 2 too many hard errors, 4 unpack77 refuses, 1 accepted"""
    code, ext, calc, rc, text = so.judge(oracle, cw, nhard, max_hard_errors)
    assert code != 3 and ext == calc                     # the codeword carries the encoder's own CRC
    return code, ext, rc, text


def match_candidates(oracle, mag, cands, counts, status_in, states, max_age, max_hard_errors, status_out=None, info=None):
    """ft8gpu_match_candidates: mag [B][94208], cands [B][cap], counts [B], status_in uint8 [B][cap][48] (or STATUS_DTYPE),
    states STATE_DTYPE [B] -> (status_out uint8 [B][cap][48], info INFO_DTYPE [B][cap]).  Records at and behind counts[f]
    keep what status_out / info held (zeros when None)."""
    import rtlsdr_ft8d_amd as ft8
    mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, 94208)
    B = mag.shape[0]
    sin = np.ascontiguousarray(status_in).view(np.uint8).reshape(B, -1, 48)
    cap = sin.shape[1]
    out = np.zeros((B, cap, 48), np.uint8) if status_out is None else np.array(status_out, copy=True).view(np.uint8).reshape(B, cap, 48)
    inf = np.zeros((B, cap), INFO_DTYPE) if info is None else np.array(info, copy=True).view(INFO_DTYPE).reshape(B, cap)
    st = sin.view(ft8.STATUS_DTYPE).reshape(B, cap)
    states = np.asarray(states).view(STATE_DTYPE).reshape(B)
    for f in range(B):
        table = None
        for i in range(int(counts[f])):
            out[f, i] = sin[f, i]
            inf[f, i] = np.zeros(1, INFO_DTYPE)[0]
            if st[f, i]["ok"] != 0 or st[f, i]["ldpc_errors"] == 0:
                continue
            llr = oracle.llr(mag[f], cands[f, i])
            if not np.isfinite(llr).all():
                inf[f, i]["result"] = 6
                continue
            if table is None:
                table = table_codewords(states[f], max_age)
            idx, C = table
            if idx.size == 0:
                continue
            metric, index, nhard, cw = best_entry(llr, idx, C)
            code, crc, rc, text = judge(oracle, cw, nhard, max_hard_errors)
            inf[f, i] = (code, nhard, index, metric)
            if code == 1:
                rec = np.zeros(1, ft8.STATUS_DTYPE)[0]
                rec["ldpc_errors"] = 0
                rec["iters"] = st[f, i]["iters"]
                rec["crc_extracted"], rec["crc_calculated"] = crc, crc
                rec["unpack_status"], rec["ok"] = rc, 1
                rec["a91"] = so.a91_of(cw)
                rec["text"] = text
                out[f, i] = np.frombuffer(rec.tobytes(), np.uint8)
    return out, inf


# ---- the update rule -------------------------------------------------------------------------------------------------------

def insert(st, payload, kind):
    """insert(P, kind) into one state (a STATE_DTYPE scalar or 0-d view), in place"""
    p = payload77(payload)
    e = st["entry"]
    pay = e["payload"]
    same = (e["used"] != 0) & (pay[:, :9] == np.frombuffer(p[:9], np.uint8)).all(axis=1) & ((pay[:, 9] & 0xF8) == p[9])
    hit = np.flatnonzero(same)
    if hit.size:
        j = int(hit[0])
        e["stamp"][j] = st["slot"]
        e["kind"][j] &= kind
        return
    at = int(st["cursor"]) % ENTRIES
    e["payload"][at] = np.frombuffer(p, np.uint8)
    e["used"][at], e["kind"][at], e["stamp"][at] = 1, kind, st["slot"]
    st["cursor"] = at + 1


def derived(payload):
    """the payloads a record derives: [] unless type 1 with two standard calls in clear; else RRR, RR73, 73 with the 29-bit call
    fields swapped, ir = 0, i3 = 1"""
    v = int.from_bytes(payload77(payload), "big") >> 3                      # the 77 bits as a number, bit 0 the most significant
    i3 = v & 7
    n29a, n29b = v >> 48, (v >> 19) & 0x1FFFFFFF
    if i3 != 1 or (n29a >> 1) < NTOKENS + MAX22 or (n29b >> 1) < NTOKENS + MAX22:
        return []
    return [(((((n29b << 29 | n29a) << 1) << 15 | g) << 3 | 1) << 3).to_bytes(10, "big") for g in DERIVED_GRIDS]


def update(msgs, n_msgs, state=None, derive=True):
    """ft8gpu_expect_update: msgs [R][S][50] (any record dtype with a field "a91"), n_msgs [R][S] -> the exit state [R]"""
    n_msgs = np.asarray(n_msgs)
    R, S = n_msgs.shape
    state = new_state(R) if state is None else np.array(state, STATE_DTYPE, copy=True, ndmin=1)
    for r in range(R):
        st = state[r:r + 1].reshape(())
        for s in range(S):
            for k in range(min(max(int(n_msgs[r, s]), 0), MAX_MESSAGES)):
                p = msgs[r, s, k]["a91"][:10].tobytes()
                insert(st, p, 0)
                if derive:
                    for d in derived(p):
                        insert(st, d, 1)
            st["slot"] = np.uint32((int(st["slot"]) + 1) & 0xFFFFFFFF)
    return state


# ---- the whole path ----------------------------------------------------------------------------------------------------------

def decode_expected(oracle, iq, state=None, max_hard_errors=49, max_age=0, derive=True, msgs=None, max_candidates=120, min_score=10,
                    nthreads=8, iters=20, stages=None):
    """ft8gpu_decode_messages_expected for iq [R][S][2][48000] -> (msgs [R][S][50], n [R][S], n_by_stage [R][S][2], exit state
    [R]): the records of ft8gpu_decode_messages, matching in place on the BP status records against the receiver's state as
    the earlier slots left it, the append step on what it accepted (pad[2] = 1), the update rule over the final records.
    stages: the oracle's (mag, cands, counts, status) of the R * S frames, to spare recomputing them."""
    import rtlsdr_ft8d_amd as ft8
    import ft8_spec_messages as sm
    import ft8_spec_multipass as mp
    iq = np.asarray(iq, np.float32)
    R, S = iq.shape[:2]
    mag, cands, counts, status = stages if stages is not None else \
        sm.oracle_stages(oracle, iq.reshape(R * S, 2, -1), max_candidates, min_score, nthreads, iters)
    out, n = sm.collect(mag, cands, counts, status, min_score=min_score,
                        msgs=np.zeros((R * S, MAX_MESSAGES), ft8.MESSAGE_DTYPE) if msgs is None else np.array(msgs).reshape(R * S, MAX_MESSAGES))
    base = sm.noise_baseline(mag)
    state = new_state(R) if state is None else np.array(state, STATE_DTYPE, copy=True, ndmin=1)
    nbs = np.zeros((R * S, 2), np.int32)
    nbs[:, 0] = n
    for s in range(S):
        a = np.arange(R) * S + s                                           # the frames of this slot, one per receiver
        so_, _info = match_candidates(oracle, mag[a], cands[a], counts[a], status[a], state, max_age, max_hard_errors)
        o2, n2 = mp.append(mag[a], base[a], cands[a], counts[a], so_, out[a], n[a], min_score=min_score)
        for j in range(R):
            for r in range(int(n[a[j]]), int(n2[j])):
                o2[j, r]["pad"][2] = 1
        out[a], n[a] = o2, n2
        state = update(o2.reshape(R, 1, MAX_MESSAGES), n2.reshape(R, 1), state, derive)
    nbs[:, 1] = n
    return out.reshape(R, S, MAX_MESSAGES), n.reshape(R, S), nbs.reshape(R, S, 2), state
