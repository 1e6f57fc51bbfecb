"""CPU restatement of the soft-bit memory (ft8gpu_combine_candidates, ft8gpu_softmem_update,
ft8gpu_decode_messages_combined; include/ft8gpu.h "soft-bit memory", DESIGN.md "Soft-bit memory") in numpy.  It is fed by the
oracle's normalised soft bits (oracle_lib.llr), normalises a sum with tests/ft8_spec_decode.normalize_logl (float32
accumulators in index order), runs bp_decode -- the numpy writing of tests/ft8_spec_decode.py by default, the oracle's C
writing where a caller asks for speed; tests/test_combine_cpu.py holds the two against each other on the guard cases -- and
takes the CRC and the record of a BP success from tests/ft8_spec_osd.py.  Every float operation is one float32 operation, so
the device compares byte for byte.

Combining.  A candidate whose status record has ok == 0 and ldpc_errors != 0:
  own = the LDPC kernel's soft bits; non-finite: result 6
  T = 2 * time_offset + time_sub, F = 2 * freq_offset + freq_sub; partners = live entries (used != 0, not expired at the
  state's slot) with |T - Te| <= 1 and |F - Fe| <= 1; none: result 0
  nagree = #{i < 174: (own[i] > 0) == (entry.llr[i] > 0)}; best = largest nagree, then smaller |dT| + |dF|, then smaller index
  nagree < min_agree: result 8;  s = entry.llr + own, x = normalize_logl(s); non-finite x: result 6
  bp_decode(x, iters): 7 no codeword, 5 all-zero, 3 CRC, 4 unpack77 < 0, 1 accepted
Info record: uint8 result, nagree, index, count, nhard, pad[3].

Update, one slot: in candidate order the first store_per_slot candidates whose final record still has ok == 0 and ldpc_errors
!= 0 and whose own is finite; info.result in (3, 4, 5, 7) stores entry[info.index].llr + own with count min(255, info.count +
1), every other one own with count 1; to entry[cursor % 128], cursor = cursor % 128 + 1; sums from the state at entry; slot
increments."""
import numpy as np

import ft8_spec_decode as sd
import ft8_spec_osd as so

F32 = np.float32
ENTRIES = 128
MAX_MESSAGES = 50
CAND_DTYPE = np.dtype([("score", "<i2"), ("time_offset", "<i2"), ("freq_offset", "<i2"), ("time_sub", "u1"), ("freq_sub", "u1")])
ENTRY_DTYPE = np.dtype([("cand", CAND_DTYPE), ("used", "u1"), ("count", "u1"), ("pad", "<u2"), ("stamp", "<u4"), ("llr", "<f4", (176,))])
STATE_DTYPE = np.dtype([("entry", ENTRY_DTYPE, (ENTRIES,)), ("cursor", "<u4"), ("slot", "<u4"), ("pad", "<u4", (2,))])
INFO_DTYPE = np.dtype([("result", "u1"), ("nagree", "u1"), ("index", "u1"), ("count", "u1"), ("nhard", "u1"), ("pad", "u1", (3,))])
assert ENTRY_DTYPE.itemsize == 720 and STATE_DTYPE.itemsize == 92176 and INFO_DTYPE.itemsize == 8
BP_RAN = (3, 4, 5, 7)


def new_state(n=1):
    return np.zeros(n, STATE_DTYPE)


_numpy_bp = None


def numpy_bp():
    """bp_decode(llr, iters) -> (plain, errors, iterations) in numpy (tests/ft8_spec_decode.py)"""
    global _numpy_bp
    if _numpy_bp is None:
        bp = sd.BP()

        def run(llr, iters):
            errors, it, plain = bp.decode(llr, iters)
            return plain, errors, it
        _numpy_bp = run
    return _numpy_bp


def position(c):
    return 2 * int(c["time_offset"]) + int(c["time_sub"]), 2 * int(c["freq_offset"]) + int(c["freq_sub"])


def live_entries(st, max_age):
    """indices of the live entries of one state at its slot"""
    e = st["entry"]
    age = (np.uint32(st["slot"]) - e["stamp"].astype(np.uint32)).astype(np.uint32)        # wraps modulo 2^32
    expired = (age > np.uint32(max_age)) if max_age != 0 else np.zeros(ENTRIES, bool)
    return np.flatnonzero((e["used"] != 0) & ~expired)


def best_partner(own, cand, st, max_age):
    """None, or (index, nagree, count) of the best partner of a candidate in one state"""
    T, F = position(cand)
    e = st["entry"]
    live = live_entries(st, max_age)
    c = e["cand"][live]
    dt = np.abs(T - (2 * c["time_offset"].astype(np.int64) + c["time_sub"]))
    df = np.abs(F - (2 * c["freq_offset"].astype(np.int64) + c["freq_sub"]))
    near = (dt <= 1) & (df <= 1)
    if not near.any():
        return None
    idx, dist = live[near], (dt + df)[near]
    with np.errstate(invalid="ignore"):
        nagree = ((own > 0)[None, :] == (e["llr"][idx][:, :174] > 0)).sum(axis=1)
    k = int(np.lexsort((idx, dist, -nagree))[0])                    # largest nagree, then smaller distance, then smaller index
    return int(idx[k]), int(nagree[k]), int(e["count"][idx[k]])


def summed(entry_llr, own):
    with np.errstate(all="ignore"):
        return (np.asarray(entry_llr[:174], F32) + np.asarray(own, F32)).astype(F32)


def normalized(s):
    with np.errstate(all="ignore"):
        return sd.normalize_logl(np.asarray(s, F32))


def judge(oracle, plain, errors, x):
    """(result, nhard, crc_extracted, crc_calculated, unpack status, text) of what bp_decode left on x"""
    plain = np.asarray(plain, np.uint8)
    if errors != 0:
        return 7, 0, 0, 0, 0, b""
    nhard = int((plain != (x > 0)).sum())
    if not plain.any():
        return 5, nhard, 0, 0, 0, b""
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


def combine_one(oracle, own, cand, st, max_age, min_agree, iters=20, bp=None):
    """one qualifying candidate -> (info record, None or (plain, ext, calc, rc, text))"""
    info = np.zeros(1, INFO_DTYPE)[0]
    if not np.isfinite(own).all():
        info["result"] = 6
        return info, None
    p = best_partner(own, cand, st, max_age)
    if p is None:
        return info, None
    index, nagree, count = p
    info["index"], info["nagree"], info["count"] = index, nagree, count
    if nagree < min_agree:
        info["result"] = 8
        return info, None
    x = normalized(summed(st["entry"]["llr"][index], own))
    if not np.isfinite(x).all():
        info["result"] = 6
        return info, None
    plain, errors, _it = (bp or numpy_bp())(x, iters)
    code, nhard, ext, calc, rc, text = judge(oracle, plain, errors, x)
    info["result"], info["nhard"] = code, nhard
    return info, ((plain, ext, calc, rc, text) if code == 1 else None)


def _qualifies(rec):
    return rec["ok"] == 0 and rec["ldpc_errors"] != 0


def combine_candidates(oracle, mag, cands, counts, status_in, states, max_age, min_agree, status_out=None, info=None, iters=20, bp=None):
    """ft8gpu_combine_candidates: mag [B][94208], cands [B][cap], counts [B], status_in uint8 [B][cap][48] (or STATUS_DTYPE),
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
        for i in range(int(counts[f])):
            out[f, i] = sin[f, i]
            inf[f, i] = np.zeros(1, INFO_DTYPE)[0]
            if not _qualifies(st[f, i]):
                continue
            own = oracle.llr(mag[f], cands[f, i])
            rec_info, win = combine_one(oracle, own, cands[f, i], states[f], max_age, min_agree, iters, bp)
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


def update(oracle, mag, cands, counts, status, info, states, store_per_slot):
    """ft8gpu_softmem_update, one slot: status = the final records, info as combine_candidates returned it -> the exit states [B]"""
    import rtlsdr_ft8d_amd as ft8
    mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, 94208)
    B = mag.shape[0]
    st = np.ascontiguousarray(status).view(np.uint8).reshape(B, -1, 48).view(ft8.STATUS_DTYPE).reshape(B, -1)
    info = np.asarray(info).view(INFO_DTYPE).reshape(B, -1)
    old = np.array(states, STATE_DTYPE, copy=True, ndmin=1)
    new = old.copy()
    for f in range(B):
        stored = 0
        cursor = int(old[f]["cursor"])
        for i in range(int(counts[f])):
            if stored >= store_per_slot:
                break
            if not _qualifies(st[f, i]):
                continue
            own = oracle.llr(mag[f], cands[f, i])
            if not np.isfinite(own).all():
                continue
            ran = int(info[f, i]["result"]) in BP_RAN
            llr = summed(old[f]["entry"]["llr"][int(info[f, i]["index"]) % ENTRIES], own) if ran else own
            at = cursor % ENTRIES
            e = new[f]["entry"]
            e["cand"][at] = cands[f, i]
            e["used"][at], e["pad"][at], e["stamp"][at] = 1, 0, old[f]["slot"]
            e["count"][at] = min(255, int(info[f, i]["count"]) + 1) if ran else 1
            e["llr"][at][:174] = llr
            e["llr"][at][174:] = 0
            cursor = at + 1
            stored += 1
        new[f]["cursor"] = cursor
        new[f]["slot"] = np.uint32((int(old[f]["slot"]) + 1) & 0xFFFFFFFF)
    return new


def decode_combined(oracle, iq, state=None, min_agree=0, max_age=0, store_per_slot=ENTRIES, msgs=None, max_candidates=120, min_score=10,
                    nthreads=8, iters=20, stages=None, bp=None, trace=None):
    """ft8gpu_decode_messages_combined for iq [R][S][2][48000] -> (msgs [R][S][50], n [R][S], n_by_stage [R][S][2], exit state
    [R]): the records of ft8gpu_decode_messages, combining in place on the BP status records against the receiver's state as
    the earlier slots left it, the append step on what it accepted (pad[2] = 2), the update rule on the final status records.
    stages: the oracle's (mag, cands, counts, status) of the R * S frames, to spare recomputing them.  trace: a list that
    receives (slot, info [R][cap]) per slot."""
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
        so_, info = combine_candidates(oracle, mag[a], cands[a], counts[a], status[a], state, max_age, min_agree, iters=iters, bp=bp)
        o2, n2 = mp.append(mag[a], base[a], cands[a], counts[a], so_, out[a], n[a], min_score=min_score)
        for j in range(R):
            for r in range(int(n[a[j]]), int(n2[j])):
                o2[j, r]["pad"][2] = 2
        out[a], n[a] = o2, n2
        state = update(oracle, mag[a], cands[a], counts[a], so_, info, state, store_per_slot)
        if trace is not None:
            trace.append((s, info))
    nbs[:, 1] = n
    return out.reshape(R, S, MAX_MESSAGES), n.reshape(R, S), nbs.reshape(R, S, 2), state
