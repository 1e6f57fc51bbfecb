"""CPU restatement of the call hints (ft8gpu_hint_candidates, ft8gpu_hint_update, ft8gpu_decode_messages_hinted; DESIGN.md
"Call hints"; include/ft8gpu.h has the rule in full).  Integers for the table and the preselection; a tried entry is judged by
tests/ft8_spec_ap.py's per-hypothesis rule on the oracle's soft bits, so the device compares byte for byte.

State: 512 entries { a, b, stamp, kind, used, phase, pad }, cursor, slot, pad[2].  kind 1 = "A ? ?", 2 = "? B ?", 3 = "A B ?";
a / b are 29-bit fields (n28 << 1 | flag), read & 0x1FFFFFFF; phase is read & 1.
  live: used != 0, kind in {1, 2, 3}, not (max_age != 0 and uint32(slot - stamp) > max_age), not (use_phase and (slot ^ phase) & 1)
  hypothesis: bits 74..76 masked with 001; kind & 1 masks 0..28 with a; kind & 2 masks 29..57 with b (nmask 32 or 61)
  preselection on h = llr > 0: nbad = masked positions where h differs; pass when nbad * 64 <= max_bad_per_64 * nmask; order by
  (nbad * 61 if nmask == 32 else nbad * 32, nmask == 32, index); the first `tries` are tried, the first accepted wins
Update: type 1 records only; F1 = bits 0..28, F2 = bits 29..57, p = slot & 1; F2 clear: insert(2, 0, F2, p), insert(1, F2, 0, p ^ 1);
F1 and F2 clear: insert(3, F1, F2, p), insert(3, F2, F1, p ^ 1); slot += 1 after each slot."""
import numpy as np

import ft8_spec_ap as sa
import ft8_spec_osd as so

ENTRIES = 512
MAX_MESSAGES = 50
MAX_TRIES = 4
F29 = 0x1FFFFFFF
NTOKENS, MAX22 = 2063592, 4194304
CLEAR = NTOKENS + MAX22
ENTRY_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("stamp", "<u4"), ("kind", "u1"), ("used", "u1"), ("phase", "u1"), ("pad", "u1")])
STATE_DTYPE = np.dtype([("entry", ENTRY_DTYPE, (ENTRIES,)), ("cursor", "<u4"), ("slot", "<u4"), ("pad", "<u4", (2,))])
INFO_DTYPE = np.dtype([("result", "u1"), ("nhard", "u1"), ("ntried", "u1"), ("iters", "u1"), ("results", "u1", (4,)), ("index", "<u2", (4,))])
assert ENTRY_DTYPE.itemsize == 16 and STATE_DTYPE.itemsize == 8208 and INFO_DTYPE.itemsize == 16


def new_state(n=1):
    return np.zeros(n, STATE_DTYPE)


def _bits29(v):
    return [(int(v) >> (28 - i)) & 1 for i in range(29)]


def hypothesis(entry):
    """ft8gpu_hint_hypothesis: the sa.HYP_DTYPE record of an entry, None if its kind is not 1, 2 or 3"""
    kind = int(entry["kind"])
    if kind not in (1, 2, 3):
        return None
    m = np.zeros(77, np.uint8)
    b = np.zeros(77, np.uint8)
    if kind & 1:
        m[0:29], b[0:29] = 1, _bits29(int(entry["a"]) & F29)
    if kind & 2:
        m[29:58], b[29:58] = 1, _bits29(int(entry["b"]) & F29)
    m[74:77] = 1
    b[76] = 1
    return sa.hypothesis(m, b)


def live_entries(st, max_age, use_phase):
    """bool [512]"""
    e = st["entry"]
    slot = np.uint32(st["slot"])
    live = (e["used"] != 0) & (e["kind"] >= 1) & (e["kind"] <= 3)
    if max_age:
        live &= ~((slot - e["stamp"]).astype(np.uint32) > np.uint32(max_age))
    if use_phase:
        live &= ((int(slot) ^ e["phase"].astype(np.uint32)) & 1) == 0
    return live


def preselect(h77, st, tries, max_bad_per_64, max_age, use_phase):
    """the table indices tried, in order: h77 = the hard decisions of payload positions 0..76 (0 / 1)"""
    h = np.asarray(h77, np.uint8)
    keys = []
    for j in np.flatnonzero(live_entries(st, max_age, use_phase)):
        hyp = hypothesis(st["entry"][j])
        m = np.unpackbits(hyp["mask"])[:77] != 0
        b = np.unpackbits(hyp["bits"])[:77]
        nmask, nbad = int(m.sum()), int((h[m] != b[m]).sum())
        assert nmask in (32, 61)
        if nbad * 64 <= max_bad_per_64 * nmask:
            keys.append((nbad * (61 if nmask == 32 else 32), nmask == 32, int(j)))
    return [k[2] for k in sorted(keys)[:tries]]


def resolve(oracle, llr, tried, indices, max_hard_errors):
    """the info record and, when an entry is accepted, (plain, ext, calc, rc, text): sa.resolve's walk over sa.attempts()' list"""
    info = np.zeros(1, INFO_DTYPE)[0]
    if tried is None:
        info["result"] = 6
        return info, None
    h = (np.asarray(llr, np.float32) > 0).astype(np.uint8)
    for k, (plain, errors, it, m, b) in enumerate(tried):
        code, nhard, ext, calc, rc, text = sa.judge(oracle, plain, errors, m, b, h, max_hard_errors)
        info["result"], info["nhard"], info["ntried"], info["iters"] = code, nhard, k + 1, min(it, 255)
        info["results"][k] = code
        info["index"][k] = indices[k]
        if code == 1:
            return info, (plain, ext, calc, rc, text)
    return info, None


def hint_candidates(oracle, mag, cands, counts, status_in, states, tries, max_bad_per_64, max_hard_errors, max_age=0, use_phase=True,
                    status_out=None, info=None, iters=20, cache=None):
    """ft8gpu_hint_candidates: mag [B][94208], cands [B][cap], counts [B], status_in uint8 [B][cap][48] (or STATUS_DTYPE), states
    STATE_DTYPE [B] -> (status_out uint8 [B][cap][48], info INFO_DTYPE [B][cap]).  Records at and behind counts[f] keep what
    status_out / info held (zeros when None).  cache: an optional dict, (f, i) -> llr and (f, i, hypothesis bytes) -> one attempt,
    valid for the same frames and iters."""
    import rtlsdr_ft8d_amd as ft8
    assert 1 <= tries <= MAX_TRIES and 0 <= max_bad_per_64 <= 64
    mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, 94208)
    B = mag.shape[0]
    sin = np.ascontiguousarray(status_in).view(np.uint8).reshape(B, -1, 48)
    cap = sin.shape[1]
    out = np.zeros((B, cap, 48), np.uint8) if status_out is None else np.array(status_out, copy=True).view(np.uint8).reshape(B, cap, 48)
    inf = np.zeros((B, cap), INFO_DTYPE) if info is None else np.array(info, copy=True).view(INFO_DTYPE).reshape(B, cap)
    st = sin.view(ft8.STATUS_DTYPE).reshape(B, cap)
    cache = {} if cache is None else cache
    for f in range(B):
        for i in range(int(counts[f])):
            out[f, i] = sin[f, i]
            inf[f, i] = np.zeros(1, INFO_DTYPE)[0]
            if st[f, i]["ok"] != 0 or st[f, i]["ldpc_errors"] == 0:
                continue
            if (f, i) not in cache:
                cache[(f, i)] = np.asarray(oracle.llr(mag[f], cands[f, i]), np.float32)
            llr = cache[(f, i)]
            if not np.isfinite(llr).all() or np.abs(llr).max() == 0:
                inf[f, i]["result"] = 6
                continue
            indices = preselect((llr[:77] > 0).astype(np.uint8), states[f], tries, max_bad_per_64, max_age, use_phase)
            if not indices:
                continue
            tried = []
            for j in indices:
                hyp = hypothesis(states[f]["entry"][j])
                key = (f, i, hyp.tobytes())
                if key not in cache:
                    cache[key] = sa.attempts(oracle, llr, [hyp], iters)[0]
                tried.append(cache[key])
            rec_info, win = resolve(oracle, llr, tried, indices, max_hard_errors)
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


def tried_hypotheses(state, info_rec):
    """the sa.HYP_DTYPE records of the entries an info record says were tried, in order"""
    return [hypothesis(state["entry"][int(info_rec["index"][k])]) for k in range(int(info_rec["ntried"]))]


# ---- the update rule -------------------------------------------------------------------------------------------------------

def insert(st, kind, a, b, phase):
    """insert(kind, a, b, phase) into one state (a STATE_DTYPE 0-d view), in place"""
    assert kind in (1, 2, 3)
    a, b, phase = int(a) & F29, int(b) & F29, int(phase) & 1
    e = st["entry"]
    same = (e["used"] != 0) & (e["kind"] == kind) & ((e["a"] & F29) == a) & ((e["b"] & F29) == b) & ((e["phase"] & 1) == phase)
    hit = np.flatnonzero(same)
    if hit.size:
        e["stamp"][int(hit[0])] = st["slot"]
        return
    at = int(st["cursor"]) % ENTRIES
    e["a"][at], e["b"][at], e["stamp"][at] = a, b, st["slot"]
    e["kind"][at], e["used"][at], e["phase"][at], e["pad"][at] = kind, 1, phase, 0
    st["cursor"] = at + 1


def fields(a91):
    """(i3, F1, F2) of a record's a91: bits 74..76, 0..28 and 29..57 as numbers"""
    v = int.from_bytes(bytes(bytearray(a91[:10])), "big") >> 3              # the 77 bits as a number, bit 0 the most significant
    return v & 7, v >> 48, (v >> 19) & F29


def inserts_of(a91, p):
    """the inserts a record causes at slot parity p: [(kind, a, b, phase)]"""
    i3, f1, f2 = fields(a91)
    if i3 != 1 or (f2 >> 1) < CLEAR:
        return []
    out = [(2, 0, f2, p), (1, f2, 0, p ^ 1)]
    if (f1 >> 1) >= CLEAR:
        out += [(3, f1, f2, p), (3, f2, f1, p ^ 1)]
    return out


def update(msgs, n_msgs, state=None):
    """ft8gpu_hint_update: msgs [R][S][50] (any record dtype with a field "a91"), n_msgs [R][S] -> the exit state [R]"""
    n_msgs = np.asarray(n_msgs)
    R, S = n_msgs.shape
    state = new_state(R) if state is None else np.array(state, STATE_DTYPE, copy=True, ndmin=1)
    for r in range(R):
        st = state[r:r + 1].reshape(())
        for s in range(S):
            p = int(st["slot"]) & 1
            for k in range(min(max(int(n_msgs[r, s]), 0), MAX_MESSAGES)):
                for ins in inserts_of(msgs[r, s, k]["a91"], p):
                    insert(st, *ins)
            st["slot"] = np.uint32((int(st["slot"]) + 1) & 0xFFFFFFFF)
    return state


# ---- the whole path ----------------------------------------------------------------------------------------------------------

def decode_hinted(oracle, iq, tries, max_bad_per_64, max_hard_errors, state=None, max_age=0, use_phase=True, msgs=None,
                  max_candidates=120, min_score=10, nthreads=8, iters=20, stages=None):
    """ft8gpu_decode_messages_hinted for iq [R][S][2][48000] -> (msgs [R][S][50], n [R][S], n_by_stage [R][S][2], exit state
    [R]): the records of ft8gpu_decode_messages, the hint stage in place on the BP status records against the receiver's state
    as the earlier slots left it, the append step on what it accepted (pad[2] = 3), the update rule over the final records.
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
        so_, _info = hint_candidates(oracle, mag[a], cands[a], counts[a], status[a], state, tries, max_bad_per_64, max_hard_errors,
                                     max_age, use_phase, iters=iters)
        o2, n2 = mp.append(mag[a], base[a], cands[a], counts[a], so_, out[a], n[a], min_score=min_score)
        for j in range(R):
            for r in range(int(n[a[j]]), int(n2[j])):
                o2[j, r]["pad"][2] = 3
        out[a], n[a] = o2, n2
        state = update(o2.reshape(R, 1, MAX_MESSAGES), n2.reshape(R, 1), state)
    nbs[:, 1] = n
    return out.reshape(R, S, MAX_MESSAGES), n.reshape(R, S), nbs.reshape(R, S, 2), state
