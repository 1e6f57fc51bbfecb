"""The call hash table of a receiver, restated in plain Python from the rule in include/ft8gpu.h ("hashed call signs"), on
top of ft8_spec_pack.call_hash.  Tests only: the reference for every comparison of ft8gpu_resolve_calls, of the host helpers
and of the whole path.  Nothing here is shared with the kernel or the C helpers; the field positions are those of the
protocol's message tables (ft8_spec_pack.py packs them the other way round).

State per receiver: entry[4096] (call S11 left-justified in blanks, len, h22), stamp[4096], slot, pad[3].
Per slot, on the records [0, n), n = the frame's count clamped to [0, 50]:
  insert   records in order, first call field before the second: every call in clear -> entry[h22 >> 10], stamp = slot
  resolve  against the table after the slot's own inserts; an entry is expired when max_age != 0 and
           (slot - stamp) mod 2^32 > max_age
  then     slot += 1 (mod 2^32)"""
import numpy as np

import ft8_spec_pack as sp

NTOKENS, MAX22 = sp.NTOKENS, sp.MAX22
ENTRIES = 4096
MAX_MESSAGES = 50
ENTRY_DTYPE = np.dtype([("call", "S11"), ("len", "u1"), ("h22", "<u4")])
STATE_DTYPE = np.dtype([("entry", ENTRY_DTYPE, (ENTRIES,)), ("stamp", "<u4", (ENTRIES,)), ("slot", "<u4"), ("pad", "<u4", (3,))])
RESOLVED_DTYPE = np.dtype([("text", "S40"), ("n_hashed", "u1"), ("n_resolved", "u1"), ("n_inserted", "u1"),
                           ("resolved_mask", "u1"), ("pad", "u1", (4,))])
assert ENTRY_DTYPE.itemsize == 16 and STATE_DTYPE.itemsize == 81936 and RESOLVED_DTYPE.itemsize == 48


def new_state(n=1):
    return np.zeros(n, STATE_DTYPE)


def _field(v, start, width):
    """bits start .. start + width - 1 of the 77-bit payload v, bit 0 first"""
    return (v >> (77 - start - width)) & ((1 << width) - 1)


def standard_call(n28):
    """the call of a 28-bit code >= NTOKENS + MAX22, as the unpacker prints it (no suffix, no 3DA0 / 3X rewriting)"""
    n = n28 - NTOKENS - MAX22
    c = []
    for alphabet in (sp.A_LETTER_SP, sp.A_LETTER_SP, sp.A_LETTER_SP, sp.A_DIGIT, sp.A_ALNUM, sp.A_ALNUM_SP):
        c.append(alphabet[n % len(alphabet)])
        n //= len(alphabet)
    return "".join(reversed(c)).strip(" ")


def parse(a91):
    """(calls in clear, hashed fields) of a record by its a91: calls as text in field order, hashed fields as (bits, hash) in
    text order"""
    v = int.from_bytes(bytes(a91[:10]), "big") >> 3
    i3 = v & 7
    calls, hashed = [], []
    if i3 in (1, 2):
        for n28 in (_field(v, 0, 28), _field(v, 29, 28)):
            if n28 >= NTOKENS + MAX22:
                calls.append(standard_call(n28))
            elif n28 >= NTOKENS:
                hashed.append((22, n28 - NTOKENS))
    elif i3 == 4:
        n58 = _field(v, 12, 58)
        c = []
        for _ in range(11):
            c.append(sp.A_CALL11[n58 % 38])
            n58 //= 38
        call = "".join(reversed(c)).strip(" ")
        if call:
            calls.append(call)
        if _field(v, 73, 1) == 0:                       # icq
            hashed.append((12, _field(v, 0, 12)))
    return calls, hashed


def insert(st, call):
    """the insert phase's write of one call into one state (a STATE_DTYPE scalar or 0-d view)"""
    h22 = sp.call_hash(call, 22)
    i = h22 >> 10
    st["entry"][i] = (call.ljust(11).encode(), len(call), h22)
    st["stamp"][i] = st["slot"]


def lookup(st, bits, h, max_age):
    """the resolve phase's lookup: the call, or None"""
    i = h >> 10 if bits == 22 else h
    e = st["entry"][i]
    if e["len"] == 0:
        return None
    if max_age != 0 and ((int(st["slot"]) - int(st["stamp"][i])) & 0xFFFFFFFF) > max_age:
        return None
    if bits == 22 and int(e["h22"]) != h:
        return None
    return e.tobytes()[:min(int(e["len"]), 11)].decode("latin-1")


def resolved_text(text25, found):
    """text25: the 25 bytes of ft8gpu_message.text; found: per hashed field, in text order, the call or None"""
    s = bytes(text25).split(b"\0")[0]
    out, i, k = b"", 0, 0
    while i < len(s):
        if s[i:i + 5] == b"<...>":
            call = found[k] if k < min(len(found), 2) else None
            out += b"<...>" if call is None else b"<" + call.encode("latin-1") + b">"
            k += 1
            i += 5
        else:
            out += s[i:i + 1]
            i += 1
    return out[:39]


def step(st, msgs, n, max_age, resolved):
    """one slot of one receiver, in place: msgs / resolved [50], st one state"""
    n = min(max(int(n), 0), MAX_MESSAGES)
    parsed = [parse(msgs[r]["a91"]) for r in range(n)]
    for calls, _ in parsed:
        for call in calls:
            insert(st, call)
    for r, (calls, hashed) in enumerate(parsed):
        found = [lookup(st, bits, h, max_age) for bits, h in hashed]
        mask = sum(1 << k for k, c in enumerate(found) if c is not None)
        text = resolved_text(msgs[r].tobytes()[:25], found)
        resolved[r] = (text, len(hashed), bin(mask).count("1"), len(calls), mask, (0, 0, 0, 0))
    st["slot"] = (int(st["slot"]) + 1) & 0xFFFFFFFF


def resolve(msgs, n_msgs, state=None, max_age=0, resolved=None):
    """ft8gpu_resolve_calls: msgs [R][S][50] (any record dtype with a91 at field "a91" and the text in its first 25 bytes),
    n_msgs [R][S] -> (resolved [R][S][50], exit state [R]); the arguments stay as they are"""
    n_msgs = np.asarray(n_msgs)
    R, S = n_msgs.shape
    state = new_state(R) if state is None else np.array(state, STATE_DTYPE, copy=True, ndmin=1)
    resolved = np.zeros((R, S, MAX_MESSAGES), RESOLVED_DTYPE) if resolved is None else np.array(resolved, RESOLVED_DTYPE, copy=True)
    assert state.shape == (R,) and resolved.shape == (R, S, MAX_MESSAGES)
    for r in range(R):
        for s in range(S):
            step(state[r], msgs[r, s], n_msgs[r, s], max_age, resolved[r, s])
    return resolved, state
