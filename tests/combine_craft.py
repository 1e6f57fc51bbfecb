"""Memories and soft bits made to order for the soft-bit memory (tests only).  ft8gpu_combine_candidates takes the waterfall,
the candidates, status_in and one memory per frame from the caller, so a test can hand the kernel any vector of 174 integers
in -255..255 as raw soft bits (osd_craft.write_candidate inverts ft8_extract_likelihood) against any memory, whose entries
are written directly as float bit patterns.  The constructed cases of DESIGN.md "Soft-bit memory" reach what radio frames
never do: every result code the rule can give, ties in nagree broken by distance and then by index, expiry at the boundary
and across the 2^32 wrap of the slot counter, count saturating at 255, a sum that cancels to all zero, NaN and infinity in
an entry, normalised sums with single positions at 2^-90, 2^-120, a subnormal and -0.0 beside ordinary values (the cases of
the division guard), a partner at each of the nine position offsets and one at offset 2 that must be ignored.

A frame carries one memory and a handful of candidates at cap 8; every frame is judged under every configuration (max_age,
min_agree).  Everything is generated from fixed seeds; tests/test_combine_cpu.py proves each case has the property it is named
for, with the oracle and the restatement (tests/ft8_spec_combine.py) alone.

The stream scenario at the end (2 receivers x 4 slots = 8 frames) is synthesised radio with the recipe of tests/synth_util.py:
every receiver hears one set of CQ stations in slots 0 and 2 and another in slots 1 and 3, each station at its own
frequency, clock offset and SNR in both of its slots, with fresh noise per slot.  The SNRs sit where BP alone mostly fails."""
import os

import numpy as np

import ft8_spec_combine as sc
import osd_craft as oc

CAP = 8
FILL = oc.FILL
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "combine_constructed.npz")

# ---- the stream scenario -------------------------------------------------------------------------------------------------------

SCENARIO_SEED = 0
SCENARIO_SNR = (-21.0, -18.0)


def scenario(seed=SCENARIO_SEED, R=2, S=4, nsig=12, snr=SCENARIO_SNR):
    """(iq float32 [R][S][2][48000], texts [R][S]): see the module docstring"""
    import rtlsdr_ft8d_amd as ft8
    import synth_util as su
    iq = np.zeros((R, S, 2, su.NSAMPLES), np.float32)
    texts = [[None] * S for _ in range(R)]
    for r in range(R):
        rng = np.random.default_rng(1000 * seed + r)
        sets = []
        for _ in range(2):
            tx = [su.random_message(rng, cq=True) for _ in range(nsig)]
            f0 = 100.0 + np.sort(rng.permutation(22)[:nsig]) * 62.5       # disjoint lanes: eight tones of 6.25 Hz and a gap
            sets.append((tx, f0, rng.uniform(0.2, 0.8, nsig), rng.uniform(snr[0], snr[1], nsig)))
        for s in range(S):
            tx, f0, t0, db = sets[s & 1]
            noise = np.random.default_rng(91000 + 100 * seed + 10 * r + s)
            fi, fq = noise.normal(0.0, 1.0, su.NSAMPLES), noise.normal(0.0, 1.0, su.NSAMPLES)
            for k, t in enumerate(tx):
                si, sq = su.cpfsk(ft8.encode(ft8.pack77(t)), float(f0[k]), int(round(t0[k] * 3200)), su.amplitude_for_snr(float(db[k]), 1.0))
                fi += si
                fq += sq
            i32, q32 = fi.astype(np.float32), fq.astype(np.float32)
            scale = np.float32(0.5) / max(np.abs(i32).max(), np.abs(q32).max(), np.float32(1e-24))
            iq[r, s, 0], iq[r, s, 1] = i32 * scale, q32 * scale
            texts[r][s] = list(tx)
    return iq, texts


def scenario_gains(oracle, iq, texts, min_agree, store_per_slot=sc.ENTRIES, max_age=0, stages=None, bp=None, max_candidates=120):
    """per slot: (planted messages BP alone decodes, planted messages gained by combining, accepted messages that were not
    planted) over the receivers, and the decode's (msgs, n, nbs, state)"""
    res = sc.decode_combined(oracle, iq, min_agree=min_agree, max_age=max_age, store_per_slot=store_per_slot, stages=stages,
                             bp=bp or oracle.bp_decode, max_candidates=max_candidates)
    msgs, n, nbs, _state = res
    R, S = n.shape
    out = []
    for s in range(S):
        base = good = bad = 0
        for r in range(R):
            base += sum(msgs[r, s, k]["text"].decode() in texts[r][s] for k in range(int(nbs[r, s, 0])))
            for k in range(int(nbs[r, s, 0]), int(nbs[r, s, 1])):
                t = msgs[r, s, k]["text"].decode()
                good += t in texts[r][s]
                bad += t not in texts[r][s]
        out.append((base, good, bad))
    return out, res


# ---- constructed memories and candidates -------------------------------------------------------------------------------------

AGE = 6                                      # the max_age of the ageing configurations
GATE = 120                                   # the min_agree of the gated configurations
CONFIGS = (("open", 0, 0), ("gate", 0, GATE), ("aged", AGE, 0), ("full", 0, 174), ("aged_gate", AGE, GATE))
STORES = (0, 1, 3, 128)                      # store_per_slot of the update expectations
TINY = {"p90": 0x12800000, "p120": 0x03800000, "sub": 0x00000200, "negzero": 0x80000001}      # 2^-90, 2^-120, a subnormal, and the
# smallest negative subnormal, which a norm factor below one half rounds to -0.0


def codeword_of(text):
    import ft8_spec_match as smt
    import rtlsdr_ft8d_amd as ft8
    return smt.codeword(bytes(ft8.pack77(text)))


def codeword_of_bits(bits91):
    """the LDPC codeword of any 91 message bits (the CRC is whatever the bits say)"""
    import ft8_spec_osd as so
    return ((np.asarray(bits91, np.int64) @ so.generator_matrix().astype(np.int64)) & 1).astype(np.uint8)


def signed(cw, mag):
    return np.where(np.asarray(cw) == 1, mag, -mag)


def cand_at(T, F, score=20):
    """the candidate record at position T = 2 * time_offset + time_sub, F = 2 * freq_offset + freq_sub"""
    c = np.zeros(1, sc.CAND_DTYPE)[0]
    c["score"], c["time_offset"], c["time_sub"], c["freq_offset"], c["freq_sub"] = score, T >> 1, T & 1, F >> 1, F & 1
    return c


def put(state, index, T, F, llr, used=1, count=1, stamp=0, pad=0, tail=(0.0, 0.0)):
    """entry `index` of a state (a STATE_DTYPE scalar); llr: 174 float32 values or uint32 bit patterns"""
    e = state["entry"]
    e["cand"][index] = cand_at(T, F, score=int(index))
    e["used"][index], e["count"][index], e["pad"][index], e["stamp"][index] = used, count, pad, stamp
    llr = np.asarray(llr)
    e["llr"][index][:174] = llr.view(np.float32) if llr.dtype == np.uint32 else llr.astype(np.float32)
    e["llr"][index][174:] = tail


def build_cases(oracle):
    """[dict(name, state STATE_DTYPE [1], cands: [dict(name, v int16 [174], T, F)])]: the candidates of a frame sit at
    freq_offset 8 * k (disjoint tone cells), F = 16 * k + freq_sub"""
    import match_craft as mcr
    frames = []

    def frame(name, state, cands):
        assert len(cands) <= CAP - 2
        frames.append(dict(name=name, state=state, cands=cands))

    def pos(k, ts=0, fs=0, to=3):
        return 2 * to + ts, 16 * k + fs

    rng = np.random.default_rng(0xC0B)
    cw = codeword_of("CQ K1ABC FN42")
    cw2 = codeword_of("CQ DL1ABC JO62")

    # a: the results.  accept: a clean entry and weak, error-ridden own soft bits; crc: a codeword whose CRC field is wrong;
    # unpack: a payload unpack77 refuses; none: junk; allzero: every soft bit negative (bp_decode leaves at once: 7); own6: zero variance
    st = sc.new_state()
    T, F = pos(1)
    put(st[0], 7, T, F, signed(cw, 4.0))
    bits = rng.integers(0, 2, 91).astype(np.uint8)
    T2, F2 = pos(4, ts=1)
    put(st[0], 64, T2, F2, signed(codeword_of_bits(bits), 5.0))
    refused = mcr._refused_payload(oracle, np.random.default_rng(5))
    import ft8_spec_match as smt
    T3, F3 = pos(9, fs=1)
    put(st[0], 127, T3, F3, signed(smt.codeword(bytes(refused)), 6.0))
    T4, F4 = pos(13)
    put(st[0], 0, T4, F4, rng.normal(0.0, 6.0, 174))
    T5, F5 = pos(20, ts=1, fs=1)
    put(st[0], 63, T5, F5, np.full(174, -5.0))
    T6, F6 = pos(25)
    put(st[0], 100, T6, F6, signed(cw, 4.0))
    frame("a", st, [
        dict(name="a_accept", v=mcr.noisy(rng, cw, 40, strong=(20, 60)), T=T, F=F),
        dict(name="a_crc", v=mcr.noisy(rng, codeword_of_bits(bits), 30, strong=(20, 60)), T=T2, F=F2),
        dict(name="a_unpack", v=mcr.noisy(rng, smt.codeword(bytes(refused)), 30, strong=(20, 60)), T=T3, F=F3),
        dict(name="a_none", v=rng.integers(-200, 200, 174), T=T4, F=F4),
        dict(name="a_allzero", v=-rng.integers(1, 200, 174), T=T5, F=F5),
        dict(name="a_own6", v=np.zeros(174, np.int16), T=T6, F=F6)])

    # b: the gate.  own agrees with the entry in exactly GATE and in GATE - 1 positions
    st = sc.new_state()
    cands = []
    for k, nag in enumerate((GATE, GATE - 1, 174, 0)):
        T, F = pos(2 + 3 * k, ts=k & 1)
        put(st[0], 10 + k, T, F, signed(cw, 4.0))
        v = signed(cw, rng.integers(30, 90, 174))
        flip = rng.choice(174, 174 - nag, replace=False)
        v[flip] = -v[flip]
        cands.append(dict(name=f"b_agree{nag}", v=v, T=T, F=F, nagree=nag))
    frame("b", st, cands)

    # c: ties.  equal nagree: the smaller distance wins over the smaller index; equal distance: the smaller index; a larger
    # nagree wins over both
    st = sc.new_state()
    T, F = pos(3)
    put(st[0], 5, T + 1, F, signed(cw, 4.0))
    put(st[0], 9, T, F, signed(cw, 2.0))                  # the same signs at distance 0
    put(st[0], 3, T + 1, F + 1, signed(cw, 3.0))          # distance 2
    T2, F2 = pos(8)
    put(st[0], 40, T2, F2 + 1, signed(cw2, 4.0))
    put(st[0], 33, T2 - 1, F2, signed(cw2, 4.0))          # distance 1 both: index 33
    T3, F3 = pos(12)
    worse = signed(cw, 4.0)
    worse[:10] = -worse[:10]
    put(st[0], 50, T3, F3, worse)                         # distance 0, ten positions fewer
    put(st[0], 90, T3 - 1, F3 - 1, signed(cw, 4.0))       # distance 2, all positions
    frame("c", st, [dict(name="c_dist", v=mcr.noisy(rng, cw, 20, strong=(20, 60)), T=T, F=F, index=9),
                    dict(name="c_index", v=mcr.noisy(rng, cw2, 20, strong=(20, 60)), T=T2, F=F2, index=33),
                    dict(name="c_nagree", v=mcr.noisy(rng, cw, 20, strong=(20, 60)), T=T3, F=F3, index=90)])

    # d, e: expiry at the boundary (age AGE is live, AGE + 1 is not) and across the 2^32 wrap of slot - stamp; dead entries
    for name, slot, stamps in (("d", 10, (10 - AGE, 10 - AGE - 1)), ("e", 2, ((2 - AGE) & 0xFFFFFFFF, (2 - AGE - 1) & 0xFFFFFFFF))):
        st = sc.new_state()
        st[0]["slot"] = slot
        cands = []
        for k, stamp in enumerate(stamps):
            T, F = pos(4 + 5 * k, fs=k)
            put(st[0], 20 + 70 * k, T, F, signed(cw, 4.0), stamp=stamp, count=3 + k)
            cands.append(dict(name=f"{name}_age{k}", v=mcr.noisy(rng, cw, 25, strong=(20, 60)), T=T, F=F, live_when_aged=(k == 0)))
        T, F = pos(20)
        put(st[0], 1, T, F, signed(cw, 4.0), used=0, stamp=slot)
        cands.append(dict(name=f"{name}_dead", v=mcr.noisy(rng, cw, 25, strong=(20, 60)), T=T, F=F))
        frame(name, st, cands)

    # f: what an entry may hold.  count 255 with a failing sum (the update saturates), a sum that cancels to all zero, NaN, infinity
    st = sc.new_state()
    cands = []
    T, F = pos(1)
    put(st[0], 2, T, F, rng.normal(0.0, 9.0, 174), count=255)
    cands.append(dict(name="f_count255", v=rng.integers(-200, 200, 174), T=T, F=F))
    T, F = pos(5, ts=1)
    v = mcr.noisy(rng, cw, 25, strong=(20, 60))
    cands.append(dict(name="f_cancel", v=v, T=T, F=F, cancel=66))
    for k, (nm, bad) in enumerate((("f_nan", np.nan), ("f_inf", np.inf), ("f_ninf", -np.inf))):
        T, F = pos(9 + 4 * k)
        llr = signed(cw, 4.0).astype(np.float32)
        llr[17 + 50 * k] = bad
        put(st[0], 30 + k, T, F, llr)
        cands.append(dict(name=nm, v=mcr.noisy(rng, cw, 25, strong=(20, 60)), T=T, F=F))
    frame("f", st, cands)

    # g: the guard cases.  own is zero at a few positions where the entry holds 2^-90, 2^-120, a subnormal or -2^-149: the
    # normalised sum has those beside ordinary values (-2^-149 becomes -0.0: the entry is strong there, so the norm factor is
    # below one half); one candidate does not converge, one has all four kinds at once
    st = sc.new_state()
    cands = []
    for k, kinds in enumerate((("p90",), ("p120",), ("sub",), ("negzero",), ("p90", "p120", "sub", "negzero"), ("p90", "sub"))):
        T, F = pos(1 + 5 * k, ts=k & 1, fs=(k >> 1) & 1)
        junk = k == 5
        base = rng.normal(0.0, 5.0, 174).astype(np.float32) if junk else signed(cw2, np.float32(8.0 if "negzero" in kinds else 3.0)).astype(np.float32)
        bitsv = base.view(np.uint32).copy()
        v = rng.integers(-200, 200, 174) if junk else mcr.noisy(rng, cw2, 45, strong=(20, 60))
        where = rng.choice(174, 3 * len(kinds), replace=False)
        for j, p in enumerate(where):
            bitsv[p] = TINY[kinds[j % len(kinds)]] | (0x80000000 if (j & 1) and kinds[j % len(kinds)] != "negzero" else 0)
            v[p] = 0
        put(st[0], 11 * k + 4, T, F, bitsv)
        cands.append(dict(name="g_" + "_".join(kinds) + ("_junk" if junk else ""), v=v, T=T, F=F, tiny=sorted(int(p) for p in where)))
    frame("g", st, cands)

    # h, i: a partner at each of the nine position offsets; at offset 2 in time or in frequency: ignored
    offs = [(dt, df) for dt in (-1, 0, 1) for df in (-1, 0, 1)]
    for name, part in (("h", offs[:5]), ("i", offs[5:] + [(2, 0), (0, -2)])):
        st = sc.new_state()
        cands = []
        for k, (dt, df) in enumerate(part):
            T, F = pos(2 + 5 * k, ts=k & 1, fs=(k >> 1) & 1, to=5 + k)
            put(st[0], 60 + k, T + dt, F + df, signed(cw, 4.0))
            cands.append(dict(name=f"{name}_off{dt:+d}{df:+d}", v=mcr.noisy(rng, cw, 25, strong=(20, 60)), T=T, F=F, off=(dt, df)))
        frame(name, st, cands)

    # j: the ring.  cursor 126 + 128 k: the stored entries wrap to 0, 1, ...; entry 126, the partner of the SECOND stored
    # candidate (BP runs on the sum and fails), is overwritten by the FIRST one in the same slot
    st = sc.new_state()
    st[0]["cursor"] = 126 + 128 * 3
    st[0]["slot"] = 41
    cands = []
    T, F = pos(2)
    cands.append(dict(name="j_first", v=rng.integers(-200, 200, 174), T=T, F=F))
    T, F = pos(6, ts=1)
    put(st[0], 126, T, F, rng.normal(0.0, 9.0, 174), count=7, stamp=40)
    cands.append(dict(name="j_partner_overwritten", v=rng.integers(-200, 200, 174), T=T, F=F))
    for k in range(3):
        T, F = pos(10 + 4 * k, fs=1)
        cands.append(dict(name=f"j_more{k}", v=rng.integers(-200, 200, 174), T=T, F=F))
    T, F = pos(24)
    put(st[0], 0, T, F, signed(cw, 4.0), count=2, stamp=39)
    cands.append(dict(name="j_accept_not_stored", v=mcr.noisy(rng, cw, 25, strong=(20, 60)), T=T, F=F))
    frame("j", st, cands)
    return frames


def place(oracle, cases, seed=0xC0B1, cap=CAP):
    """the frames' candidates with fabricated status records: records that are only copied (ok != 0, or ldpc_errors == 0) in
    between, ragged counts, FILL behind the counts, one frame without candidates
    -> dict(mag [B][94208], cands [B][cap], counts [B], status_in uint8 [B][cap][48], states [B], where {case name: (f, i)})"""
    rng = np.random.default_rng(seed)
    B = len(cases) + 1
    cands = np.zeros((B, cap), oc.CAND_DTYPE)
    counts = np.zeros(B, np.int32)
    status = rng.integers(0, 256, (B, cap, 48)).astype(np.uint8)     # junk: an accepted record has to be composed afresh
    mag = np.zeros((B, oc.MAG_ARRAY), np.uint8)
    states = sc.new_state(B)
    where = {}
    for f, fr in enumerate(cases):
        states[f] = fr["state"][0]
        slot = 0
        copies = set(rng.choice(len(fr["cands"]) + 1, min(2, cap - len(fr["cands"])), replace=False).tolist())
        for k, c in enumerate(fr["cands"]):
            if k in copies:                                            # copied only; the candidate is not looked at
                cands[f, slot] = (int(rng.integers(0, 60)), int(rng.integers(-12, 24)), int(rng.integers(0, 249)), slot & 1, (slot >> 1) & 1)
                if rng.integers(0, 2):
                    status[f, slot, 9] = (1, 255, 0x40)[int(rng.integers(0, 3))]
                else:
                    status[f, slot, 9], status[f, slot, 0], status[f, slot, 1] = 0, 0, 0
                slot += 1
            cands[f, slot] = cand_at(c["T"], c["F"], score=int(rng.integers(0, 60)))
            status[f, slot, 9] = 0
            status[f, slot, 0:2] = np.frombuffer(np.array([1 if k & 1 else 83], "<i2").tobytes(), np.uint8)
            status[f, slot, 2:4] = np.frombuffer(np.array([int(rng.integers(0, 51))], "<i2").tobytes(), np.uint8)
            oc.write_candidate(mag[f], np.asarray(c["v"], np.int64), cands[f, slot])
            if "cancel" in c:                                          # the entry is minus the candidate's own soft bits
                own = oracle.llr(mag[f], cands[f, slot])
                put(states[f], c["cancel"], c["T"], c["F"], -own)
            where[c["name"]] = (f, slot)
            slot += 1
        counts[f] = slot
    states[B - 1] = cases[0]["state"][0]                               # a memory, but no candidate
    status[np.arange(cap)[None, :] >= counts[:, None]] = FILL
    return dict(mag=mag, cands=cands, counts=counts, status_in=status, states=states, where=where)


def expected(oracle, placed, bp=None):
    """{config name: (status_out uint8 [B][cap][48] in place on status_in, info [B][cap] prefilled with FILL,
    {store_per_slot: exit states [B]})}"""
    out = {}
    B, cap = placed["cands"].shape
    for name, max_age, gate in CONFIGS:
        info0 = np.full((B, cap), FILL, np.uint8).repeat(8, axis=1).view(sc.INFO_DTYPE).reshape(B, cap)
        status, info = sc.combine_candidates(oracle, placed["mag"], placed["cands"], placed["counts"], placed["status_in"],
                                             placed["states"], max_age, gate, status_out=placed["status_in"], info=info0, bp=bp)
        after = {s: sc.update(oracle, placed["mag"], placed["cands"], placed["counts"], status, info, placed["states"], s) for s in STORES}
        out[name] = (status, info, after)
    return out


def load_golden(path=GOLDEN):
    d = dict(np.load(path))
    B = d["counts"].shape[0]
    d["cands"] = d["cands"].view(oc.CAND_DTYPE).reshape(B, -1)
    d["states"] = d["states"].view(sc.STATE_DTYPE).reshape(B)
    d["where"] = {str(n): (int(f), int(i)) for n, (f, i) in zip(d["names"], d["slots"])}
    for name, _age, _gate in CONFIGS:
        d["info_" + name] = d["info_" + name].view(sc.INFO_DTYPE).reshape(B, -1)
        for s in STORES:
            d[f"after_{name}_{s}"] = d[f"after_{name}_{s}"].view(sc.STATE_DTYPE).reshape(B)
    return d
