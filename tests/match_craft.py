"""Tables and soft bits made to order for the expected messages (tests only).  ft8gpu_match_candidates takes the waterfall,
the candidates, status_in and one table per frame from the caller, so a test can hand the kernel any vector of 174 integers in
-255..255 as raw soft bits (osd_craft.write_candidate inverts ft8_extract_likelihood) against any table.  The constructed
cases of DESIGN.md "Expected messages" reach what radio frames never do: gates at and below a codeword's hard errors, equal
payloads on both sides of a round seam, tied metrics of different payloads, the last lane of the last round, tables from empty
to full with dead and expired entries in between, ages at the limit and across the 2^32 wrap of the slot counter, saturated
weights, every result code, and garbage in every byte the rule says is ignored.

A frame carries one table and a handful of candidates; every frame is judged under every configuration (max_age, gate).
Everything is generated from fixed seeds; tests/test_match_cpu.py proves each case has the property it is named for, with the
oracle and the restatement (tests/ft8_spec_match.py) alone.

The stream scenario at the end (3 receivers x 4 slots) is synthesised radio: slots 0 and 1 are two disjoint station sets,
slot 2 repeats slot 0 about 10 dB weaker, slot 3 closes slot 1's two-call messages ("B A RR73" after "A B ...") at weak SNR.
Its seed was picked on the CPU with the restatement (scenario_gains): the first of 0..5 at which, at the recommended gate,
slot 2 gains a message, slot 3 gains one with derive = 1, and slot 3 gains none with derive = 0.  All six seeds do -- over the
three receivers seed 0 gains 10 repeats in slot 2 and 18 closings in slot 3, and accepts nothing that was not on the air."""
import os

import numpy as np

import ft8_spec_match as smt
import osd_craft as oc

CAP = oc.CAP
FILL = oc.FILL
AGE = 6                                      # the max_age of the ageing configurations
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_constructed.npz")
CALLS = ("K1ABC", "W9XYZ", "K1JT", "DL1ABC", "G4XYZ", "JA1XYZ", "VK2DEF", "EA5GH", "OH2BH", "PY2ZZ", "ZL1AA", "SM5XX")
GRIDS = ("FN42", "EM48", "FN20", "JO62", "IO91", "PM95", "QF56", "IM98", "KP20", "GG66")


def payload_of(text):
    import rtlsdr_ft8d_amd as ft8
    return ft8.pack77(text)


def random_texts(rng, n):
    """n distinct standard messages (CQ, grid, report, closing)"""
    out = []
    while len(out) < n:
        a, b = rng.choice(len(CALLS), 2, replace=False)
        kind = int(rng.integers(0, 4))
        t = (f"CQ {CALLS[a]} {GRIDS[int(rng.integers(0, len(GRIDS)))]}", f"{CALLS[a]} {CALLS[b]} {GRIDS[int(rng.integers(0, len(GRIDS)))]}",
             f"{CALLS[a]} {CALLS[b]} {int(rng.integers(-24, 10)):+03d}", f"{CALLS[a]} {CALLS[b]} {('RRR', 'RR73', '73')[int(rng.integers(0, 3))]}")[kind]
        if t not in out:
            out.append(t)
    return out


def random_payload(rng):
    """a type 1 payload with random standard-call fields and a random grid / report field (unpack77 accepts it)"""
    n28a, n28b = (int(x) for x in rng.integers(smt.NTOKENS + smt.MAX22, 1 << 28, 2))
    g = int(rng.integers(0, 32400))
    v = ((((n28a << 1) << 29 | (n28b << 1)) << 1) << 15 | g) << 3 | 1
    return np.frombuffer((v << 3).to_bytes(10, "big"), np.uint8)


def unrelated_payloads(rng, n, avoid=()):
    """the payloads of n distinct random CQ messages (synth_util.random_message) that are not in `avoid`: what a receiver's table
    holds beside the messages on the air -- they share the 32 constant bits of "CQ ? ?" with most traffic, so their codewords
    lie nearer to a CQ candidate's soft bits than random payloads do"""
    import synth_util as su
    texts = []
    while len(texts) < n:
        t = su.random_message(rng, cq=True)
        if t not in texts and t not in avoid:
            texts.append(t)
    return [payload_of(t) for t in texts]


def put(state, index, payload, used=1, kind=0, stamp=0):
    e = state["entry"]
    e["payload"][index] = np.frombuffer(bytes(payload), np.uint8)
    e["used"][index], e["kind"][index], e["stamp"][index] = used, kind, stamp


def noisy(rng, cw, errors, strong=(100, 180), weak=(1, 5)):
    """raw soft bits of codeword cw with `errors` weak positions of the wrong sign"""
    mags = rng.integers(*strong, 174)
    v = np.where(np.asarray(cw) == 1, mags, -mags).astype(np.int16)
    bad = rng.choice(174, errors, replace=False)
    v[bad] = -np.sign(v[bad]) * rng.integers(*weak, errors)
    return v


def _refused_payload(oracle, rng):
    for _ in range(256):
        bits = rng.integers(0, 2, 77).astype(np.uint8)
        p = np.packbits(np.concatenate([bits, np.zeros(3, np.uint8)]))
        if oracle.unpack77(p.tobytes())[0] < 0:
            return p
    raise AssertionError("no payload that unpack77 refuses")


# ---- the frames -------------------------------------------------------------------------------------------------------------

def build_cases(oracle):
    """[dict(name, state STATE_DTYPE scalar array [1], cands: [dict(name, v int16 [174], time_offset (optional), ...expectations)])]"""
    frames = []

    def frame(name, state, cands):
        frames.append(dict(name=name, state=state, cands=cands))

    # a: a codeword in noise among unrelated entries, judged at a gate equal to its nhard and at one below
    rng = np.random.default_rng(0xA)
    st = smt.new_state()
    texts = random_texts(rng, 24)
    for k, t in enumerate(texts):
        put(st[0], 3 * k + 1, payload_of(t), stamp=0)
    cands = []
    for e, k in ((0, 0), (12, 5), (30, 11), (45, 23)):
        cands.append(dict(name=f"a_{e}_errors", v=noisy(rng, smt.codeword(payload_of(texts[k])), e), index=3 * k + 1, nhard=e, text=texts[k]))
    frame("a_noise", st, cands)

    # b: the same payload at indices 63 and 64, and at 0 and 511: the smallest index wins across a round seam
    for lo, hi in ((63, 64), (0, 511)):
        st = smt.new_state()
        p = payload_of("K1ABC W9XYZ RR73")
        put(st[0], hi, p)
        put(st[0], lo, p)
        put(st[0], 200, payload_of("CQ K1JT FN20"))
        frame(f"b_same_{lo}_{hi}", st, [dict(name=f"b_{lo}_{hi}", v=noisy(rng, smt.codeword(p), 7), index=lo, nhard=7)])

    # c: two different payloads with equal metric: constant weights and h halfway between the two codewords
    rng = np.random.default_rng(0xC)
    for first, second in ((70, 200), (450, 130)):
        while True:
            pa, pb = random_payload(rng), random_payload(rng)
            diff = np.flatnonzero(smt.codeword(pa) ^ smt.codeword(pb))
            if diff.size % 2 == 0:
                break
        h = smt.codeword(pa).copy()
        h[diff[::2]] ^= 1                                              # half of the differing positions side with pb
        st = smt.new_state()
        put(st[0], first, pa)
        put(st[0], second, pb)
        frame(f"c_tie_{first}_{second}", st, [dict(name=f"c_{first}_{second}", v=np.where(h == 1, 9, -9).astype(np.int16),
                                                   index=min(first, second), nhard=diff.size // 2, tie=True)])

    # d: the best entry in lane 63 of the last round of a full table
    rng = np.random.default_rng(0xD)
    st = smt.new_state()
    for j in range(smt.ENTRIES):
        put(st[0], j, random_payload(rng))
    frame("d_last_lane", st, [dict(name="d_511", v=noisy(rng, smt.codeword(st[0]["entry"]["payload"][511]), 20), index=511, nhard=20),
                              dict(name="d_448", v=noisy(rng, smt.codeword(st[0]["entry"]["payload"][448]), 3), index=448, nhard=3),
                              dict(name="d_0", v=noisy(rng, smt.codeword(st[0]["entry"]["payload"][0]), 9), index=0, nhard=9)])

    # e: tables with 0, 1, 63, 64, 65, 511 and 512 live entries, dead and expired entries in between (slot 100: entries of
    # stamp 100 - AGE - 1 are expired under max_age = AGE and live under max_age = 0)
    rng = np.random.default_rng(0xE)
    for nlive in (0, 1, 63, 64, 65, 511, 512):
        st = smt.new_state()
        st[0]["slot"] = 100
        live = np.sort(rng.choice(smt.ENTRIES, nlive, replace=False))
        for j in range(smt.ENTRIES):
            if j in set(live.tolist()):
                put(st[0], j, random_payload(rng), stamp=100 - int(rng.integers(0, AGE + 1)))
            elif rng.integers(0, 2):
                put(st[0], j, random_payload(rng), used=1, stamp=100 - AGE - 1 - int(rng.integers(0, 50)))       # expired under AGE
            else:
                put(st[0], j, random_payload(rng), used=0, stamp=100)                                            # dead
        cands = []
        if nlive:
            for j in sorted({int(live[0]), int(live[-1]), int(live[len(live) // 2])}):
                cands.append(dict(name=f"e_{nlive}_live_{j}", v=noisy(rng, smt.codeword(st[0]["entry"]["payload"][j]), 10), index_aged=j, nhard=10))
        dead = [j for j in range(smt.ENTRIES) if st[0]["entry"]["used"][j] == 0]
        if dead:
            cands.append(dict(name=f"e_{nlive}_dead", v=noisy(rng, smt.codeword(st[0]["entry"]["payload"][dead[0]]), 0), never=dead[0]))
        cands.append(dict(name=f"e_{nlive}_random", v=(rng.integers(1, 60, 174) * rng.choice([-1, 1], 174)).astype(np.int16)))
        frame(f"e_{nlive}_live", st, cands)

    # f: an age exactly at the limit, one beyond it, and the slot counter wrapped past 2^32
    rng = np.random.default_rng(0xF)
    for name, slot, stamp, live_aged in (("f_at_limit", 1000, 1000 - AGE, True), ("f_beyond", 1000, 1000 - AGE - 1, False),
                                         ("f_wrapped_at_limit", 2, (2 - AGE) & 0xFFFFFFFF, True),
                                         ("f_wrapped_beyond", 2, (2 - AGE - 1) & 0xFFFFFFFF, False),
                                         ("f_future_stamp", 5, 9, False)):
        st = smt.new_state()
        st[0]["slot"] = slot
        p = payload_of("W9XYZ K1ABC -11")
        put(st[0], 77, p, stamp=stamp)
        put(st[0], 300, payload_of("CQ DL1ABC JO62"), stamp=slot)
        frame(name, st, [dict(name=name, v=noisy(rng, smt.codeword(p), 5), index=77, nhard=5, live_aged=live_aged)])

    # g: all-saturated weights: every raw soft bit 254 or 255, h all ones, against the all-zero payload: metric 174 * 255,
    #    result 5; and the all-zero payload as the best entry of an ordinary vector
    rng = np.random.default_rng(0x6)
    st = smt.new_state()
    put(st[0], 9, np.zeros(10, np.uint8))
    frame("g_saturated", st, [dict(name="g_all_saturated", v=rng.integers(254, 256, 174).astype(np.int16), result=5, nhard=174, metric=174 * 255, index=9),
                              dict(name="g_zero_payload", v=noisy(rng, np.zeros(174, np.uint8), 2), result=5, nhard=2, index=9)])

    # h: a payload unpack77 refuses
    rng = np.random.default_rng(0x8)
    st = smt.new_state()
    bad = _refused_payload(oracle, rng)
    put(st[0], 64, bad)
    frame("h_refused", st, [dict(name="h_unpack_refuses", v=noisy(rng, smt.codeword(bad), 4), result=4, nhard=4, index=64)])

    # i: soft bits that are not finite after the normalisation (all zero: NaN; all equal: inf), all symbols outside the
    #    waterfall (NaN), and some of them outside (finite)
    rng = np.random.default_rng(0x9)
    st = smt.new_state()
    p = payload_of("CQ K1ABC FN42")
    put(st[0], 0, p)
    frame("i_not_finite", st, [dict(name="i_all_zero", v=np.zeros(174, np.int16), result=6),
                               dict(name="i_all_minus_7", v=np.full(174, -7, np.int16), result=6),
                               dict(name="i_all_plus_255", v=np.full(174, 255, np.int16), result=6),
                               dict(name="i_all_outside", v=noisy(rng, smt.codeword(p), 0), time_offset=90, result=6),
                               dict(name="i_all_before", v=noisy(rng, smt.codeword(p), 0), time_offset=-80, result=6),
                               dict(name="i_tail_outside", v=noisy(rng, smt.codeword(p), 0), time_offset=30, index=0),
                               dict(name="i_head_outside", v=noisy(rng, smt.codeword(p), 0), time_offset=-10, index=0)])

    # j: garbage where the rule says it is ignored: payload bits 77..79, used values above 1, kind, cursor >= 512, pad
    rng = np.random.default_rng(0x1)
    st = smt.new_state()
    texts = random_texts(rng, 12)
    for k, t in enumerate(texts):
        p = payload_of(t).copy()
        p[9] |= int(rng.integers(1, 8))
        put(st[0], 40 * k + 7, p, used=int(rng.integers(2, 256)), kind=int(rng.integers(0, 256)))
    st[0]["cursor"] = 0xFFFFFE01
    st[0]["pad"] = (0xDEADBEEF, 0x12345678)
    frame("j_garbage", st, [dict(name=f"j_{k}", v=noisy(rng, smt.codeword(payload_of(texts[k])), 6), index=40 * k + 7, nhard=6, text=texts[k])
                            for k in (0, 5, 11)])

    # k: a small random sweep against a random table
    rng = np.random.default_rng(0x2)
    st = smt.new_state()
    for j in rng.choice(smt.ENTRIES, 90, replace=False):
        put(st[0], int(j), random_payload(rng))
    cands = []
    for i in range(24):
        if i % 3 == 0:
            v = rng.integers(0, 3, 174)
        elif i % 3 == 1:
            v = rng.integers(0, 256, 174)
        else:
            j = int(rng.choice(np.flatnonzero(st[0]["entry"]["used"])))
            v = np.abs(noisy(rng, smt.codeword(st[0]["entry"]["payload"][j]), int(rng.integers(20, 70)), strong=(2, 40)))
            v = np.where(noisy(rng, smt.codeword(st[0]["entry"]["payload"][j]), 0) > 0, v, -v)
            flip = rng.choice(174, int(rng.integers(20, 70)), replace=False)
            v[flip] = -v[flip]
        cands.append(dict(name=f"k_{i}", v=(v * (rng.choice([-1, 1], 174) if i % 3 != 2 else 1)).astype(np.int16)))
    frame("k_sweep", st, cands)
    for fr in frames:
        for c in fr["cands"]:
            c["v"] = np.array(c["v"], np.int16)
            c["v"].setflags(write=False)
    return frames


def configs(cases):
    """[(name, max_age, gate)]: every frame is judged under every configuration"""
    errs = sorted({c["nhard"] for fr in cases if fr["name"] == "a_noise" for c in fr["cands"] if c["nhard"] > 0})
    out = [("open", 0, 174), ("aged", AGE, 174), ("gate_0", 0, 0)]
    for e in errs:
        out.append((f"gate_{e}", 0, e))
        if e > 0 and e - 1 not in errs:
            out.append((f"gate_{e - 1}", 0, e - 1))
    seen, uniq = set(), []
    for c in out:
        if c[0] not in seen:
            seen.add(c[0])
            uniq.append(c)
    return uniq


def place(cases, seed=0x3A7C, cap=CAP):
    """the frames' candidates at disjoint freq_offset ranges with fabricated status records: records that are only copied
    (ok != 0, or ldpc_errors == 0) in between, ragged counts, FILL behind the counts, one frame without candidates
    -> dict(mag [B][94208], cands [B][cap], counts [B], status_in uint8 [B][cap][48], states [B], where {case name: (f, i)})"""
    rng = np.random.default_rng(seed)
    B = len(cases) + 1
    cands = np.zeros((B, cap), oc.CAND_DTYPE)
    counts = np.zeros(B, np.int32)
    status = rng.integers(0, 256, (B, cap, 48)).astype(np.uint8)     # junk: an accepted record has to be composed afresh
    mag = np.zeros((B, oc.MAG_ARRAY), np.uint8)
    states = smt.new_state(B)
    where = {}
    for f, fr in enumerate(cases):
        states[f] = fr["state"][0]
        ranges = rng.permutation(oc.PER_FRAME)
        slot = 0
        for k, c in enumerate(fr["cands"]):
            assert k < oc.PER_FRAME and slot < cap - 1
            if rng.integers(0, 3) == 0:                                # copied only; the candidate is not looked at
                cands[f, slot] = (int(rng.integers(0, 60)), int(rng.integers(-12, 24)), int(rng.integers(0, 249)), slot & 1, (slot >> 1) & 1)
                if rng.integers(0, 2):
                    status[f, slot, 9] = (1, 255, 0x40)[int(rng.integers(0, 3))]
                else:
                    status[f, slot, 9], status[f, slot, 0], status[f, slot, 1] = 0, 0, 0
                slot += 1
            to = c.get("time_offset", int(rng.integers(-7, 21)))       # -7..20: every data symbol inside the waterfall
            cands[f, slot] = (int(rng.integers(0, 60)), to, 8 * int(ranges[k]), (slot + f) & 1, ((slot + f) >> 1) & 1)
            status[f, slot, 9] = 0
            status[f, slot, 0:2] = np.frombuffer(np.array([1 if k & 1 else 83], "<i2").tobytes(), np.uint8)
            status[f, slot, 2:4] = np.frombuffer(np.array([int(rng.integers(0, 51))], "<i2").tobytes(), np.uint8)
            oc.write_candidate(mag[f], c["v"], cands[f, slot])
            where[c["name"]] = (f, slot)
            slot += 1
        counts[f] = slot
    states[B - 1] = cases[0]["state"][0]                               # a table, but no candidate
    status[np.arange(cap)[None, :] >= counts[:, None]] = FILL
    return dict(mag=mag, cands=cands, counts=counts, status_in=status, states=states, where=where)


def expected(oracle, placed, cfgs):
    """{config name: (status_out uint8 [B][cap][48] in place on status_in, info [B][cap] prefilled with FILL)}"""
    out = {}
    B, cap = placed["cands"].shape
    for name, max_age, gate in cfgs:
        info0 = np.full((B, cap), FILL, np.uint8).repeat(8, axis=1).view(smt.INFO_DTYPE).reshape(B, cap)
        out[name] = smt.match_candidates(oracle, placed["mag"], placed["cands"], placed["counts"], placed["status_in"], placed["states"],
                                         max_age, gate, status_out=placed["status_in"], info=info0)
    return out


def load_golden(path=GOLDEN):
    """the frozen fixture: dict(mag, cands, counts, status_in, states, names, where, configs [(name, max_age, gate)],
    info_<config>, status_<config>)"""
    d = dict(np.load(path))
    d["cands"] = d["cands"].view(oc.CAND_DTYPE).reshape(d["counts"].shape[0], -1)
    d["states"] = d["states"].view(smt.STATE_DTYPE).reshape(-1)
    d["configs"] = [(str(n), int(a), int(g)) for n, a, g in zip(d["config_names"], d["config_max_age"], d["config_gate"])]
    d["where"] = {str(n): (int(f), int(i)) for n, (f, i) in zip(d["names"], d["slots"])}
    for name, _a, _g in d["configs"]:
        d["info_" + name] = d["info_" + name].view(smt.INFO_DTYPE).reshape(d["counts"].shape[0], -1)
    return d


# ---- the update rule on fabricated records -----------------------------------------------------------------------------------

def update_layout(seed=0x0DD):
    """texts per [receiver][slot] for the update rule: every deriving and non-deriving message type, /R flags, repeats that
    refresh heard and derived entries, heard-over-derived and derived-over-heard, counts outside [0, 50]"""
    import synth_util as su
    rng = np.random.default_rng(seed)
    r0 = [["CQ K1ABC FN42", "K1ABC W9XYZ EM48", "W9XYZ K1ABC -11"],
          ["K1ABC W9XYZ R-09", "W9XYZ K1ABC RRR", "CQ DX K1JT FN20", "K1ABC/R W9XYZ EM48", "K1ABC W9XYZ/R R EM48"],
          [],
          ["K1ABC W9XYZ 73", "CQ K1ABC FN42", "<K1ABC> W9XYZ -05", "W9XYZ <PJ4/K1ABC> RRR", "K1ABC/P W9XYZ/P EM48", "TNX BOB 73 GL",
           "0123456789ABCDEF01", "<W9XYZ> PJ4/K1ABC RR73", "CQ PJ4/K1ABC", "QRZ K1JT FN20", "DE K1JT FN20", "CQ 123 K1JT FN20"],
          ([su.random_message(rng, cq=k % 2 == 0) for k in range(8)], 70),
          ([su.random_message(rng, cq=False) for _ in range(5)], -3)]
    r1 = [[su.random_message(rng, cq=False) for _ in range(45)] for _ in range(6)]      # 45 records x 4 inserts x 6 slots: the ring wraps past 512
    r2 = [["K1ABC W9XYZ RR73"], ["W9XYZ K1ABC -11"], ["K1ABC W9XYZ RR73"], [], ["W9XYZ K1ABC -11"], ["DL1ABC G4XYZ JO62"]]
    return [r0, r1, r2]


# ---- the stream scenario -------------------------------------------------------------------------------------------------------

SCENARIO_SEED = 0


def scenario(oracle, seed=SCENARIO_SEED, R=3, S=4, nsig=12):
    """(iq float32 [R][S][2][48000], texts [R][S]): see the module docstring"""
    import rtlsdr_ft8d_amd as ft8
    import synth_util as su
    assert S == 4
    iq = np.zeros((R, S, 2, su.NSAMPLES), np.float32)
    texts = [[None] * S for _ in range(R)]
    for r in range(R):
        rng = np.random.default_rng(1000 * seed + r)
        first = [su.random_message(rng, cq=k % 2 == 0) for k in range(nsig)]
        second = [su.random_message(rng, cq=False) for _ in range(nsig)]
        closings = [f"{t.split()[1]} {t.split()[0]} {('RR73', 'RRR', '73')[k % 3]}" for k, t in enumerate(second)]
        f0 = 100.0 + np.sort(rng.permutation(22)[:nsig]) * 62.5         # disjoint lanes: eight tones of 6.25 Hz and a gap
        t0 = rng.uniform(0.2, 0.8, nsig)
        snr = [rng.uniform(-12.0, 0.0, nsig) for _ in range(2)]
        plan = [(first, snr[0]), (second, snr[1]), (first, snr[0] - 10.0), (closings, rng.uniform(-23.0, -17.0, nsig))]
        for s, (tx, db) in enumerate(plan):
            noise = np.random.default_rng(77000 + 100 * seed + 10 * r + s)
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


def scenario_gains(oracle, iq, texts, gate, derive, stages=None):
    """per slot: (planted messages gained by matching, accepted messages that were not planted) over the receivers"""
    msgs, n, nbs, _state = smt.decode_expected(oracle, iq, max_hard_errors=gate, derive=derive, stages=stages)
    R, S = n.shape
    out = []
    for s in range(S):
        good = bad = 0
        for r in range(R):
            for k in range(int(nbs[r, s, 0]), int(nbs[r, s, 1])):
                t = msgs[r, s, k]["text"].decode()
                good += t in texts[r][s]
                bad += t not in texts[r][s]
        out.append((good, bad))
    return out
