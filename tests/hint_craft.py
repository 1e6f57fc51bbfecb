"""Constructed cases for the call hints (ft8gpu_hint_candidates / ft8gpu_hint_update / ft8gpu_decode_messages_hinted), all
produced on the CPU from the restatement (tests/ft8_spec_hint.py) and the oracle.

Soft bits.  The vectors of tests/ap_craft.py (converging and failing words, a wrong CRC, a payload unpack77 refuses, unusable
soft bits, random sweeps) and three planted two-call messages BP fails on while "A B ?" recovers them (p_0 .. p_2; p_0 has at
least two wrong hard decisions in its call fields, p_2 none in field 1 but some in field 2), placed by osd_craft.build_frames
(fabricated status records, copied-only records in between, ragged counts, a frame without candidates).

Tables.  configs() gives (name, one state used for every frame, tries, max_bad_per_64, max_hard_errors, max_age, use_phase): no
live entry, expired entries, wrong phase with use_phase 0 and 1, the planted entry at indices 0 / 63 / 64 / 511, kind 0 and 4,
garbage above bit 28, nbad at the gate and one above, gates 0 and 64, key ties between sizes and within one size, five passing
entries with the planted one ranked first / fourth / fifth at tries 1..4, and a first try that fails in front of an accepted
one with each of 7 (BP finds no codeword), 8 (q_8), 2 (the hard-error gate, p_2), 3 (q_3: a wrong CRC) and 4 (q_4: a field
unpack77 refuses).

update_layout(): fabricated records for the update rule.  scenario(): 3 receivers x 4 slots of QSOs that advance CQ -> call ->
report -> R-report -> RR73, the later steps too weak for BP."""
import os

import numpy as np

import ap_craft as ac
import ft8_spec_ap as sa
import ft8_spec_hint as sh
import ft8_spec_osd as so
import osd_craft as oc

CAP = oc.CAP
FILL = oc.FILL
ITERS = 20
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hint_constructed.npz")
P_TEXTS = ("K1ABC W9XYZ -11", "DL1ABC G4XYZ R-08", "JA1XYZ VK2DEF JO62")
UNRELATED = ("EA5GH", "OH2BH", "PY2ZZ", "ZL1AA", "SM5XX", "K1JT", "W1AW", "G3ABC", "F5XYZ", "I2ABC", "VE3DEF", "LU1XX")


def fields_of_text(text):
    """(F1, F2) of a standard message"""
    import ft8_spec_pack as sp
    tok = text.split()
    p = np.frombuffer(sp.pack_standard(tok[0], tok[1], tok[2] if len(tok) > 2 else ""), np.uint8)
    i3, f1, f2 = sh.fields(p)
    assert i3 == 1
    return f1, f2


def call_field(call):
    """the 29-bit field of a standard call in clear"""
    return fields_of_text(f"{call} {call} RRR")[0]


def put(state, index, kind, a, b, phase=0, used=1, stamp=0):
    e = state["entry"][0] if state.shape else state["entry"]
    e[index] = (a, b, stamp, kind, used, phase, 0)


def h_field(v, first):
    """the hard decisions of v on payload bits [first, first + 29) as a number, MSB first"""
    return int("".join("1" if x > 0 else "0" for x in v[first:first + 29]), 2)


def nbad_of(v, a, b):
    """(wrong hard decisions in field 1, in field 2, in i3) against the fields a, b"""
    return bin(h_field(v, 0) ^ a).count("1"), bin(h_field(v, 29) ^ b).count("1"), int(v[74] > 0) + int(v[75] > 0) + int(v[76] <= 0)


def _planted(cases, oracle):
    for k, text in enumerate(P_TEXTS):
        a, b = fields_of_text(text)
        e = np.zeros(1, sh.ENTRY_DTYPE)[0]
        e["a"], e["b"], e["kind"] = a, b, 3
        hyp = sh.hypothesis(e)
        cw = oc._payload_codeword(ac._payload_bits(oracle, text))
        rng = np.random.default_rng(0x1A0 + k)
        for trial in range(20000):
            v = ac._noisy(rng, cw, 20.0, 27.0 + (trial % 5))
            if k == 2:                                                 # field 1 and i3 as sent, at the magnitudes the noise left
                at = np.r_[0:29, 74:77]
                v[at] = np.where(cw[at] == 1, np.abs(v[at]), -np.abs(v[at]))
            n1, n2, n3 = nbad_of(v, a, b)
            if (k == 0 and (n1 + n2 < 2 or n3)) or (k == 2 and (n1 or n3 or not n2)) or (n1 + n2 + n3) * 64 > 16 * 61:
                continue
            llr = ac.llr_of(v)
            if oracle.bp_decode(llr, ITERS)[1] == 0:
                continue
            info, win = sa.resolve(oracle, llr, sa.attempts(oracle, llr, [hyp], ITERS), 174)
            if win is None or not np.array_equal(win[0], cw):
                continue
            if k == 2:                                                 # "A ? ?" alone recovers it too, with more hard errors
                e1 = e.copy()
                e1["kind"] = 1
                i1, w1 = sa.resolve(oracle, llr, sa.attempts(oracle, llr, [sh.hypothesis(e1)], ITERS), 174)
                if w1 is None or not np.array_equal(w1[0], cw) or int(i1["nhard"]) <= int(info["nhard"]):
                    continue
            break
        else:
            raise AssertionError("no vector that BP misses and the hint recovers: " + text)
        cases.append(dict(case="p", name=f"p_{k}", v=v, text=text, a=a, b=b, codeword=cw, nhard=int(info["nhard"])))


BAD_TOKEN = 1000000 << 1                    # field 1 with n28 between the "CQ aaaa" tokens and NTOKENS: unpack77 refuses it
Q_TEXT, Q_OTHER = "OH2BH EA5GH -07", "SM5XX"


def _word(f1, f2, third16, crc_xor=0):
    """the codeword of the type 1 payload (f1, f2, third field), its CRC-14 XORed with crc_xor"""
    bits = np.array([int(c) for c in format((((f1 << 29 | f2) << 16 | third16) << 3) | 1, "077b")], np.uint8)
    crc = so.crc14(bits) ^ crc_xor
    info = np.concatenate([bits, [(crc >> (13 - i)) & 1 for i in range(14)]]).astype(np.int64)
    return ((info @ so.generator_matrix().astype(np.int64)) & 1).astype(np.uint8)


def _entry(kind, a, b):
    e = np.zeros(1, sh.ENTRY_DTYPE)[0]
    e["a"], e["b"], e["kind"] = a, b, kind
    return e


def _between(cases, oracle):
    """q_3 / q_4: soft bits between two words that share field 2 and the third field -- a word no decoder may accept (its CRC
    is wrong; its field 1 is a token unpack77 refuses) and a sent message.  Where the words agree the soft bits are strong;
    field 1 leans weakly to the bad word, so "X ? ?" of the bad word ranks in front of "A B ?" of the message; the other
    positions where they differ are weak with random signs.  BP under the first entry lands on the bad word (3 / 4), under
    the second on the message.  q_8: a clean word of the message whose hard decision is wrong at one bit of field 1 -- the
    entry that agrees with that wrong bit ranks first, BP overturns the forced bit and leaves a codeword that differs from
    the hypothesis on a masked position (8); "A B ?" is accepted next."""
    a, b = fields_of_text(Q_TEXT)
    i3, f1, f2 = sh.fields(np.packbits(np.concatenate([ac._payload_bits(oracle, Q_TEXT), np.zeros(3, np.uint8)])))
    assert (i3, f1, f2) == (1, a, b)
    third = int("".join(map(str, ac._payload_bits(oracle, Q_TEXT)[58:74])), 2)
    good = _word(a, b, third)
    assert np.array_equal(good, oc._payload_codeword(ac._payload_bits(oracle, Q_TEXT)))
    other = call_field(Q_OTHER)
    rc, _t = oracle.unpack77(np.packbits(np.concatenate([_word(BAD_TOKEN, b, third)[:77], np.zeros(3, np.uint8)])).tobytes())
    assert rc < 0
    for name, code, x, bad in (("q_3", 3, other, _word(other, b, third, 1)), ("q_4", 4, BAD_TOKEN, _word(BAD_TOKEN, b, third))):
        hx, hy = sh.hypothesis(_entry(1, x, 0)), sh.hypothesis(_entry(3, a, b))
        for seed in range(400):
            rng = np.random.default_rng(0x9000 + 1000 * code + seed)
            differ = good != bad
            v = oc._signed(good, rng.integers(60, 200, 174))
            v[differ] = (rng.integers(1, 4, int(differ.sum())) * rng.choice([-1, 1], int(differ.sum()))).astype(np.int16)
            f1d = np.flatnonzero(differ[:29])
            v[f1d] = np.where(bad[f1d] == 1, 1, -1) * rng.integers(1, 4, len(f1d))
            llr = ac.llr_of(v)
            ix, wx = sa.resolve(oracle, llr, sa.attempts(oracle, llr, [hx], ITERS), 174)
            iy, wy = sa.resolve(oracle, llr, sa.attempts(oracle, llr, [hy], ITERS), 174)
            if int(ix["result"]) == code and wy is not None and np.array_equal(wy[0], good):
                break
        else:
            raise AssertionError(f"no soft bits between the two words for code {code}")
        cases.append(dict(case="q", name=name, v=v, text=Q_TEXT, a=a, b=b, x=x, codeword=good, result=code))
    rng = np.random.default_rng(0x98)
    v = oc._signed(good, rng.integers(100, 181, 174))
    v[5] = -np.sign(v[5]) * 2
    x = _flip(a, [5])
    llr = ac.llr_of(v)
    ix, _w = sa.resolve(oracle, llr, sa.attempts(oracle, llr, [sh.hypothesis(_entry(1, x, 0))], ITERS), 174)
    assert int(ix["result"]) == 8, ix
    cases.append(dict(case="q", name="q_8", v=v, text=Q_TEXT, a=a, b=b, x=x, codeword=good, result=8))


_cases = []


def build_cases(oracle):
    if not _cases:
        cases = [dict(c) for c in ac.build_cases(oracle)]
        _planted(cases, oracle)
        _between(cases, oracle)
        for c in cases:
            c["v"] = np.array(c["v"], np.int16)
            c["v"].setflags(write=False)
        _cases.extend(cases)
    return _cases


def _flip(value, positions):
    """a 29-bit field with the payload bits at `positions` (0 = the MSB) inverted"""
    for p in positions:
        value ^= 1 << (28 - p)
    return value


def _agreeing(v, first, field, agree):
    """positions of the field (0..28) at which v's hard decision agrees (or disagrees) with it"""
    h = h_field(v, first)
    return [p for p in range(29) if (((h ^ field) >> (28 - p)) & 1 == 0) == agree]


def configs(cases):
    """[(name, state [1], tries, max_bad_per_64, max_hard_errors, max_age, use_phase)]"""
    by = {c["name"]: c for c in cases}
    p0, p1, p2 = by["p_0"], by["p_1"], by["p_2"]
    unrelated = [call_field(c) for c in UNRELATED]
    out = []

    def state(slot=10):
        st = sh.new_state(1)
        st["slot"] = slot
        return st

    def planted_all(st, at=(5, 70, 300), phase=0, stamp=10):
        for i, c in zip(at, (p0, p1, p2)):
            put(st, i, 3, c["a"], c["b"], phase, stamp=stamp)

    def add(name, st, tries=2, gate=16, hard=174, max_age=0, use_phase=1):
        out.append((name, st, tries, gate, hard, max_age, use_phase))

    add("empty", state())
    st = state()
    planted_all(st)
    add("planted", st)
    st = state(slot=100)
    planted_all(st, stamp=90)
    add("expired", st, max_age=9)
    add("not_expired", st, max_age=10)
    st = state(slot=0x00000003)
    planted_all(st, stamp=0xFFFFFFFE, phase=1)
    add("wrapped_age", st, max_age=5)
    st = state(slot=11)
    planted_all(st, phase=0)
    add("wrong_phase_used", st, use_phase=1)
    add("wrong_phase_ignored", st, use_phase=0)
    st = state(slot=11)
    planted_all(st, phase=0xFF)                                        # read & 1
    add("phase_garbage", st, use_phase=1)
    for at in ((0, 63, 64), (511, 0, 63), (64, 511, 0), (63, 64, 511)):
        st = state()
        planted_all(st, at=at)
        for j, u in enumerate(unrelated):
            put(st, 100 + 7 * j, 1 + j % 3, u, unrelated[(j + 1) % len(unrelated)], j & 1, stamp=10)
        add("at_%d_%d_%d" % at, st, tries=4)
    st = state()
    for i, c in zip((5, 70, 300), (p0, p1, p2)):
        put(st, i, 0 if i != 70 else 4, c["a"], c["b"], 0, stamp=10)
    put(st, 6, 3, p0["a"], p0["b"], 0, used=0, stamp=10)             # kind 3 but not used
    add("kind_0_and_4", st)
    st = state()
    for i, c in zip((5, 70, 300), (p0, p1, p2)):
        put(st, i, 3, c["a"] | 0xE0000000, c["b"] | 0xA0000000, 0xFE, stamp=10)
    add("garbage_above_bit_28", st)
    # nbad at the gate and one above: a kind 1 entry made from p_0's own hard decisions with k bits inverted has nbad = k
    # (p_0's i3 decisions are right), and nbad * 64 <= gate * 32 says 2 k <= gate
    h1 = h_field(p0["v"], 0)
    for k, gate, name in ((3, 6, "nbad_at_the_gate"), (4, 6, "nbad_above_the_gate"), (0, 0, "gate_0_passes_nbad_0"), (1, 0, "gate_0_refuses_nbad_1")):
        st = state()
        put(st, 9, 1, _flip(h1, range(k)), 0, 0, stamp=10)
        add(name, st, tries=1, gate=gate)
    st = state()
    planted_all(st)
    for j, u in enumerate(unrelated):
        put(st, 20 + j, 1 + j % 3, u, unrelated[(j + 3) % len(unrelated)], 0, stamp=10)
    for tries in (1, 4):
        add(f"gate_64_tries_{tries}", st, tries=tries, gate=64)
    # ties: entries made from p_0's hard decisions have nbad 0 whatever their size -- the 61-bit entry goes first, then the
    # smaller index
    h2 = h_field(p0["v"], 29)
    st = state()
    put(st, 3, 1, h1, 0, 0, stamp=10)
    put(st, 4, 2, 0, h2, 0, stamp=10)
    put(st, 400, 3, h1, h2, 0, stamp=10)
    put(st, 2, 1, _flip(h1, [7]), 0, 0, stamp=10)
    add("ties_between_and_within_sizes", st, tries=4)
    # five passing entries: p_0's own and four decoys that differ from it in one bit -- where p_0's hard decision is wrong
    # the decoy ranks in front of it, where it is right behind it
    wrong = [(0, p) for p in _agreeing(p0["v"], 0, p0["a"], False)] + [(1, p) for p in _agreeing(p0["v"], 29, p0["b"], False)]
    right = [(0, p) for p in _agreeing(p0["v"], 0, p0["a"], True)][:4]
    assert len(wrong) >= 2

    def decoy(which):
        fld, p = which
        return (_flip(p0["a"], [p]), p0["b"]) if fld == 0 else (p0["a"], _flip(p0["b"], [p]))

    # (a decoy in front at a smaller index may also tie with another decoy: the index decides)
    for rank in (1, 4, 5):
        front = rank - 1
        st = state()
        firsts = [wrong[j % len(wrong)] for j in range(front)]
        # decoys in front: one wrong position each; if there are more decoys than wrong positions, two wrong positions at once
        seen = set()
        for j in range(front):
            a, b = decoy(firsts[j])
            if (a, b) in seen:
                a, b = decoy(wrong[0])
                a2, b2 = decoy(wrong[1])
                a, b = a ^ (a2 ^ p0["a"]), b ^ (b2 ^ p0["b"])
            seen.add((a, b))
            put(st, 40 + j, 3, a, b, 0, stamp=10)
        put(st, 200, 3, p0["a"], p0["b"], 0, stamp=10)
        for j in range(4 - front):
            a, b = decoy(right[j])
            put(st, 300 + j, 3, a, b, 0, stamp=10)
        for tries in (1, 2, 3, 4):
            add(f"planted_ranked_{rank}_tries_{tries}", st, tries=tries, gate=24)
    # the hard-error gate refuses the first try and accepts the second: p_2 has no wrong decision in field 1, so "A ? ?" ranks
    # in front of "A B ?"; its hard errors count field 2's positions too
    st = state()
    put(st, 8, 1, p2["a"], 0, 0, stamp=10)
    put(st, 7, 3, p2["a"], p2["b"], 0, stamp=10)
    add("first_try_refused_by_the_gate", st, tries=2, hard=int(p2["nhard"]))
    add("both_tries_refused_by_the_gate", st, tries=2, hard=max(int(p2["nhard"]) - 1, 0))
    # a first try that ends in 3, 4 or 8 in front of the accepted "A B ?": the entries of q_3, q_4 and q_8 in one table
    q3, q4, q8 = by["q_3"], by["q_4"], by["q_8"]
    st = state()
    put(st, 10, 1, q3["x"], 0, 0, stamp=10)
    put(st, 11, 1, q4["x"], 0, 0, stamp=10)
    put(st, 12, 1, q8["x"], 0, 0, stamp=10)
    put(st, 13, 3, q3["a"], q3["b"], 0, stamp=10)
    add("first_try_3_4_8_then_accepted", st, tries=2, gate=32)
    add("first_try_3_4_8_alone", st, tries=1, gate=32)
    # the CQ field as a kind 1 entry: ap_craft's a_* (CQ messages BP misses), c_wrong_crc (3) and d_unpack_refuses
    st = state()
    put(st, 500, 1, 2 << 1, 0, 0, stamp=10)
    add("cq_as_a_hint", st, tries=1, gate=64)
    return out


def build(oracle, seed=0x417):
    """(cases, frames, mag, configs)"""
    cases = build_cases(oracle)
    frames = oc.build_frames(cases, seed=seed)
    mag = oc.waterfalls(oc.vectors_of(cases), frames)
    return cases, frames, mag, configs(cases)


def states_for(st, B):
    return np.repeat(np.asarray(st, sh.STATE_DTYPE).reshape(1), B)


def expected(oracle, frames, mag, cfgs, cache=None):
    """{name: (status_out in place, info)} from the restatement"""
    cache = {} if cache is None else cache
    B = len(frames["counts"])
    out = {}
    for name, st, tries, gate, hard, max_age, use_phase in cfgs:
        out[name] = sh.hint_candidates(oracle, mag, frames["cands"], frames["counts"], frames["status_in"], states_for(st, B), tries, gate,
                                       hard, max_age, use_phase, status_out=frames["status_in"], iters=ITERS, cache=cache)
    return out


def load_golden(path=GOLDEN):
    d = dict(np.load(path))
    B = len(d["counts"])
    d["cands"] = d["cands"].view(oc.CAND_DTYPE).reshape(B, -1)
    d["names"] = [str(n) for n in d["names"]]
    d["states"] = d["states"].view(sh.STATE_DTYPE).reshape(-1)
    return d


def golden_status(d, k):
    """the expected status_out (in place on status_in) of configuration k of the frozen fixture"""
    st = np.array(d["status_in"], copy=True)
    hit = d[f"rewritten_{k}"]
    st[hit[:, 0], hit[:, 1]] = d[f"status_{k}"]
    return st


# ---- the update rule on fabricated records -----------------------------------------------------------------------------------

def records_of(layout):
    """layout [R][S] of text lists (or (texts, count)) -> (msgs [R][S][50] with a91 set, n_msgs [R][S])"""
    import rtlsdr_ft8d_amd as ft8
    R, S = len(layout), max(len(r) for r in layout)
    msgs = np.zeros((R, S, 50), ft8.MESSAGE_DTYPE)
    n = np.zeros((R, S), np.int32)
    for r, row in enumerate(layout):
        for s, cell in enumerate(row):
            texts, count = cell if isinstance(cell, tuple) else (cell, len(cell))
            for k, t in enumerate(texts[:50]):
                msgs[r, s, k]["a91"][:10] = ft8.pack77(t) if isinstance(t, str) else t
            n[r, s] = count
    return msgs, n


def update_layout(seed=0x0DD):
    """texts per [receiver][slot], 3 x 12: every message type, tokens and hashed calls in either field, /R flags, repeats that
    refresh, counts outside [0, 50], and a receiver whose 45 records per slot wrap the ring past 512"""
    import synth_util as su
    rng = np.random.default_rng(seed)
    r0 = [["CQ K1ABC FN42", "K1ABC W9XYZ EM48", "W9XYZ K1ABC -11"],
          ["K1ABC W9XYZ R-09", "W9XYZ K1ABC RRR", "CQ DX K1JT FN20", "K1ABC/R W9XYZ EM48", "K1ABC W9XYZ/R R EM48"],
          [],
          ["K1ABC W9XYZ 73", "CQ K1ABC FN42", "<K1ABC> W9XYZ -05", "W9XYZ <PJ4/K1ABC> RRR", "K1ABC/P W9XYZ/P EM48", "TNX BOB 73 GL",
           "0123456789ABCDEF01", "<W9XYZ> PJ4/K1ABC RR73", "CQ PJ4/K1ABC", "QRZ K1JT FN20", "DE K1JT FN20", "CQ 123 K1JT FN20"],
          ([su.random_message(rng, cq=k % 2 == 0) for k in range(8)], 70),
          ([su.random_message(rng, cq=False) for _ in range(5)], -3),
          ["K1ABC W9XYZ R-09"], [], ["W9XYZ K1ABC -11"], ["CQ K1ABC FN42"], [], ["K1ABC W9XYZ EM48"]]
    r1 = [[su.random_message(rng, cq=False) for _ in range(45)] for _ in range(12)]
    r2 = [["K1ABC W9XYZ RR73"], ["W9XYZ K1ABC -11"], ["K1ABC W9XYZ RR73"], [], ["W9XYZ K1ABC -11"], ["DL1ABC G4XYZ JO62"],
          [], [], ["DL1ABC G4XYZ JO62"], ["G4XYZ DL1ABC -01"], ["K1ABC W9XYZ RR73"], []]
    return [r0, r1, r2]


# ---- the stream scenario -------------------------------------------------------------------------------------------------------

STEPS = 5


def qso_step(a, b, grid, rpt, step):
    """step 0..4 of a QSO that A opens: CQ, B's call, A's report, B's R-report, A's RR73"""
    return (f"CQ {a} {grid[0]}", f"{a} {b} {grid[1]}", f"{b} {a} {rpt[0]}", f"{a} {b} R{rpt[1]}", f"{b} {a} RR73")[step]


def scenario(oracle, seed=0, R=3, S=4, nsig=12):
    """(iq float32 [R][S][2][48000], texts [R][S]): nsig QSOs per receiver on disjoint audio lanes; QSO k is at step
    (k % 2) + s in slot s, the first two slots well above BP's threshold, the later ones at -23 .. -17 dB"""
    import rtlsdr_ft8d_amd as ft8
    import synth_util as su
    iq = np.zeros((R, S, 2, su.NSAMPLES), np.float32)
    texts = [[None] * S for _ in range(R)]
    for r in range(R):
        rng = np.random.default_rng(4000 + 1000 * seed + r)
        pairs = []
        while len(pairs) < nsig:
            t = su.random_message(rng, cq=False).split()
            if "/" not in t[0] + t[1] and "<" not in t[0] + t[1] and t[0] != t[1]:
                pairs.append((t[0], t[1]))
        grids = [(su.random_message(rng, cq=True).split()[-1], su.random_message(rng, cq=True).split()[-1]) for _ in range(nsig)]
        rpts = [("%+03d" % rng.integers(-20, 5), "%+03d" % rng.integers(-20, 5)) for _ in range(nsig)]
        f0 = 100.0 + np.sort(rng.permutation(22)[:nsig]) * 62.5         # disjoint lanes: eight tones of 6.25 Hz and a gap
        t0 = rng.uniform(0.2, 0.8, nsig)
        for s in range(S):
            db = rng.uniform(-12.0, 0.0, nsig) if s < 2 else rng.uniform(-23.0, -17.0, nsig)
            tx = [qso_step(pairs[k][0], pairs[k][1], grids[k], rpts[k], (k % 2) + s) for k in range(nsig)]
            noise = np.random.default_rng(88000 + 100 * seed + 10 * r + s)
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
