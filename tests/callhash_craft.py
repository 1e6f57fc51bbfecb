"""Message records made to order for the call hash table (tests only): no radio path.  A record's a91 comes from the library's
packer ft8gpu_pack77 (host C), which packs <CALL> fields and type 4; its text is what the oracle's unpack77 prints for those
bits ("<...>" for every hashed call); every other byte of the record, the CRC bits of a91 and every record at or above a
frame's count are junk.  tests/golden/make_callhash_golden.py freezes build_cases() in tests/golden/callhash_cases.npz.

A case is dict(name, msgs [R][S][50], n_msgs [R][S], state [R] entry state, max_age); the expected outputs are the restatement's
(tests/ft8_spec_callhash.py).  The cases, by the numbers of the test list in DESIGN.md "Call hash table":
  1 basic        a call heard in slot 0 resolves in slot 1; a hashed record at index 0 against a full call at index 7
  2 type4        both iflip values, RRR / RR73 / 73, icq (inserts, no lookup)
  3 collide_*    two calls with equal 12-bit and different 22-bit hashes, within a slot (by record order and by field order)
                 and across slots; two calls with equal 22-bit hashes
  4 age_*        max_age 0 / 1 / 2 at ages 0 .. 3; an entry state with slot = 0xFFFFFFFE
  5 chain        3 receivers x 4 slots of mixed traffic (the tests cut it into calls and permute the receivers)
  6 counts       counts 0, 50, 51 and -1
  7 long         both fields hashed, an 11-character call, /R and /P, the 34-character text
  8 plain        free text and telemetry"""
import numpy as np

import ft8_spec_callhash as sc
import ft8_spec_pack as sp

MAX_MESSAGES = 50
LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
JUNK = 0xC3


def message_dtype():
    import rtlsdr_ft8d_amd as ft8
    return ft8.MESSAGE_DTYPE


def record(oracle, rng, text):
    """one 64-byte record: junk, then a91 = pack77(text) with junk behind bit 76, and the text the unpacker prints for it"""
    import rtlsdr_ft8d_amd as ft8
    rec = np.frombuffer(rng.integers(0, 256, 64, dtype=np.uint8).tobytes(), ft8.MESSAGE_DTYPE).copy()
    p = ft8.pack77(text)
    a91 = rng.integers(0, 256, 12, dtype=np.uint8)
    a91[:10] = p
    a91[9] = (p[9] & 0xF8) | (a91[9] & 0x07)
    rc, printed = oracle.unpack77(p.tobytes())
    assert rc == 0, text
    rec["a91"][0] = a91
    rec["text"][0] = printed.encode()
    return rec[0], printed


def frames(oracle, layout, seed):
    """layout[r][s] = the texts of receiver r's slot s, or (texts, count) to give the frame another count than len(texts)
    -> (msgs [R][S][50], n_msgs [R][S], printed texts [r][s][k])"""
    rng = np.random.default_rng(seed)
    R, S = len(layout), len(layout[0])
    msgs = np.frombuffer(rng.integers(0, 256, R * S * MAX_MESSAGES * 64, dtype=np.uint8).tobytes(), message_dtype()).copy()
    msgs = msgs.reshape(R, S, MAX_MESSAGES)
    n_msgs = np.zeros((R, S), np.int32)
    printed = [[[] for _ in range(S)] for _ in range(R)]
    for r in range(R):
        assert len(layout[r]) == S
        for s in range(S):
            cell = layout[r][s]
            texts, count = cell if isinstance(cell, tuple) else (cell, len(cell))
            n_msgs[r, s] = count
            for k, t in enumerate(texts):
                msgs[r, s, k], shown = record(oracle, rng, t)
                printed[r][s].append(shown)
    return msgs, n_msgs, printed


def random_call(rng):
    """a standard call sign"""
    pfx = rng.choice(["K", "W", "N", "G", "F", "DL", "JA", "VK", "EA", "OH"])
    return pfx + str(rng.integers(0, 10)) + "".join(rng.choice(list(LETTERS), size=rng.integers(1, 4)))


def colliding_pairs(seed=0xC0, limit=20000):
    """((a, b) with equal 12-bit and different 22-bit hashes, (c, d) with equal 22-bit hashes), distinct standard calls from a
    seeded stream; the numbers of calls drawn until each kind appeared"""
    rng = np.random.default_rng(seed)
    by12, by22, seen = {}, {}, set()
    pair12 = pair22 = None
    drawn12 = drawn22 = 0
    for drawn in range(1, limit + 1):
        c = random_call(rng)
        if c in seen:
            continue
        seen.add(c)
        h22 = sp.call_hash(c, 22)
        if pair22 is None and h22 in by22:
            pair22, drawn22 = (by22[h22], c), drawn
        if pair12 is None and (h22 >> 10) in by12 and sp.call_hash(by12[h22 >> 10], 22) != h22:
            pair12, drawn12 = (by12[h22 >> 10], c), drawn
        by22.setdefault(h22, c)
        by12.setdefault(h22 >> 10, c)
        if pair12 and pair22:
            return pair12, pair22, drawn12, drawn22
    raise AssertionError("no colliding calls found")


LONG_A, LONG_B = "VP2E/W1ABCD", "PJ4/K1ABC/P"           # 11 characters each


def _case(oracle, name, layout, seed, max_age=0, slot0=0):
    msgs, n_msgs, printed = frames(oracle, layout, seed)
    state = sc.new_state(len(layout))
    state["slot"] = slot0
    return dict(name=name, msgs=msgs, n_msgs=n_msgs, state=state, max_age=max_age, printed=printed)


def chain_layout(seed=0x5EED, R=3, S=4):
    """mixed traffic: full calls, hashed fields of calls heard earlier, now, later or never, type 4 both ways, free text"""
    rng = np.random.default_rng(seed)
    layout = []
    for r in range(R):
        calls = [random_call(rng) for _ in range(6)]
        longs = ["PJ4/" + calls[0], calls[1] + "/QRP", "KH1/" + calls[2]]
        slots = []
        for s in range(S):
            texts = []
            for _ in range(int(rng.integers(3, 12))):
                kind = int(rng.integers(0, 8))
                a, b, l = calls[rng.integers(0, 6)], calls[rng.integers(0, 6)], longs[rng.integers(0, 3)]
                texts.append([f"CQ {a} FN42", f"{a} {b} -07", f"<{l}> {a} R-12", f"{a} <{l}> RR73", f"<{a}> {l} RRR",
                              f"{l} <{b}>", f"CQ {l}", "TNX 73 GL"][kind])
            slots.append(texts)
        layout.append(slots)
    return layout


def build_cases(oracle):
    (a12, b12), (a22, b22), _, _ = colliding_pairs()
    cases = []
    add = lambda *a, **k: cases.append(_case(oracle, *a, **k))
    filler = ["CQ W9XYZ EN37", "N0CAL K9AN -15", "TNX BOB 73 GL", "CQ DX G4ABC IO91", "K1JT W1AW FN31", "CQ 123 JA1ZZZ PM95"]
    # 1
    add("basic", [[["CQ K1ABC FN42", "CQ PJ4/K1ABC"], ["<K1ABC> PJ4/W1AW RR73", "<PJ4/K1ABC> W9XYZ -11", "<PJ4/W9XYZ> K1ABC R-03"]],
                  [["<KH1/KH7Z> K1ABC -09"] + filler + ["CQ KH1/KH7Z", "<KH1/KH7Z> W1AW 73"], ["KH7Z <KH1/KH7Z> RRR"]]], 1)
    # 2
    add("type4", [[["CQ K1ABC FN42", "<K1ABC> PJ4/K1ABC", "PJ4/K1ABC <K1ABC>", "<K1ABC> PJ4/K1ABC RRR", "PJ4/K1ABC <K1ABC> RR73",
                    "<K1ABC> PJ4/K1ABC 73", "PJ4/K1ABC <W9XYZ> 73", "CQ KH1/KH7Z", "W1AW <KH1/KH7Z> RRR"],
                   ["<KH1/KH7Z> PJ4/K1ABC RR73", "<W1AW> KH1/KH7Z", "CQ W1AW/QRP"]]], 2)
    # 3
    look12 = lambda c: f"<{c}> PJ4/W1AW RR73"
    look22 = lambda c: f"<{c}> W9XYZ -11"
    add("collide_12_record_order", [[[look12(a12), look22(a12), look22(b12), f"CQ {a12} FN42", f"CQ {b12} FN42"]],
                                    [[look12(a12), look22(a12), look22(b12), f"CQ {b12} FN42", f"CQ {a12} FN42"]]], 3)
    add("collide_12_field_order", [[[f"{a12} {b12} -07", look12(a12), look22(a12), look22(b12)]],
                                   [[f"{b12} {a12} -07", look12(a12), look22(a12), look22(b12)]]], 4)
    add("collide_12_across_slots", [[[f"CQ {a12} FN42", look22(a12)], [f"CQ {b12} FN42", look12(a12), look22(a12), look22(b12)],
                                     [look12(b12), look22(a12), f"CQ {a12} FN42"]]], 5)
    add("collide_22", [[[f"CQ {a22} FN42", look22(a22), look12(a22)], [f"CQ {b22} FN42", look22(a22), look22(b22), look12(b22)],
                        [f"{b22} {a22} 73", look22(b22)]]], 6)
    # 4: heard in slot 0, asked for at ages 0 .. 3
    ask = ["<K1ABC> PJ4/W1AW RR73", "<PJ4/K1ABC> W9XYZ -11"]
    aged = [[["CQ K1ABC FN42", "CQ PJ4/K1ABC"] + ask, ask, ask, ask]]
    for max_age in (0, 1, 2):
        add(f"age_{max_age}", aged, 7, max_age=max_age)
        add(f"age_{max_age}_wrap", aged, 7, max_age=max_age, slot0=0xFFFFFFFE)
    # 5
    add("chain", chain_layout(), 8)
    # 6
    fifty = [f"CQ {random_call(np.random.default_rng(600 + k))} FN42" for k in range(24)] + \
            [f"<PJ4/K1ABC> {random_call(np.random.default_rng(700 + k))} -11" for k in range(25)] + ["CQ PJ4/K1ABC"]
    add("counts", [[(["CQ K1ABC FN42", "<K1ABC> PJ4/W1AW 73"], 0), (fifty, 50), (fifty, 51), (["CQ W1AW FN31"], -1),
                    ["<K1ABC> PJ4/W1AW 73", "<PJ4/K1ABC> W1AW 73", "<W1AW> PJ4/W1AW"]]], 9)
    # 7
    add("long", [[[f"CQ {LONG_A}", f"CQ {LONG_B}", f"<{LONG_A}> <{LONG_B}> R FN20", f"<{LONG_B}> <{LONG_A}> RR73",
                   "K1ABC/R W9XYZ EN37", "W1AW K9AN/P -05", "<K1ABC> PJ4/W1AW", "<K9AN> PJ4/W1AW", "<PJ4/W1AW> K1ABC/R R FN42",
                   f"<{LONG_A}> <K1NOT> R FN20", f"<K1NOT> <{LONG_B}> 73", f"W9XYZ <{LONG_A}> -30"]]], 10)
    # 8
    add("plain", [[["TNX BOB 73 GL", "123456789ABCDEF012", "CQ K1ABC FN42", "0F00000000000000FF", "A", "+-./? 0Z"]]], 11)
    return cases


def expected(case):
    """the restatement's (resolved, exit state) of a case, on resolved records prefilled with JUNK"""
    pre = np.frombuffer(np.full(case["msgs"].size * 48, JUNK, np.uint8).tobytes(), sc.RESOLVED_DTYPE).reshape(case["msgs"].shape)
    return sc.resolve(case["msgs"], case["n_msgs"], case["state"], case["max_age"], pre)


def load_golden(path=None):
    """the frozen cases of tests/golden/callhash_cases.npz: [dict(name, msgs, n_msgs, state, max_age, resolved, state_out)]"""
    import os
    d = np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "callhash_cases.npz"))
    out = []
    for name, max_age in zip(d["names"], d["max_age"]):
        n_msgs = d[f"n_msgs_{name}"]
        R, S = n_msgs.shape
        state = sc.new_state(R)
        state["slot"] = d[f"slot0_{name}"]
        out.append(dict(name=str(name), msgs=d[f"msgs_{name}"].view(message_dtype()).reshape(R, S, MAX_MESSAGES), n_msgs=n_msgs,
                        state=state, max_age=int(max_age),
                        resolved=d[f"resolved_{name}"].view(sc.RESOLVED_DTYPE).reshape(R, S, MAX_MESSAGES),
                        state_out=d[f"state_{name}"].view(sc.STATE_DTYPE).reshape(R)))
    return out
