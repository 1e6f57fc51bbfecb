"""Soft bits made to order for a-priori decoding (tests only): the constructed cases of DESIGN.md "A-priori decoding" on top
of tests/osd_craft.py, whose write_candidate() makes ft8_extract_likelihood return any 174 integers a test chooses and whose
build_frames() places them with fabricated status records.

  a  a CQ codeword in noise that BP misses in 20 iterations and the "CQ ? ?" hypothesis recovers ("CQ DX ? ?" for a CQ DX
     message); judged at the gate equal to its hard errors (accepted) and one below (result 2, record untouched)
  b  a codeword that is no CQ message, clean, with three sign flips, and in noise: under "CQ ? ?" no codeword is reached
     (result 7); under a hypothesis that has one bit of its first call field wrong BP overturns the forced bit and
     converges on the codeword (result 8)
  c  a valid codeword with the CQ bits and a wrong CRC (result 3)
  d  a payload unpack77 refuses, with its own CRC, under a hypothesis that masks all 77 of its bits (result 4)
  e  an all-zero hypothesis on all-negative soft bits: bp_decode leaves at the all-zero word, "no codeword" (result 7)
  f  unusable soft bits: all zero (NaN after the normalisation), constant (+-infinity), every symbol outside blocks 0..91
     (result 6); one candidate with only its head outside, which is decoded
  s  a random sweep
The configurations (hypothesis table, gate) are derived from the cases; tests/test_ap_cpu.py proves with the oracle that
each case is what it is named for."""
import numpy as np

import ft8_spec_ap as sa
import ft8_spec_decode as sd
import ft8_spec_osd as so
import osd_craft as oc

CAP = oc.CAP
FILL = oc.FILL
ITERS = 20
SWEEP = 24
A_TEXTS = (("CQ K1ABC FN42", "CQ ? ?"), ("CQ W9XYZ EM48", "CQ ? ?"), ("CQ DX K1JT FN20", "CQ DX ? ?"))   # message, recovering pattern
B_TEXT = "K1ABC W9XYZ -11"


def llr_of(v):
    """the normalised soft bits of integer raw soft bits (sums of small integers are exact in any order)"""
    return sd.normalize_logl(np.asarray(v, np.float32))


def _payload_bits(oracle, text):
    """the 77 bits of a standard message, "CQ DX CALL GRID" included (tests/ft8_spec_pack.py)"""
    import ft8_spec_pack as sp
    tok = text.split()
    if len(tok) == 4:
        tok = [tok[0] + " " + tok[1]] + tok[2:]
    return np.unpackbits(np.frombuffer(sp.pack_standard(*tok), np.uint8))[:77]


def _noisy(rng, cw, amp, sigma):
    x = np.where(cw == 1, amp, -amp) + rng.normal(0.0, sigma, 174)
    v = np.clip(np.rint(x), -255, 255).astype(np.int16)
    v[v == 0] = 1
    return v


def _case_a(cases, oracle):
    for k, (text, pattern) in enumerate(A_TEXTS):
        hyp = sa.from_text(pattern)
        cw = oc._payload_codeword(_payload_bits(oracle, text))
        rng = np.random.default_rng(0xA0 + k)
        for trial in range(4000):
            v = _noisy(rng, cw, 20.0, 27.0 + (trial % 5))
            llr = llr_of(v)
            if oracle.bp_decode(llr, ITERS)[1] == 0:
                continue
            tried = sa.attempts(oracle, llr, [hyp], ITERS)
            info, win = sa.resolve(oracle, llr, tried, 174)
            if win is not None and np.array_equal(win[0], cw):
                break
        else:
            raise AssertionError("no vector that BP misses and AP recovers: " + text)
        cases.append(dict(case="a", name=f"a_{k}", v=v, text=text, pattern=pattern, codeword=cw, nhard=int(info["nhard"])))


def _case_b(cases, oracle):
    cw = oc._payload_codeword(_payload_bits(oracle, B_TEXT))
    rng = np.random.default_rng(0xB)
    cases.append(dict(case="b", name="b_clean", v=oc._signed(cw, rng.integers(100, 181, 174)), codeword=cw, result=7))
    cases.append(dict(case="b", name="b_flips", v=_flipped(rng, oc._signed(cw, rng.integers(100, 181, 174)), 3), codeword=cw, result=7))
    cases.append(dict(case="b", name="b_noise", v=_noisy(rng, cw, 12.0, 30.0), codeword=cw, result=7))


def _flipped(rng, v, n):
    v = v.copy()
    at = rng.choice(np.arange(77, 174), n, replace=False)
    v[at] = -np.sign(v[at]) * rng.integers(1, 5, n)
    return v


def _case_cd(cases, oracle):
    rng = np.random.default_rng(0xC)
    m, b = sa.mask_and_bits(sa.cq_hypothesis())
    bits = rng.integers(0, 2, 77).astype(np.uint8)
    bits[m[:77]] = b[:77][m[:77]]
    crc = so.crc14(bits) ^ 0x0001
    info = np.concatenate([bits, [(crc >> (13 - i)) & 1 for i in range(14)]]).astype(np.int64)
    cw = ((info @ so.generator_matrix().astype(np.int64)) & 1).astype(np.uint8)
    cases.append(dict(case="c", name="c_wrong_crc", v=oc._signed(cw, rng.integers(60, 200, 174)), codeword=cw, result=3))
    for _ in range(64):
        bits = rng.integers(0, 2, 77).astype(np.uint8)
        rc, _text = oracle.unpack77(np.packbits(np.concatenate([bits, np.zeros(3, np.uint8)])).tobytes())
        if rc < 0:
            break
    else:
        raise AssertionError("no payload that unpack77 refuses")
    cw = oc._payload_codeword(bits)
    cases.append(dict(case="d", name="d_unpack_refuses", v=_flipped(rng, oc._signed(cw, rng.integers(20, 200, 174)), 4), codeword=cw,
                      payload=bits, result=4))


def _case_ef(cases):
    rng = np.random.default_rng(0xE)
    cases.append(dict(case="e", name="e_all_negative", v=(-rng.permutation(np.arange(1, 256))[:174]).astype(np.int16), result=7))
    cases.append(dict(case="f", name="f_all_zero", v=np.zeros(174, np.int16), result=6))
    cases.append(dict(case="f", name="f_all_minus_7", v=np.full(174, -7, np.int16), result=6))
    cases.append(dict(case="f", name="f_all_plus_255", v=np.full(174, 255, np.int16), result=6))
    v = (rng.integers(1, 200, 174) * rng.choice([-1, 1], 174)).astype(np.int16)
    cases.append(dict(case="f", name="f_past_the_end", v=v, time_offset=92, result=6))
    cases.append(dict(case="f", name="f_before_the_start", v=v, time_offset=-80, result=6))
    cases.append(dict(case="f", name="f_head_outside", v=v, time_offset=-12))


def _case_s(cases, n=SWEEP):
    rng = np.random.default_rng(0x5)
    edge = (-12, -10, 21, 24)
    for i in range(n):
        kind = i % 3
        if kind == 0:
            v = rng.integers(0, 3, 174)
        elif kind == 1:
            v = rng.integers(0, 256, 174)
        else:
            v = rng.integers(0, 4, 174)
            big = rng.choice(174, int(rng.integers(1, 9)), replace=False)
            v[big] = rng.integers(30, 256, len(big))
        c = dict(case="s", name=f"s_{i}", v=(v * rng.choice([-1, 1], 174)).astype(np.int16))
        if i % 4 == 3:
            c["time_offset"] = edge[(i // 4) % len(edge)]
        cases.append(c)


# ---- radio frames ------------------------------------------------------------------------------------------------------------
# Eight of the 20-signal CQ frames of seeds 1000..1031 (SNR U[-22, 0] dB), picked on the CPU with tools/ap_gain.py's per-frame
# figures: on six of them "CQ ? ?" gains a planted message over BP, on 1018 BP converges under the hypothesis on a word that
# is no planted codeword, on 1026 nothing converges.
RADIO_SEEDS = (1000, 1001, 1004, 1007, 1012, 1014, 1018, 1026)
NOISE_SEEDS = tuple(range(5000, 5008))


def radio_frames(oracle, seeds=RADIO_SEEDS, nsig=20, snr=(-22.0, 0.0)):
    """(iq [B][2][48000], planted texts per frame)"""
    import synth_util as S
    enc = S.oracle_encode_fn(oracle)
    fr = [S.make_frame(s, nsig, enc, snr_range=snr) for s in seeds]
    return np.stack([f[0] for f in fr]), [f[1] for f in fr]


_cases = []


def build_cases(oracle):
    if not _cases:
        cases = []
        _case_a(cases, oracle)
        _case_b(cases, oracle)
        _case_cd(cases, oracle)
        _case_ef(cases)
        _case_s(cases)
        for c in cases:
            c["v"] = np.array(c["v"], np.int16)
            c["v"].setflags(write=False)
        _cases.extend(cases)
    return _cases


def one_bit_hypothesis():
    m = np.zeros(77, np.uint8)
    m[76] = 1
    return sa.hypothesis(m, m)                           # the last bit of i3 = 1


def b_one_wrong_hypothesis(codeword):
    """the first call field of case b's message (bits 0..28) with bit 5 inverted: BP has one forced bit to overturn"""
    m = np.zeros(77, np.uint8)
    m[:29] = 1
    b = np.array(codeword[:77], np.uint8)
    b[5] ^= 1
    return sa.hypothesis(m, b)


def configs(cases):
    """[(name, hypotheses, gate)]: the hypothesis tables and gates the constructed cases are judged at"""
    by = {c["name"]: c for c in cases}
    cq, cqdx = sa.cq_hypothesis(), sa.from_text("CQ DX ? ?")
    ones = np.ones(77, np.uint8)
    out = [("cq", [cq], 174)]
    for k in range(len(A_TEXTS)):
        e, pattern = by[f"a_{k}"]["nhard"], by[f"a_{k}"]["pattern"]
        tag = "cq" if pattern == "CQ ? ?" else "cqdx"
        out += [(f"{tag}_gate_{e}", [sa.from_text(pattern)], e), (f"{tag}_gate_{e - 1}", [sa.from_text(pattern)], e - 1)]
    out += [("cqdx_cq", [cqdx, cq], 174), ("cq_cqdx", [cq, cqdx], 174),
            ("four", [sa.from_text("K1ABC ? ?"), sa.from_text("CQ POTA ? ?"), cqdx, cq], 174),
            ("d_all_77", [sa.hypothesis(ones, by["d_unpack_refuses"]["payload"])], 174),
            ("a0_all_77", [sa.hypothesis(ones, by["a_0"]["codeword"][:77])], 174),
            ("zero_all_77", [sa.hypothesis(ones, np.zeros(77, np.uint8))], 174),
            ("b_one_wrong", [b_one_wrong_hypothesis(by["b_clean"]["codeword"])], 174),
            ("one_bit", [one_bit_hypothesis()], 174), ("cq_gate_0", [cq], 0)]
    seen, uniq = set(), []
    for name, hyps, gate in out:
        if name not in seen:
            seen.add(name)
            uniq.append((name, hyps, gate))
    return uniq


def hyps_array(hyps):
    a = np.zeros(len(hyps), sa.HYP_DTYPE)
    for k, h in enumerate(hyps):
        a[k] = h
    return a


def build(oracle, seed=0xA9):
    """(cases, frames, mag, configs): the cases placed by osd_craft.build_frames (fabricated status records, ragged counts, a
    frame without candidates), their waterfalls, and the configurations"""
    cases = build_cases(oracle)
    frames = oc.build_frames(cases, seed=seed)
    mag = oc.waterfalls(oc.vectors_of(cases), frames)
    return cases, frames, mag, configs(cases)


def fixture_status(d, name):
    """the expected status_out (in place on status_in) of the frozen fixture d (tests/golden/ap_constructed.npz) at a configuration"""
    st = np.array(d["status_in"], copy=True)
    hit = d[f"rewritten_{name}"]
    st[hit[:, 0], hit[:, 1]] = d[f"status_{name}"]
    return st
