"""CPU tests of a-priori decoding: ft8gpu_ap_from_text against tests/ft8_spec_pack.py; the restatement of the rule
(tests/ft8_spec_ap.py) on radio frames -- it gains planted messages over BP and accepts nothing outside the planted set, on
noise frames either -- and on the constructed soft bits of tests/ap_craft.py, where each case is proven with the oracle to be
what it is named for, the oracle's bp_decode is held against the numpy writing of tests/ft8_spec_decode.py, and the frozen
fixture tests/golden/ap_constructed.npz (which the device is held to as well) is reproduced."""
import os

import numpy as np
import pytest

import ap_craft as ac
import ft8_spec_ap as sa
import ft8_spec_osd as so
import osd_craft as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ("CQ ? ?", "CQ DX ? ?", "CQ POTA ? ?", "CQ 123 ? ?", "K1ABC ? ?", "K1ABC W9XYZ ?", "? W9XYZ ?", "? ? RR73", "? W9XYZ FN42",
            "CQ K1ABC FN42", "CQ DX K1JT FN20", "DE ? ?", "QRZ ? ?", "K1ABC/R ? ?", "? ? -11", "? ? ?")
REFUSED = ("", "CQ", "CQ ?", "CQ DX ?", "? ? ? ?", "CQ DX ? ? ?", "K1ABC/P ? ?", "HELLO ? ?", "K1ABC W9XYZ R FN42", "CQ ? ? ?",
           "K1ABC ? HELLO", "? TOOLONGCALL ?", "CQ ?? ?")


def test_ap_from_text_equals_the_packer_restatement():
    import rtlsdr_ft8d_amd as ft8
    for p in PATTERNS:
        got, want = ft8.ap_from_text(p), sa.from_text(p)
        assert got.tobytes() == want.tobytes(), (p, bytes(got["mask"]).hex(), bytes(want["mask"]).hex())
        assert sa.validate([got])
    # a whole message: every bit masked, the bits are the packer's
    full = ft8.ap_from_text("CQ K1ABC FN42")
    assert bytes(full["bits"]) == bytes(ft8.pack77("CQ K1ABC FN42")) and np.unpackbits(full["mask"]).sum() == 77
    # the hypothesis agrees with every message the pattern stands for
    for msg, pat in (("CQ W9XYZ EM48", "CQ ? ?"), ("CQ DX K1JT FN20", "CQ DX ? ?"), ("K1ABC W9XYZ -11", "K1ABC ? ?"),
                     ("K1ABC W9XYZ RR73", "K1ABC W9XYZ ?"), ("K1ABC W9XYZ RR73", "? ? RR73")):
        h, payload = ft8.ap_from_text(pat), ft8.pack77(msg)
        assert np.array_equal(payload & h["mask"], h["bits"]), (msg, pat)


def test_cq_pattern_is_exactly_the_32_constant_bits():
    import rtlsdr_ft8d_amd as ft8
    h = ft8.ap_from_text("CQ ? ?")
    mask = np.unpackbits(h["mask"])
    assert np.flatnonzero(mask).tolist() == list(range(0, 29)) + [74, 75, 76]
    assert np.flatnonzero(np.unpackbits(h["bits"])).tolist() == [26, 76]          # the call field's value 2, i3 = 1
    assert h.tobytes() == sa.cq_hypothesis().tobytes()


def test_ap_from_text_refusals():
    import ctypes as C
    import rtlsdr_ft8d_amd as ft8
    for p in REFUSED:
        with pytest.raises(ValueError):
            ft8.ap_from_text(p)
    L = ft8.load_library()
    out = np.full(20, 0xA5, np.uint8)
    assert L.ft8gpu_ap_from_text(b"CQ ?", out.ctypes.data) == -1 and (out == 0xA5).all()          # refused: out untouched
    assert L.ft8gpu_ap_from_text(None, out.ctypes.data) == -1 and L.ft8gpu_ap_from_text(b"CQ ? ?", None) == -1
    assert L.ft8gpu_ap_from_text(b"CQ ? ?" + b" " * 40, out.ctypes.data) == -1


# ---- radio frames ------------------------------------------------------------------------------------------------------------

def _accepted_texts(ft8, st, info, counts):
    out = []
    for f in range(len(counts)):
        recs = st[f].view(ft8.STATUS_DTYPE).reshape(-1)
        out.append([recs[i]["text"].decode() for i in range(int(counts[f])) if info[f, i]["result"] == 1])
    return out


def test_restatement_on_radio_frames_gains_and_accepts_nothing_outside(oracle):
    """the chosen frames (ap_craft.RADIO_SEEDS): AP accepts at least 3 candidates and gains at least 1 planted message over BP
    (here: 29 and 8); everything it accepts is a planted message; on eight noise frames it accepts nothing"""
    import rtlsdr_ft8d_amd as ft8
    import ft8_spec_messages as sm
    import ft8_spec_multipass as mp
    iq, planted = ac.radio_frames(oracle)
    hyps = [sa.cq_hypothesis()]
    mag, cands, counts, status = sm.oracle_stages(oracle, iq, 120, 10, 8)
    st, info = sa.ap_candidates(oracle, mag, cands, counts, status, hyps, 174)
    texts = _accepted_texts(ft8, st, info, counts)
    accepted = sum(len(t) for t in texts)
    bp, n_bp, _ = sa.decode_ap(oracle, iq, 1, [], 174, -1, 0)
    ap, n_ap, nbs = sa.decode_ap(oracle, iq, 1, hyps, 174, -1, 0)
    h_bp, m_bp = mp.planted_hits(bp, n_bp, planted)
    h_ap, m_ap = mp.planted_hits(ap, n_ap, planted)
    print(f"accepted {accepted}, planted {h_bp} -> {h_ap}, outside {m_bp} -> {m_ap}, n_by_stage {nbs[:, 0].tolist()}")
    assert accepted >= 3 and h_ap - h_bp >= 1                         # the test is not vacuous
    assert all(t in planted[f] for f in range(len(texts)) for t in texts[f]) and m_ap == m_bp == 0
    assert np.array_equal(nbs[:, 0, 0], n_bp) and np.array_equal(nbs[:, 0, 1], n_ap) and np.array_equal(nbs[:, 0, 2], n_ap)
    for f in range(len(iq)):                                           # BP's records first, then AP's, tagged 1 + hyp
        assert ap[f, :n_bp[f]].tobytes() == bp[f, :n_bp[f]].tobytes()
        assert (ap[f, n_bp[f]:n_ap[f]]["pad"][:, 1] == 1).all() and not ap[f, :n_bp[f]]["pad"].any()
    # the recommended gate loses none of them
    st40, info40 = sa.ap_candidates(oracle, mag, cands, counts, status, hyps, ft8.AP_MAX_HARD_ERRORS)
    assert st40.tobytes() == st.tobytes()
    # results seen on radio frames: accepted, no codeword, and (frame 1018) a wrong codeword the CRC stops
    seen = set(int(r) for f in range(len(iq)) for r in info[f, :counts[f]]["result"])
    assert {0, 1, 3, 7} <= seen, seen
    noise, _ = ac.radio_frames(oracle, ac.NOISE_SEEDS, 0)
    mag, cands, counts, status = sm.oracle_stages(oracle, noise, 120, 10, 8)
    for hy in (hyps, [sa.cq_hypothesis(), sa.from_text("CQ DX ? ?")]):
        st, info = sa.ap_candidates(oracle, mag, cands, counts, status, hy, 174)
        assert counts.sum() >= 40 and not (info["result"] == 1).any() and st.tobytes() == status.tobytes()


# ---- constructed soft bits -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built(oracle):
    cases, frames, mag, configs = ac.build(oracle)
    want = {name: sa.ap_candidates(oracle, mag, frames["cands"], frames["counts"], frames["status_in"], hyps, gate, iters=ac.ITERS)
            for name, hyps, gate in configs}
    return cases, frames, mag, configs, want


def _at(cases, frames, want, config, name):
    import rtlsdr_ft8d_amd as ft8
    ci = [c["name"] for c in cases].index(name)
    f, i = oc.slots(frames)[ci]
    st, info = want[config]
    return cases[ci], info[f, i], st[f, i].view(ft8.STATUS_DTYPE)[0], frames["status_in"][f, i], (f, i)


def test_constructed_cases_are_what_they_are_named_for(oracle, built):
    import rtlsdr_ft8d_amd as ft8
    cases, frames, mag, configs, want = built
    gates = {name: gate for name, _, gate in configs}
    # (a) BP misses it at 20 iterations, the hypothesis recovers it; the gate on both sides of its hard errors
    for k, (text, pattern) in enumerate(ac.A_TEXTS):
        tag = "cq" if pattern == "CQ ? ?" else "cqdx"
        c, info, rec, rec_in, (f, i) = _at(cases, frames, want, f"{tag}_gate_{cases[k]['nhard']}", f"a_{k}")
        llr = oracle.llr(mag[f], frames["cands"][f, i])
        assert np.array_equal(llr, ac.llr_of(oc.effective(c["v"], frames["cands"][f, i]["time_offset"])))
        plain, errors, it = oracle.bp_decode(llr, ac.ITERS)
        assert errors != 0 and it == ac.ITERS                                   # BP alone: no codeword
        e = c["nhard"]
        assert 1 <= e == gates[f"{tag}_gate_{e}"] and tuple(info)[:3] == (1, e, 0) and 0 < info["iters"] < ac.ITERS
        assert rec["ok"] == 1 and rec["text"].decode() == text and rec["ldpc_errors"] == 0 and rec["pad"] == 0
        assert rec["iters"] == rec_in.view(ft8.STATUS_DTYPE)[0]["iters"] and rec["crc_extracted"] == rec["crc_calculated"]
        assert np.array_equal(np.unpackbits(rec["a91"])[:91], c["codeword"][:91])
        c, info, rec, rec_in, _ = _at(cases, frames, want, f"{tag}_gate_{e - 1}", f"a_{k}")
        assert tuple(info)[:3] == (2, e, 0) and rec.tobytes() == rec_in.tobytes()                 # refused: record untouched
    # (b) no CQ message: 7 under "CQ ? ?"; one forced bit wrong: BP overturns it, 8
    for name in ("b_clean", "b_flips", "b_noise"):
        c, info, rec, rec_in, _ = _at(cases, frames, want, "cq", name)
        assert info["result"] == 7 and info["iters"] == ac.ITERS and rec.tobytes() == rec_in.tobytes()
    for name in ("b_clean", "b_flips"):
        c, info, rec, rec_in, (f, i) = _at(cases, frames, want, "b_one_wrong", name)
        assert info["result"] == 8 and rec.tobytes() == rec_in.tobytes()
        hyp = ac.b_one_wrong_hypothesis(c["codeword"])
        tried = sa.attempts(oracle, oracle.llr(mag[f], frames["cands"][f, i]), [hyp], ac.ITERS)
        plain, errors = tried[0][0], tried[0][1]
        assert errors == 0 and np.array_equal(plain, c["codeword"]) and plain[5] != sa.mask_and_bits(hyp)[1][5]
    # (c) CQ bits, a codeword, a wrong CRC; (d) unpack77 refuses the payload, all 77 bits masked
    c, info, rec, rec_in, _ = _at(cases, frames, want, "cq", "c_wrong_crc")
    assert info["result"] == 3 and rec.tobytes() == rec_in.tobytes()
    assert not ((c["codeword"].astype(np.int32) @ so.parity_check_matrix().T.astype(np.int32)) & 1).any()
    assert so.crc14(c["codeword"][:77]) ^ 1 == int("".join(map(str, c["codeword"][77:91])), 2)
    c, info, rec, rec_in, _ = _at(cases, frames, want, "d_all_77", "d_unpack_refuses")
    assert info["result"] == 4 and info["nhard"] == 4 and rec.tobytes() == rec_in.tobytes()
    assert oracle.unpack77(np.packbits(np.concatenate([c["payload"], np.zeros(3, np.uint8)])).tobytes())[0] < 0
    # (e) the all-zero hypothesis on all-negative soft bits: bp_decode leaves at the all-zero word without checking it --
    # "no codeword", result 7 at iteration 0; result 5 cannot be reached through bp_decode
    c, info, rec, rec_in, (f, i) = _at(cases, frames, want, "zero_all_77", "e_all_negative")
    assert tuple(info)[:4] == (7, 0, 0, 0) and rec.tobytes() == rec_in.tobytes()
    plain, errors, it = oracle.bp_decode(oracle.llr(mag[f], frames["cands"][f, i]), ac.ITERS)
    assert not plain.any() and errors == 83 and it == 0
    assert not any((info_all["result"] == 5).any() for _, info_all in want.values())
    # (f) unusable soft bits: NaN, +-infinity, every symbol outside the waterfall
    kinds = set()
    for name in ("f_all_zero", "f_all_minus_7", "f_all_plus_255", "f_past_the_end", "f_before_the_start"):
        for config in want:
            c, info, rec, rec_in, (f, i) = _at(cases, frames, want, config, name)
            assert info.tobytes() == bytes([6, 0, 0, 0, 0, 0, 0, 0]) and rec.tobytes() == rec_in.tobytes()
        llr = oracle.llr(mag[f], frames["cands"][f, i])
        kinds.add("nan" if np.isnan(llr).all() else ("+inf" if (llr == np.inf).all() else ("-inf" if (llr == -np.inf).all() else "?")))
    assert kinds == {"nan", "+inf", "-inf"}
    assert _at(cases, frames, want, "cq", "f_head_outside")[1]["result"] == 7
    # (g) two hypotheses, only the second accepted; the same pair the other way round
    for k, (first, second) in ((0, ("cqdx_cq", "cq_cqdx")), (2, ("cq_cqdx", "cqdx_cq"))):
        c, info, rec, _, _ = _at(cases, frames, want, first, f"a_{k}")
        assert info["hyp"] == 1 and info["results"][0] not in (0, 1) and info["results"].tolist()[1:] == [1, 0, 0] and rec["ok"] == 1
        c, info2, rec2, _, _ = _at(cases, frames, want, second, f"a_{k}")
        assert info2["hyp"] == 0 and info2["results"].tolist() == [1, 0, 0, 0] and rec2.tobytes() == rec.tobytes()
        assert (info2["nhard"], info2["iters"]) == (info["nhard"], info["iters"])
    c, info, rec, _, _ = _at(cases, frames, want, "four", "a_0")
    assert info["hyp"] == 3 and info["results"].tolist() == [7, 7, 7, 1]
    # (h) a mask of one bit and masks of 77 bits
    assert np.unpackbits(ac.one_bit_hypothesis()["mask"]).sum() == 1
    c, info, rec, _, _ = _at(cases, frames, want, "one_bit", "b_flips")
    assert tuple(info)[:3] == (1, 3, 0) and rec["text"].decode() == ac.B_TEXT
    c, info, rec, _, _ = _at(cases, frames, want, "a0_all_77", "a_0")
    assert info["result"] == 1 and rec["text"].decode() == ac.A_TEXTS[0][0]
    # every code but 5 is seen, and records that do not qualify are copied with an all-zero info
    seen = set(int(r) for _, inf in want.values() for f in range(len(mag)) for r in inf[f, :frames["counts"][f]]["result"])
    assert seen == {0, 1, 2, 3, 4, 6, 7, 8}, seen
    st, info = want["cq"]
    skipped = (frames["vec"] < 0) & (np.arange(oc.CAP)[None, :] < frames["counts"][:, None])
    assert skipped.sum() >= 5 and not info[skipped].view(np.uint64).any() and np.array_equal(st[skipped], frames["status_in"][skipped])


def test_second_writing_of_bp_agrees_on_the_named_cases(oracle, built):
    """the numpy bp_decode of tests/ft8_spec_decode.py in place of the oracle's, on the named cases (the sweep left out: the
    numpy iteration is slow) at two configurations"""
    cases, frames, mag, configs, want = built
    named = [ci for ci, c in enumerate(cases) if c["case"] != "s"]
    where = oc.slots(frames)
    bp = sa.numpy_bp()
    by = {name: (hyps, gate) for name, hyps, gate in configs}
    for config in ("cqdx_cq", "b_one_wrong"):
        hyps, gate = by[config]
        for ci in named:
            f, i = where[ci]
            llr = oracle.llr(mag[f], frames["cands"][f, i])
            info, _ = sa.resolve(oracle, llr, sa.attempts(oracle, llr, hyps, ac.ITERS, bp=bp), gate)
            assert info.tobytes() == want[config][1][f, i].tobytes(), (config, cases[ci]["name"])


def test_validate_refuses_what_the_entry_refuses():
    cq = sa.cq_hypothesis()
    assert sa.validate([cq]) and sa.validate([cq] * 4) and not sa.validate([]) and not sa.validate([cq] * 5)
    bad = cq.copy()
    bad["bits"][1] |= 0x80                               # bit 8 is masked; set bit 40 instead: outside the mask
    assert sa.validate([bad])
    bad["bits"][5] |= 0x01
    assert not sa.validate([bad])
    none = np.zeros(1, sa.HYP_DTYPE)[0]
    assert not sa.validate([none])
    past = cq.copy()
    past["mask"][9] |= 0x04                              # bit 77
    assert not sa.validate([past])


def test_frozen_constructed_fixture(oracle):
    """tests/golden/ap_constructed.npz is what the restatement gives today, and its cases are ap_craft's"""
    d = np.load(os.path.join(ROOT, "tests", "golden", "ap_constructed.npz"))
    cases = ac.build_cases(oracle)
    assert [str(n) for n in d["names"]] == [c["name"] for c in cases] and np.array_equal(d["vectors"], oc.vectors_of(cases))
    B = len(d["counts"])
    frames = dict(cands=d["cands"].view(oc.CAND_DTYPE).reshape(B, -1), counts=d["counts"], status_in=d["status_in"], vec=d["vec"])
    mag = oc.waterfalls(d["vectors"], frames)
    assert [str(n) for n in d["configs"]] == [name for name, _, _ in ac.configs(cases)]
    for name, gate in zip(d["configs"], d["gates"]):
        hyps = d[f"hyps_{name}"].view(sa.HYP_DTYPE)
        st, info = sa.ap_candidates(oracle, mag, frames["cands"], frames["counts"], frames["status_in"], hyps, int(gate),
                                    status_out=frames["status_in"], iters=ac.ITERS)
        assert info.view(np.uint8).tobytes() == d[f"info_{name}"].tobytes(), name
        assert st.tobytes() == ac.fixture_status(d, str(name)).tobytes(), name
