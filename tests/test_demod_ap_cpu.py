"""CPU tests of a-priori decoding on the soft bits demodulated from the I/Q samples (include/ft8gpu.h "a-priori decoding on the
soft bits demodulated from the I/Q samples"): the record and parameter layouts against gcc, the restatement
tests/ft8_spec_apsoft.py against the pieces it is made of (ft8_spec_demod.analyse / demod_one for the rows, ft8_spec_ap.attempts /
resolve for the rule on a row, ft8_spec_demod.decode_demod without hypotheses), the constructed rows of tests/apsoft_craft.py,
each named case asserted by name, and a seeded sensitivity row.  No GPU is used here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ap_craft as ac
import apsoft_craft as xc
import demod_edges_craft as de
import ft8_spec_ap as sa
import ft8_spec_apsoft as sx
import ft8_spec_demod as sdm
import ft8_spec_messages as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as ft8
    return ft8


def test_layouts_against_gcc(ft8, tmp_path):
    fields = ("result", "nhard", "hyp", "iters", "set", "pad", "results")
    pfields = ("demod", "nhyp", "ap_max_hard_errors", "hyps")
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ft8gpu.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(ft8gpu_apsoft_info));', 'printf("psize %zu\\n", sizeof(ft8gpu_demod_ap_params));']
    lines += [f'printf("{f} %zu\\n", offsetof(ft8gpu_apsoft_info, {f}));' for f in fields]
    lines += [f'printf("p_{f} %zu\\n", offsetof(ft8gpu_demod_ap_params, {f}));' for f in pfields]
    lines += ['printf("consts %d %d %d\\n", FT8GPU_SOFT_STRIDE, FT8GPU_APSOFT_MAX_HARD_ERRORS, FT8GPU_AP_MAX_HYPOTHESES);', 'return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=gnu17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    want = {"size": "20", "psize": "100", "result": "0", "nhard": "1", "hyp": "2", "iters": "3", "set": "4", "pad": "5", "results": "8",
            "p_demod": "0", "p_nhyp": "12", "p_ap_max_hard_errors": "16", "p_hyps": "20",
            "consts": f"{sx.STRIDE} {sx.MAX_HARD_ERRORS} {sa.MAX_HYPOTHESES}"}
    assert got == want
    for dt in (ft8.APSOFT_INFO_DTYPE, sx.INFO_DTYPE):
        assert dt.itemsize == 20 and [dt.fields[f][1] for f in fields] == [int(want[f]) for f in fields]
        assert dt.fields["results"][0].shape == (3, 4)
    assert ft8.APSOFT_INFO_DTYPE == sx.INFO_DTYPE and (ft8.SOFT_STRIDE, ft8.APSOFT_MAX_HARD_ERRORS) == (sx.STRIDE, sx.MAX_HARD_ERRORS)
    assert C.sizeof(ft8.DemodApParams) == 100 and [getattr(ft8.DemodApParams, f).offset for f in pfields] == [0, 12, 16, 20]
    assert sx.STRIDE * 3 * 4 == 2112 and 2112 % 16 == 0


# ---- the rows ---------------------------------------------------------------------------------------------------------------------

ROW_NAMES = ("good_behind_a_refusal", "set2_accepts", "set3_accepts", "scaled_inf_psync", "crc_refuses")


@pytest.fixture(scope="module")
def edge_rows(ft8, oracle):
    """five named candidates of tests/demod_edges_craft.py, one per frame, behind a record that does not qualify"""
    iq, cands, _counts, status, where = de.constructed(ft8, oracle)
    at = [where[n] for n in ROW_NAMES]
    B = len(at)
    c2 = np.zeros((B, 3), ft8.CAND_DTYPE)
    s2 = np.zeros((B, 3), ft8.STATUS_DTYPE)
    for k, (f, i) in enumerate(at):
        c2[k, 0], s2[k, 0] = cands[f, i], status[f, i]
        c2[k, 1], s2[k, 1] = cands[f, i], status[f, i]
        s2[k, 0]["ok"], s2[k, 0]["ldpc_errors"] = 1, 0                 # not attempted
        c2[k, 2], s2[k, 2] = cands[f, i], status[f, i]                 # behind the count
    iq2 = np.stack([iq[f] for f, _i in at])
    return iq2, c2, np.full(B, 2, np.int32), s2, {}


@pytest.mark.parametrize("sets", range(1, 8))
def test_soft_rows_are_the_sets_x_where_the_rule_says_so(oracle, edge_rows, sets):
    iq, cands, counts, status, cache = edge_rows
    w4 = sdm.twiddles()
    fill = np.full((len(iq), 3, 3, sx.STRIDE), 7.5, np.float32)
    out, inf, soft = sx.demod_soft(oracle, iq, cands, counts, status, sets, 174, soft=fill, bp=oracle.bp_decode, w4=w4, cache=cache)
    want_out, want_inf = sdm.demod_candidates(oracle, iq, cands, counts, status, sets, 174, bp=oracle.bp_decode, w4=w4, cache=cache)
    assert out.tobytes() == want_out.tobytes() and inf.tobytes() == want_inf.tobytes()
    accepted = {}
    for k, name in enumerate(ROW_NAMES):
        assert (soft[k, 0] == 0).all() and not np.signbit(soft[k, 0]).any()        # not attempted: 176 times +0
        assert (soft[k, 2] == 7.5).all()                                           # behind the count: the caller's bytes
        analysis = cache[(k, cands[k, 1].tobytes())]
        info, win = sdm.demod_one(oracle, iq[k, 0], iq[k, 1], cands[k, 1], w4, sets, 174, bp=oracle.bp_decode, analysis=analysis)
        assert info.tobytes() == inf[k, 1].tobytes()
        for n in (1, 2, 3):
            x = analysis[3][n][1]
            named = (sets >> (n - 1)) & 1
            reached = named and not (win is not None and n > info["set"])
            row = soft[k, 1, n - 1]
            if reached and x is not None:
                assert row[:174].tobytes() == x.tobytes() and row[174:].tobytes() == bytes(8), (name, n)
            else:
                assert row.tobytes() == bytes(4 * sx.STRIDE), (name, n)
        if win is not None:
            accepted[name] = int(info["set"])
        if name == "scaled_inf_psync":                                 # every set is non-finite: three zero rows, result 6
            assert all(analysis[3][n][1] is None for n in (1, 2, 3)) and (soft[k, 1] == 0).all() and info["result"] == 6
    if sets == 7:
        assert accepted == {"good_behind_a_refusal": 1, "set2_accepts": 2, "set3_accepts": 3}
    if sets == 4:
        assert accepted.get("set3_accepts") == 3 and "set2_accepts" not in accepted


# ---- the rule on a row is AP's -----------------------------------------------------------------------------------------------------

def test_one_usable_row_is_ap_s_rule_and_nothing_else(ft8, oracle):
    cases = ac.build_cases(oracle)
    rows = xc.candidates(oracle)
    st = np.zeros((1, 1), ft8.STATUS_DTYPE)
    st["ldpc_errors"], st["iters"] = 9, 20
    seen = set()
    for _name, hyps, gate in ac.configs(cases):
        hy = ac.hyps_array(hyps)
        for name in ("set1", "dx", "no_cq_clean", "crc", "unpack", "all_negative", "scaled_m59", "edge_sub"):
            row = rows[name][0, :174]
            for n in (1, 2, 3):
                soft = np.zeros((1, 1, 3, sx.STRIDE), np.float32)
                soft[0, 0, n - 1] = rows[name][0]
                out, inf = sx.ap_soft_candidates(oracle, soft, np.ones(1, np.int32), st, 7, hy, gate)
                want, win = sa.resolve(oracle, row, sa.attempts(oracle, row, hy, 20), gate)
                got = inf[0, 0]
                assert (got["result"], got["nhard"], got["hyp"], got["iters"], got["set"]) == \
                    (want["result"], want["nhard"], want["hyp"], want["iters"], n)
                assert got["results"][n - 1].tobytes() == want["results"].tobytes()
                others = [m for m in range(3) if m != n - 1 and (m < n - 1 or win is None)]        # zero rows: unusable where reached
                assert all(got["results"][m].tolist() == [6, 0, 0, 0] for m in others)
                assert (out[0, 0].view(ft8.STATUS_DTYPE)[0]["ok"] == 1) == (win is not None)
                if win is not None:
                    assert bytes(out[0, 0].view(ft8.STATUS_DTYPE)[0]["text"]).rstrip(b"\0") == win[4].rstrip(b"\0")
                seen.add(int(want["result"]))
    assert {1, 2, 3, 4, 7, 8} <= seen


# ---- the constructed rows ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def crafted(ft8, oracle):
    soft, counts, status, where = xc.build(ft8, oracle)
    cases = ac.build_cases(oracle)
    cfg = {name: (ac.hyps_array(hyps), gate) for name, hyps, gate in ac.configs(cases)}
    return soft, counts, status, where, cfg, {c["name"]: c for c in cases}


def run(oracle, crafted, config, sets=7):
    soft, counts, status, where, cfg, _by = crafted
    hyps, gate = cfg[config]
    out, inf = sx.ap_soft_candidates(oracle, soft, counts, status, sets, hyps, gate)
    return out, inf, where


def brief(r):
    return int(r["result"]), int(r["set"]), int(r["hyp"])


def test_constructed_rows_are_what_they_are_named_for(ft8, oracle, crafted):
    soft, counts, status, where, _cfg, by = crafted
    assert set(xc.NAMES) <= set(where) and list(counts) == [len(xc.NAMES), 0, 3, xc.CAP, 17]
    out, inf, w = run(oracle, crafted, "cq")
    assert [brief(inf[w[n]]) for n in ("set1", "set2", "set3", "zero_between", "nan_then_good")] == \
        [(1, 1, 0), (1, 2, 0), (1, 3, 0), (1, 3, 0), (1, 2, 0)]
    assert inf[w["set3"]]["results"].tolist() == [[7, 0, 0, 0], [7, 0, 0, 0], [1, 0, 0, 0]]
    assert inf[w["zero_between"]]["results"].tolist() == [[7, 0, 0, 0], [6, 0, 0, 0], [1, 0, 0, 0]]      # an all-zero row between usable ones
    assert inf[w["nan_then_good"]]["results"].tolist() == [[6, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]
    r = inf[w["unusable"]]                                                                             # NaN; +inf; -inf beside +inf
    assert brief(r) == (6, 0, 0) and r["results"].tolist() == [[6, 0, 0, 0]] * 3 and (r["nhard"], r["iters"]) == (0, 0)
    assert out[w["unusable"]].tobytes() == status[w["unusable"]].tobytes()
    for n in ("copied_ok", "copied_no_errors"):
        assert inf[w[n]].tobytes() == bytes(20) and out[w[n]].tobytes() == status[w[n]].tobytes()
    assert brief(inf[w["crc"]]) == (3, 1, 0) and brief(inf[w["no_cq"]]) == (7, 2, 0) and brief(inf[w["all_negative"]]) == (7, 1, 0)
    for n in ("edge_m57", "edge_m59", "edge_sub"):                     # one element either side of the guard's 2^-58: the decode is the same
        assert brief(inf[w[n]]) == (1, 1, 0) and out[w[n]].tobytes()[4:] == out[w["set1"]].tobytes()[4:]
    for n, e in (("edge_m57", -57), ("edge_m59", -59), ("edge_sub", -140), ("scaled_m57", -57), ("scaled_m59", -59), ("scaled_sub", -140)):
        a = np.abs(soft[w[n]][0, :174])
        assert a[a > 0].min() == np.float32(2.0 ** e)
    assert np.abs(soft[w["scaled_sub"]][0]).max() < 2.0 ** -126 and np.isfinite(soft[w["scaled_p100"]]).all()
    assert np.abs(soft[w["scaled_p100"]][0]).max() > 2.0 ** 100
    for n in ("scaled_m57", "scaled_m59", "scaled_sub", "scaled_p100"):
        assert inf[w[n]]["set"] == 1 and inf[w[n]]["results"][0][0] != 6                               # usable, whatever BP makes of them
    text = bytes(out[w["set1"]].view(ft8.STATUS_DTYPE)[0]["text"]).rstrip(b"\0").decode()
    assert text == by["a_0"]["text"] and out[w["set1"]].view(ft8.STATUS_DTYPE)[0]["iters"] == 20
    # the gate at the accepted word's hard errors and one below
    e = by["a_0"]["nhard"]
    assert inf[w["set2"]]["nhard"] == e
    _o, at_gate, _w = run(oracle, crafted, f"cq_gate_{e}")
    _o, below, _w = run(oracle, crafted, f"cq_gate_{e - 1}")
    assert brief(at_gate[w["set2"]]) == (1, 2, 0) and brief(below[w["set2"]]) == (2, 2, 0)
    assert below[w["set2"]]["results"].tolist() == [[7, 0, 0, 0], [2, 0, 0, 0], [6, 0, 0, 0]] and below[w["set2"]]["nhard"] == e
    # acceptance under hypothesis 3 of 4; codes 4 and 8; the all-zero word
    _o, four, _w = run(oracle, crafted, "four")
    assert brief(four[w["dx"]]) == (1, 1, 2) and four[w["dx"]]["results"][0].tolist() == [7, 7, 1, 0]
    _o, d77, _w = run(oracle, crafted, "d_all_77")
    assert brief(d77[w["unpack"]]) == (4, 1, 0)
    _o, wrong, _w = run(oracle, crafted, "b_one_wrong")
    assert brief(wrong[w["no_cq_clean"]]) == (8, 1, 0)
    _o, zero, _w = run(oracle, crafted, "zero_all_77")
    assert brief(zero[w["all_negative"]]) == (7, 1, 0) and zero[w["all_negative"]]["iters"] == 0       # BP leaves at the all-zero word


def test_sets_name_which_rows_are_walked(oracle, crafted):
    _soft, _counts, _status, w, _cfg, _by = crafted
    for sets in range(1, 8):
        _out, inf, _w = run(oracle, crafted, "cq", sets)
        named = [n for n in (1, 2, 3) if (sets >> (n - 1)) & 1]
        r = inf[w["set3"]]
        assert brief(r) == ((1, 3, 0) if 3 in named else (7, named[-1], 0))
        assert [r["results"][n - 1][0] != 0 for n in (1, 2, 3)] == [n in named for n in (1, 2, 3)]
        assert brief(inf[w["unusable"]]) == (6, 0, 0)                  # sets that name only unusable rows
        z = inf[w["zero_between"]]
        if sets == 2:
            assert brief(z) == (6, 0, 0) and z["results"].tolist() == [[0, 0, 0, 0], [6, 0, 0, 0], [0, 0, 0, 0]]


# ---- the whole path ----------------------------------------------------------------------------------------------------------------

SEEDS = range(3300, 3332)                     # the snr-21 row of tools/demod_gain.py: one CQ station per frame at -21 dB


@pytest.fixture(scope="module")
def seeded(oracle):
    import synth_util as S
    enc = S.oracle_encode_fn(oracle)
    fr = [S.make_frame(s, 1, enc, snr_range=(-21.0, -21.0)) for s in SEEDS]
    iq = np.ascontiguousarray(np.stack([f[0] for f in fr]), np.float32)
    planted = [f[1] for f in fr]
    stages = sm.oracle_stages(oracle, iq, 120, 10, 4, 20)
    return iq, planted, stages, {}


def test_without_hypotheses_the_whole_path_is_decode_demod(oracle, seeded):
    iq, _planted, stages, cache = seeded
    part = tuple(a[:6] for a in stages)
    a = sx.decode_demod_ap(oracle, iq[:6], hyps=(), stages=part, bp=oracle.bp_decode, cache=cache)
    b = sdm.decode_demod(oracle, iq[:6], stages=part, bp=oracle.bp_decode, cache=cache)
    assert a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all() and (a[2][:, :2] == b[2]).all() and (a[2][:, 2] == a[2][:, 1]).all()


def test_seeded_row_gains_planted_messages_and_nothing_else(oracle, seeded):
    """32 frames of one CQ station at -21 dB: AP on the demodulated soft bits gains at least one message over the demodulation, every
    record is a planted message, gained records carry pad[1] = 1 and the set in pad[3]"""
    iq, planted, stages, cache = seeded
    trace = []
    m, n, nbs = sx.decode_demod_ap(oracle, iq, hyps=[sa.from_text("CQ ? ?")], ap_gate=sx.MAX_HARD_ERRORS, stages=stages, bp=oracle.bp_decode,
                                   cache=cache, trace=trace)
    m0, n0, nbs0 = sdm.decode_demod(oracle, iq, stages=stages, bp=oracle.bp_decode, cache=cache)
    print("frames decoded after BP, the demodulation, AP:", [int((nbs[:, k] > 0).sum()) for k in range(3)])
    assert (nbs[:, :2] == nbs0).all() and (nbs[:, 2] == n).all() and (n >= n0).all()
    assert int((n - n0).sum()) >= 1
    for f in range(len(n)):
        assert m[f, :n0[f]].tobytes() == m0[f, :n0[f]].tobytes()
        for r in range(int(n[f])):
            assert m[f, r]["text"].decode() in planted[f], (f, r, m[f, r]["text"])
        for r in range(int(n0[f]), int(n[f])):
            rec = trace[0][1][f, int(m[f, r]["cand_index"])]
            assert m[f, r]["pad"][1] == 1 and 1 <= m[f, r]["pad"][3] <= 3 and rec["result"] == 1 and rec["set"] == m[f, r]["pad"][3]
