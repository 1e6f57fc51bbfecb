"""CPU tests of the constructed soft bits (tests/osd_craft.py): the waterfall cells give the oracle's ft8_extract_likelihood
exactly the integers asked for, every case a..h has the property it is named for in the restatement
(tests/ft8_spec_osd.py), the restatement agrees with the brute-force search of tests/test_osd_cpu.py where only these cases
reach, and the frozen fixture (tests/golden/osd_constructed.npz) still is what the generator beside it writes."""
import os

import numpy as np
import pytest

import ft8_spec_osd as so
import osd_craft as oc
from test_osd_cpu import _independent_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built(oracle):
    cases = oc.build_cases(oracle)
    frames = oc.build_frames(cases)
    mag = oc.waterfalls(oc.vectors_of(cases), frames)
    llr = [oracle.llr(mag[f], frames["cands"][f, i]) for f, i in oc.slots(frames)]
    return cases, frames, mag, llr


def _of(built, *letters):
    cases, frames, mag, llr = built
    return [(c, llr[ci]) for ci, c in enumerate(cases) if c["case"] in letters]


def test_raw_soft_bits_are_the_integers_asked_for(oracle, built):
    cases, frames, mag, _ = built
    where = oc.slots(frames)
    assert len(where) == len(cases) >= 300
    subs, heads, tails = set(), 0, 0
    for ci, (f, i) in enumerate(where):
        cand = frames["cands"][f, i]
        want = oc.effective(cases[ci]["v"], cand["time_offset"])
        raw = oracle.llr(mag[f], cand, normalise=False)
        assert np.array_equal(raw, want.astype(np.float32)), cases[ci]["name"]
        subs.add((int(cand["time_sub"]), int(cand["freq_sub"])))
        if cand["time_offset"] < -7:                                  # the first symbols lie before block 0: they read 0
            assert not raw[:3].any() and cases[ci]["v"][:3 * (-7 - cand["time_offset"])].any()
            heads += 1
        if cand["time_offset"] > 20:                                  # the last symbols lie past block 91
            assert not raw[-3:].any() and cases[ci]["v"][-3 * (cand["time_offset"] - 20):].any()
            tails += 1
    assert len(subs) == 4 and heads >= 10 and tails >= 10
    # the frames: ragged counts, a frame without candidates, records that are only copied between the attempted ones
    import rtlsdr_ft8d_amd as ft8
    st = frames["status_in"].view(ft8.STATUS_DTYPE).reshape(len(mag), -1)
    counts = frames["counts"]
    assert (counts == 0).any() and len(set(counts.tolist())) > 4 and counts.max() < oc.CAP
    live = np.arange(oc.CAP)[None, :] < counts[:, None]
    attempt = (st["ok"] == 0) & (st["ldpc_errors"] != 0)
    assert np.array_equal(attempt & live, frames["vec"] >= 0)
    assert set(st["ldpc_errors"][attempt & live].tolist()) == {1, 83} and len(set(st["iters"][attempt & live].tolist())) > 20
    assert (live & ~attempt & (st["ok"] != 0)).sum() >= 10 and (live & ~attempt & (st["ok"] == 0)).sum() >= 10
    assert (frames["status_in"][~live] == oc.FILL).all()


def test_case_a_last_pivot_in_the_third_slot(built):
    seen = set()
    for c, llr in _of(built, "a"):
        order = so.sort_order(llr)
        piv_row, piv_col, _ = so.eliminate(order)
        assert piv_col[-1] == c["last_pivot"] >= 128 and piv_row[-1] == c["pivot_row"]
        assert int(llr[order[piv_col[-1]]] > 0) == c["pivot_h"]
        seen.add((piv_row[-1] >= 64, c["pivot_h"]))
    assert len(seen) == 4 and max(c["last_pivot"] for c, _ in _of(built, "a")) == 152


def test_case_b_saturated_weights(built):
    got = {}
    for c, llr in _of(built, "b"):
        w = so.hard_and_weights(llr)[1]
        got[c["name"]] = (int((w == 255).sum()), int((w == 0).sum()), float(np.abs(llr).max()))
        assert got[c["name"]][0] == c["saturated"]
    assert [got[f"b_{k}_of_255"][0] for k in (1, 2, 3, 4, 5)] == [1, 2, 3, 4, 0]
    assert 28.0 < got["b_5_of_255"][2] < 32.0 <= got["b_4_of_255"][2]          # the near side: five large values do not saturate
    assert all(v[1] >= 50 for v in got.values())                                # weights of 0, from soft bits of exactly 0 among others


def test_cases_c_d_e_results(oracle, built):
    for c, llr in _of(built, "c"):
        assert not np.isfinite(llr).all(), c["name"]
    inf = [c["name"] for c, llr in _of(built, "c") if np.isinf(llr).all()]
    nan = [c["name"] for c, llr in _of(built, "c") if np.isnan(llr).all()]
    assert "c_all_minus_7" in inf and nan == ["c_all_zero"]
    for c, llr in _of(built, "d", "e"):
        for order in range(3):
            metric, pat, nhard, cw = so.search(llr)[order]
            assert (pat, nhard) == (0, 0) and so.judge(oracle, cw, nhard, 83)[0] == c["result"], (c["name"], order)
            if c["case"] == "d":
                assert metric == 0 and not cw.any()
            else:
                assert np.array_equal(cw, c["codeword"]) and np.array_equal(cw[:77], c["payload"])


def test_case_f_gate_boundary(oracle, built):
    """every planted message comes back at pattern 0 with nhard == e, e = 83 included"""
    assert [c["errors"] for c, _ in _of(built, "f")] == [1, 20, 27, 83]
    for c, llr in _of(built, "f"):
        e = c["errors"]
        for order in range(3):
            metric, pat, nhard, cw = so.search(llr)[order]
            assert (pat, nhard) == (0, e) and np.array_equal(cw, c["codeword"]), (c["name"], order)
            code, _, _, _, text = so.judge(oracle, cw, nhard, e)
            assert code == 1 and text.decode() == c["text"]
            assert so.judge(oracle, cw, nhard, e - 1)[0] == 2


def test_case_g_pattern_indices(built):
    got = []
    for c, llr in _of(built, "g"):
        res = so.search(llr)
        for order in range(3):
            metric, pat, nhard, cw = res[order]
            if order >= c["order"]:
                assert pat == c["pattern"] and nhard == c["nhard"] and np.array_equal(cw, c["codeword"]), (c["name"], order)
            else:
                assert not np.array_equal(cw, c["codeword"]), (c["name"], order)
        got.append(res[2][1])
    assert tuple(got) == oc.G_PATTERNS


def test_restatement_against_brute_force_on_cases_a_b_g_h(built):
    ties = 0
    sel = _of(built, "a", "b", "g", "h")
    assert len(sel) == 4 + 5 + 14 + 40
    for c, llr in sel:
        res = so.search(llr)
        basis, C, metrics = _independent_search(llr)
        h = (llr > 0).astype(np.uint8)
        for order in range(3):
            metric, pat, nhard, cw = res[order]
            k = int(np.argmin(metrics[:so.NPAT[order]]))               # first minimum: ties to the smallest index
            assert (metric, pat) == (int(metrics[k]), k), (c["name"], order)
            assert np.array_equal(cw, C[k]) and nhard == int((cw ^ h).sum())
        if c["case"] == "h":
            ties += int((metrics == metrics.min()).sum() > 1)
    print(f"case h: {ties} of 40 vectors have more than one pattern at the minimum metric")
    assert 4 * ties >= 40


def test_every_result_code_and_tally(oracle, built):
    cases, frames, mag, _ = built
    searches, infos = {}, {}
    for order, gate in oc.CONFIGS:
        infos[(order, gate)] = so.osd_candidates(oracle, mag, frames["cands"], frames["counts"], frames["status_in"], order, gate,
                                                 searches=searches)[1]
    t = oc.tallies(oracle, cases, frames, mag, infos)
    print(t)
    assert t["results_seen"] == [0, 1, 2, 3, 4, 5, 6] and tuple(t["case_g_patterns"]) == oc.G_PATTERNS
    assert t["max_last_pivot"] >= 152 and all(t["saturated_weight_counts"].get(str(k), 0) >= 1 for k in (1, 2, 3, 4))


def test_frozen_fixture(oracle):
    import rtlsdr_ft8d_amd as ft8
    d = np.load(os.path.join(ROOT, "tests", "golden", "osd_constructed.npz"))
    frames = dict(cands=d["cands"].view(oc.CAND_DTYPE).reshape(len(d["counts"]), -1), counts=d["counts"], status_in=d["status_in"],
                  vec=d["vec"])
    names = [str(n) for n in d["names"]]
    cases = [c for c in oc.build_cases(oracle) if c["case"] != "i"]
    assert names[:len(cases)] == [c["name"] for c in cases] and np.array_equal(d["vectors"][:len(cases)], oc.vectors_of(cases))
    mag = oc.waterfalls(d["vectors"], frames)
    searches, accepted = {}, 0
    for order, gate in d["configs"]:
        st, info = so.osd_candidates(oracle, mag, frames["cands"], frames["counts"], frames["status_in"], int(order), int(gate),
                                     status_out=frames["status_in"], searches=searches)
        assert st.tobytes() == oc.fixture_status(d, order, gate).tobytes(), (order, gate)
        assert info.tobytes() == d[f"info_o{order}_g{gate}"].tobytes(), (order, gate)
        accepted += int((info["result"] == 1).sum())
    assert accepted >= 12
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "osd_constructed.npz")) <= os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "osd_frame.npz"))
