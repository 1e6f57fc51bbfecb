"""CPU tests of the call hints (include/ft8gpu.h "call hints"): the restatement tests/ft8_spec_hint.py on the constructed cases
of tests/hint_craft.py -- each configuration has the property it is named for, and the frozen fixture
tests/golden/hint_constructed.npz (which the device is held to as well) is reproduced; the update rule on fabricated records;
the host helpers of csrc/ft8_hint.c against the restatement and under ASan + UBSan; the struct layouts; the identity with the
a-priori restatement fed with ft8gpu_hint_hypothesis of the tried entries; the 3 x 4 stream scenario.  No GPU is used here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ft8_spec_ap as sa
import ft8_spec_hint as sh
import ft8_spec_match as smt
import ft8_spec_messages as sm
import hint_craft as hc
import osd_craft as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIO = dict(tries=2, max_bad_per_64=16, max_hard_errors=40)     # AP's measured gate; tries and the preselection gate are not measured yet


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc"), "-j8"])
    m.load_library()
    return m


@pytest.fixture(scope="module")
def built(oracle, ft8):
    cases, frames, mag, cfgs = hc.build(oracle)
    return cases, frames, mag, cfgs, hc.expected(oracle, frames, mag, cfgs)


# ---- the constructed cases -----------------------------------------------------------------------------------------------------

def test_frozen_constructed_fixture(built):
    cases, frames, mag, cfgs, want = built
    d = hc.load_golden()
    assert d["names"] == [c[0] for c in cfgs] and [str(n) for n in d["case_names"]] == [c["name"] for c in cases]
    assert np.array_equal(d["vectors"], oc.vectors_of(cases)) and np.array_equal(d["params"], np.array([c[2:] for c in cfgs]))
    for key in ("counts", "status_in", "vec"):
        assert np.array_equal(d[key], frames[key]), key
    assert d["cands"].tobytes() == frames["cands"].tobytes()
    for k, c in enumerate(cfgs):
        assert d["states"][k].tobytes() == np.asarray(c[1]).tobytes(), c[0]
        status, info = want[c[0]]
        assert d[f"info_{k}"].tobytes() == info.tobytes(), c[0]
        assert hc.golden_status(d, k).tobytes() == status.tobytes(), c[0]


def test_configurations_are_what_they_are_named_for(built):
    cases, frames, mag, cfgs, want = built
    where = dict(zip([c["name"] for c in cases], oc.slots(frames)))
    planted = ("p_0", "p_1", "p_2")

    def info(config, name):
        return want[config][1][where[name]]

    def accepted(config):
        i = want[config][1]
        return int(sum((i[f, :frames["counts"][f]]["result"] == 1).sum() for f in range(len(frames["counts"]))))

    for name in ("empty", "expired", "wrong_phase_used", "kind_0_and_4", "nbad_above_the_gate", "gate_0_refuses_nbad_1"):
        i = want[name][1]
        assert not any((i[f, :frames["counts"][f]]["ntried"] != 0).any() for f in range(len(frames["counts"]))), name
        assert want[name][0].tobytes() == frames["status_in"].tobytes()
        assert {int(info(name, c["name"])["result"]) for c in cases} == {0, 6}, name       # 6: the unusable soft bits, tables or not
    for name in ("planted", "not_expired", "wrapped_age", "wrong_phase_ignored", "phase_garbage", "garbage_above_bit_28"):
        for p, at in zip(planted, (5, 70, 300)):
            r = info(name, p)
            assert r["result"] == 1 and r["ntried"] == 1 and r["index"][0] == at and r["results"][0] == 1, (name, p, r)
        assert want[name][1].tobytes() == want["planted"][1].tobytes()
    for at in ((0, 63, 64), (511, 0, 63), (64, 511, 0), (63, 64, 511)):
        name = "at_%d_%d_%d" % at
        for p, j in zip(planted, at):
            r = info(name, p)
            assert r["result"] == 1 and r["index"][r["ntried"] - 1] == j, (name, p, r)
    # the gates: one entry, made from p_0's own hard decisions with k bits inverted
    for name, tried in (("nbad_at_the_gate", 1), ("nbad_above_the_gate", 0), ("gate_0_passes_nbad_0", 1), ("gate_0_refuses_nbad_1", 0)):
        r = info(name, "p_0")
        assert r["ntried"] == tried and (not tried or r["index"][0] == 9), (name, r)
    for tries in (1, 4):
        i = want[f"gate_64_tries_{tries}"][1]
        usable = [info(f"gate_64_tries_{tries}", c["name"]) for c in cases]
        assert all(r["result"] == 6 or r["ntried"] >= 1 for r in usable)                  # every live entry passes
        assert max(int(r["ntried"]) for r in usable) == tries
    # ties: nbad 0 in every entry made from p_0's hard decisions -- the 61-bit entry first, then the smaller index; nbad 1 last
    r = info("ties_between_and_within_sizes", "p_0")
    assert r["ntried"] == 4 and list(r["index"]) == [400, 3, 4, 2] and r["result"] != 1, r
    # five passing entries
    for rank in (1, 4, 5):
        for tries in (1, 2, 3, 4):
            r = info(f"planted_ranked_{rank}_tries_{tries}", "p_0")
            order = list(r["index"][:r["ntried"]])
            if rank <= tries:
                assert r["result"] == 1 and r["ntried"] == rank and order[-1] == 200 and all(c in (7, 8) for c in r["results"][:rank - 1]), (rank, tries, r)
            else:
                assert r["result"] in (7, 8) and r["ntried"] == tries and 200 not in order, (rank, tries, r)
    r = info("planted_ranked_4_tries_4", "p_0")
    print("a first try that fails in front of the accepted one:", list(r["results"]), list(r["index"]))
    # the hard-error gate between the two sizes of p_2's hypotheses
    r = info("first_try_refused_by_the_gate", "p_2")
    assert list(r["results"][:2]) == [2, 1] and list(r["index"][:2]) == [8, 7] and r["result"] == 1 and r["ntried"] == 2, r
    r = info("both_tries_refused_by_the_gate", "p_2")
    assert list(r["results"][:2]) == [2, 2] and r["result"] == 2, r
    # the CQ field as a hint: a-priori decoding's own cases
    assert info("cq_as_a_hint", "c_wrong_crc")["result"] == 3 and info("cq_as_a_hint", "a_0")["result"] == 1
    # q_3, q_4, q_8: the named code first, then "A B ?" accepted; alone, the code is the result
    for name, code, at in (("q_3", 3, 10), ("q_4", 4, 11), ("q_8", 8, 12)):
        r = info("first_try_3_4_8_then_accepted", name)
        assert list(r["results"][:2]) == [code, 1] and list(r["index"][:2]) == [at, 13] and r["result"] == 1 and r["ntried"] == 2, (name, r)
        r = info("first_try_3_4_8_alone", name)
        assert r["result"] == code and r["ntried"] == 1 and r["index"][0] == at, (name, r)
    # every code the rule lists in front of an accepted try: a record with results[k] == code at some k < ntried - 1, result 1
    before_accept = set()
    for c in cfgs:
        i = want[c[0]][1]
        for f in range(len(frames["counts"])):
            for r in i[f, :frames["counts"][f]]:
                if r["result"] == 1:
                    before_accept |= {int(x) for x in r["results"][:int(r["ntried"]) - 1]}
    assert before_accept == {2, 3, 4, 7, 8}, before_accept
    seen = {int(x) for c in cfgs for f in range(len(frames["counts"])) for x in want[c[0]][1][f, :frames["counts"][f]]["results"].ravel()}
    assert seen == {0, 1, 2, 3, 4, 7, 8}, seen                         # 5 cannot occur (the header says why), 6 tries nothing
    assert accepted("planted") >= 3


def test_statuses_equal_ap_with_the_tried_hypotheses(oracle, ft8, built):
    """for every candidate of every configuration: ft8_spec_ap fed with ft8gpu_hint_hypothesis of the entries the info record
    names, in that order, leaves the same status record"""
    cases, frames, mag, cfgs, want = built
    B = len(frames["counts"])
    for name, st, tries, gate, hard, max_age, use_phase in cfgs:
        status, info = want[name]
        for f in range(B):
            for i in range(int(frames["counts"][f])):
                n = int(info[f, i]["ntried"])
                if n == 0:
                    assert status[f, i].tobytes() == frames["status_in"][f, i].tobytes()
                    continue
                hyps = [ft8.hint_hypothesis(st["entry"][0][int(j)]) for j in info[f, i]["index"][:n]]
                assert all(h is not None and h.tobytes() == sh.hypothesis(st["entry"][0][int(j)]).tobytes()
                           for h, j in zip(hyps, info[f, i]["index"][:n]))
                one = np.ones(1, np.int32)
                ap_st, ap_info = sa.ap_candidates(oracle, mag[f:f + 1], frames["cands"][f:f + 1, i:i + 1], one, frames["status_in"][f:f + 1, i:i + 1],
                                                  hyps, hard, iters=hc.ITERS)
                assert ap_st[0, 0].tobytes() == status[f, i].tobytes(), (name, f, i)
                assert list(ap_info[0, 0]["results"][:n]) == list(info[f, i]["results"][:n]) and ap_info[0, 0]["nhard"] == info[f, i]["nhard"]


# ---- the update rule -------------------------------------------------------------------------------------------------------------

def test_update_rule_on_fabricated_records(ft8):
    layout = hc.update_layout()
    msgs, n = hc.records_of(layout)
    state = sh.update(msgs, n)
    r0 = state[0]["entry"]
    used = r0[r0["used"] != 0]
    k1abc, w9xyz, k1jt = (hc.call_field(c) for c in ("K1ABC", "W9XYZ", "K1JT"))
    # slot 0: "CQ K1ABC FN42" -- F1 is a token: only the two F2 inserts; "K1ABC W9XYZ EM48" -- all four
    assert [tuple(int(x) for x in (e["kind"], e["a"], e["b"], e["phase"])) for e in used[:6]] == \
        [(2, 0, k1abc, 0), (1, k1abc, 0, 1), (2, 0, w9xyz, 0), (1, w9xyz, 0, 1), (3, k1abc, w9xyz, 0), (3, w9xyz, k1abc, 1)]
    keys = {tuple(int(x) for x in (e["kind"], e["a"], e["b"], e["phase"])) for e in used}
    assert len(keys) == len(used)                                      # no entry twice
    # "CQ DX K1JT FN20" at slot 1: the sender only; /R flags are part of the field; hashed calls, type 2 / 4 / free text: nothing
    assert (2, 0, k1jt, 1) in keys and (1, k1jt, 0, 0) in keys and not any(k[0] == 3 and k1jt in k[1:3] for k in keys)
    assert (3, k1abc | 1, w9xyz, 1) in keys and (3, k1abc, w9xyz | 1, 1) in keys
    for text in ("<K1ABC> W9XYZ -05", "W9XYZ <PJ4/K1ABC> RRR"):
        i3, f1, f2 = sh.fields(ft8.pack77(text))
        assert i3 == 1 and ((f1 >> 1) < sh.CLEAR) != ((f2 >> 1) < sh.CLEAR)
    assert len(sh.inserts_of(ft8.pack77("<K1ABC> W9XYZ -05"), 0)) == 2 and sh.inserts_of(ft8.pack77("W9XYZ <PJ4/K1ABC> RRR"), 0) == []
    for text in ("K1ABC/P W9XYZ/P EM48", "TNX BOB 73 GL", "<W9XYZ> PJ4/K1ABC RR73", "CQ PJ4/K1ABC"):
        assert sh.inserts_of(ft8.pack77(text), 1) == [], text
    assert state[0]["slot"] == 12 and state[1]["slot"] == 12
    # counts outside [0, 50]: 70 is 50 (records 8.. are zero: type 0), -3 is none
    one = sh.update(msgs[:1, 4:6], n[:1, 4:6])
    assert one[0]["cursor"] == sh.update(msgs[:1, 4:5], np.array([[8]]))[0]["cursor"] and one[0]["slot"] == 2
    # the ring wraps: 45 records x 4 inserts x 12 slots
    assert 1 <= state[1]["cursor"] <= 512 and (state[1]["entry"]["used"] == 1).all() and len(set(state[1]["entry"]["stamp"])) > 1
    # a refresh touches the stamp only, also of an expired entry; the result does not depend on the cut
    r2 = state[2]["entry"]
    first = r2[0]
    assert (first["kind"], first["stamp"]) == (2, 10) and state[2]["cursor"] == (r2["used"] != 0).sum() < 4 * 8    # eight records, some of them refreshes
    cut = sh.update(msgs[:, 6:], n[:, 6:], sh.update(msgs[:, :6], n[:, :6]))
    assert cut.tobytes() == state.tobytes()
    # slot at 0xFFFFFFFF wraps; duplicates in a caller-built state: the smallest index is refreshed
    st = sh.new_state(1)
    st["slot"], st["cursor"] = 0xFFFFFFFF, 100 + 512
    hc.put(st, 9, 2, 0, w9xyz, 1, stamp=5)
    hc.put(st, 4, 2, 0xE0000000, w9xyz | 0x20000000, 0xFF, used=7, stamp=6)
    st = sh.update(msgs[2:3, :2], n[2:3, :2], st)                      # "K1ABC W9XYZ RR73" at parity 1, "W9XYZ K1ABC -11" at parity 0
    assert st[0]["slot"] == 1 and st[0]["entry"][4]["stamp"] == 0xFFFFFFFF and st[0]["entry"][9]["stamp"] == 5
    # three new entries from the first record, two from the second: its "A B ?" pair is the first record's, refreshed
    assert st[0]["cursor"] == 100 + 5 and st[0]["entry"][100]["stamp"] == 0xFFFFFFFF and st[0]["entry"][104]["stamp"] == 0
    assert st[0]["entry"][101]["kind"] == 3 and st[0]["entry"][101]["stamp"] == 0 and st[0]["entry"][102]["stamp"] == 0
    assert st[0]["entry"][4]["used"] == 7 and st[0]["entry"][4]["a"] == 0xE0000000


def test_host_helpers_equal_the_restatement(ft8):
    assert ft8.HINT_STATE_DTYPE == sh.STATE_DTYPE and ft8.HINT_INFO_DTYPE == sh.INFO_DTYPE and ft8.HINT_ENTRIES == sh.ENTRIES
    rng = np.random.default_rng(0x417)
    got, want = ft8.hint_state(1), sh.new_state(1)
    got.view(np.uint8)[:] = 0xA5
    ft8.hint_reset(got)
    assert got.tobytes() == want.tobytes()
    pool = [(int(rng.integers(1, 4)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 256))) for _ in range(300)]
    for step in range(1500):
        k, a, b, p = pool[int(rng.integers(0, len(pool)))]
        if step % 97 == 0:
            got["slot"] = want["slot"] = int(rng.integers(0, 1 << 32))
        ft8.hint_insert(got, k, a, b, p)
        sh.insert(want.reshape(()), k, a, b, p)
    assert got.tobytes() == want.tobytes() and (want["entry"]["used"] == 1).sum() > 250
    with pytest.raises(ValueError):
        ft8.hint_insert(got, 0, 1, 1, 0)
    for pattern, kind in (("K1ABC ? ?", 1), ("? W9XYZ ?", 2), ("K1ABC W9XYZ ?", 3), ("CQ DX ? ?", 1), ("K1ABC/R W9XYZ ?", 3)):
        st = ft8.hint_state(1)
        ft8.hint_insert_text(st, pattern, 1)
        e = st["entry"][0][0]
        assert e["kind"] == kind and e["used"] == 1 and e["phase"] == 1
        assert ft8.hint_hypothesis(e).tobytes() == sa.from_text(pattern).tobytes() == sh.hypothesis(e).tobytes(), pattern
    for bad in ("? ? ?", "K1ABC W9XYZ RR73", "? ? -11", "K1ABC", "K1ABC/P ? ?"):
        with pytest.raises(ValueError):
            ft8.hint_insert_text(ft8.hint_state(1), bad, 0)
    e = np.zeros(1, sh.ENTRY_DTYPE)[0]
    for kind in (0, 4, 255):
        e["kind"] = kind
        assert ft8.hint_hypothesis(e) is None and sh.hypothesis(e) is None


def test_host_helpers_under_asan_ubsan(tmp_path):
    """a program of its own (tests/host_asan/hint_asan_main.c) linked with csrc/ft8_hint.c and ft8_pack.c; nothing is loaded into python"""
    exe = str(tmp_path / "hint_asan")
    csrc = os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_asan", "hint_asan_main.c"), os.path.join(csrc, "ft8_hint.c"),
                           os.path.join(csrc, "ft8_pack.c"), "-lm", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "hint_asan ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


def test_struct_layouts_against_the_c_compiler(ft8, tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "ft8gpu.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(ft8gpu_hint_entry),
 offsetof(ft8gpu_hint_entry, b), offsetof(ft8gpu_hint_entry, stamp), offsetof(ft8gpu_hint_entry, kind), offsetof(ft8gpu_hint_entry, used),
 offsetof(ft8gpu_hint_entry, phase), sizeof(ft8gpu_hint_state), offsetof(ft8gpu_hint_state, cursor), offsetof(ft8gpu_hint_state, slot),
 sizeof(ft8gpu_hint_info), offsetof(ft8gpu_hint_info, ntried), offsetof(ft8gpu_hint_info, results), offsetof(ft8gpu_hint_info, index),
 sizeof(ft8gpu_hint_params), offsetof(ft8gpu_hint_params, max_age), offsetof(ft8gpu_hint_params, use_phase), FT8GPU_HINT_ENTRIES); return 0; }'''
    src, exe = tmp_path / "t.c", str(tmp_path / "t")
    src.write_text(prog)
    subprocess.check_call(["gcc", "-std=gnu17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    vals = list(map(int, subprocess.check_output([exe]).split()))
    e, s, i = ft8.HINT_ENTRY_DTYPE, ft8.HINT_STATE_DTYPE, ft8.HINT_INFO_DTYPE
    assert vals == [e.itemsize, e.fields["b"][1], e.fields["stamp"][1], e.fields["kind"][1], e.fields["used"][1], e.fields["phase"][1],
                    s.itemsize, s.fields["cursor"][1], s.fields["slot"][1], i.itemsize, i.fields["ntried"][1], i.fields["results"][1],
                    i.fields["index"][1], ctypes.sizeof(ft8.HintParams), ft8.HintParams.max_age.offset, ft8.HintParams.use_phase.offset,
                    ft8.HINT_ENTRIES]
    assert vals[:1] + vals[6:7] + vals[9:10] + vals[13:14] == [16, 8208, 16, 20]


# ---- the stream scenario ---------------------------------------------------------------------------------------------------------

def _is_report(text):
    last = text.split()[-1]
    return len(last) >= 3 and last[-3] in "+-"                          # -11, R-08


def test_stream_scenario_gains_report_steps(oracle, ft8):
    """3 receivers x 4 slots of QSOs that advance CQ -> call -> report -> R-report -> RR73 (hint_craft.scenario), the last two
    slots too weak for BP: the call hints gain report-step messages that the expected messages with derive cannot list, and
    nothing that was not on the air is accepted"""
    iq, texts = hc.scenario(oracle)
    R, S = iq.shape[:2]
    stages = sm.oracle_stages(oracle, iq.reshape(R * S, 2, -1))
    msgs, n, nbs, state = sh.decode_hinted(oracle, iq, stages=stages, **SCENARIO)
    gained, reports, wrong = [0] * S, 0, 0
    for r in range(R):
        for s in range(S):
            assert not msgs[r, s, :nbs[r, s, 0]]["pad"][:, 2].any()
            for k in range(int(nbs[r, s, 0]), int(nbs[r, s, 1])):
                t = msgs[r, s, k]["text"].decode()
                assert msgs[r, s, k]["pad"][2] == 3
                gained[s] += t in texts[r][s]
                wrong += t not in texts[r][s]
                reports += t in texts[r][s] and _is_report(t)
    em, en, enbs, _ = smt.decode_expected(oracle, iq, derive=True, stages=stages)
    by_match = [t.decode() for r in range(R) for s in range(S) for t in em[r, s, enbs[r, s, 0]:enbs[r, s, 1]]["text"]]
    match_reports = sum(1 for t in by_match if _is_report(t))
    print(f"scenario: call hints gain {gained} per slot ({reports} report steps), {wrong} not planted; matching with derive gains "
          f"{len(by_match)} ({match_reports} report steps)")
    assert wrong == 0 and gained[0] == 0 and reports >= 3 and reports > match_reports
    assert (state["slot"] == S).all() and (state["entry"]["used"].sum(axis=1) > 20).all()
