"""CPU tests of the expected messages (include/ft8gpu.h "expected messages"): the restatement tests/ft8_spec_match.py on the
constructed cases of tests/match_craft.py -- each case has the property it is named for, and the frozen fixture
tests/golden/match_constructed.npz (which the device is held to as well) is reproduced; the update rule on fabricated
records; the host helpers of csrc/ft8_pack.c against the restatement and under ASan + UBSan; the restatement on radio frames
and on the 3 x 4 stream scenario.  No GPU is used here."""
import os
import subprocess

import numpy as np
import pytest

import ap_craft as ac
import callhash_craft as cc
import ft8_spec_match as smt
import ft8_spec_messages as sm
import match_craft as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc"), "-j8"])
    m.load_library()
    return m


@pytest.fixture(scope="module")
def built(oracle, ft8):
    cases = mc.build_cases(oracle)
    cfgs = mc.configs(cases)
    placed = mc.place(cases)
    return cases, cfgs, placed, mc.expected(oracle, placed, cfgs)


# ---- the constructed cases -----------------------------------------------------------------------------------------------------

def test_frozen_constructed_fixture(built):
    cases, cfgs, placed, want = built
    d = mc.load_golden()
    assert d["configs"] == cfgs and d["where"] == placed["where"]
    for key in ("mag", "counts", "status_in"):
        assert np.array_equal(d[key], placed[key]), key
    assert d["cands"].tobytes() == placed["cands"].tobytes() and d["states"].tobytes() == placed["states"].tobytes()
    for name, _age, _gate in cfgs:
        status, info = want[name]
        assert d["status_" + name].tobytes() == status.tobytes(), name
        assert d["info_" + name].tobytes() == info.tobytes(), name


def test_constructed_cases_are_what_they_are_named_for(oracle, ft8, built):
    cases, cfgs, placed, want = built
    by = {c["name"]: (fr, c) for fr in cases for c in fr["cands"]}
    at = placed["where"]

    def info(config, name):
        return want[config][1][at[name]]

    def status(config, name):
        return want[config][0][at[name]].view(ft8.STATUS_DTYPE)[0]

    # a: accepted at a gate equal to nhard, refused with 2 at one below; the record is that of a BP success
    for e in (12, 30, 45):
        name = f"a_{e}_errors"
        fr, c = by[name]
        i1, i0 = info(f"gate_{e}", name), info(f"gate_{e - 1}", name)
        assert (i1["result"], i1["nhard"], i1["index"]) == (1, e, c["index"]) and (i0["result"], i0["nhard"], i0["index"]) == (2, e, c["index"])
        assert i1["metric"] == i0["metric"]
        rec, before = status(f"gate_{e}", name), placed["status_in"][at[name]].view(ft8.STATUS_DTYPE)[0]
        assert rec["ok"] == 1 and rec["ldpc_errors"] == 0 and rec["iters"] == before["iters"] and rec["text"].decode() == c["text"]
        assert rec["crc_extracted"] == rec["crc_calculated"] == sm.crc_of_payload(rec["a91"]) and rec["pad"] == 0
        assert want[f"gate_{e - 1}"][0][at[name]].tobytes() == placed["status_in"][at[name]].tobytes()
    assert info("gate_0", "a_0_errors")["result"] == 1 and info("gate_0", "a_12_errors")["result"] == 2
    # b, d: the smallest index of equal payloads across a round seam; lane 63 of the last round
    for name in ("b_63_64", "b_0_511", "d_511", "d_448", "d_0"):
        fr, c = by[name]
        i = info("open", name)
        assert (i["result"], i["index"], i["nhard"]) == (1, c["index"], c["nhard"]), name
    for lo, hi in ((63, 64), (0, 511)):
        e = by[f"b_{lo}_{hi}"][0]["state"][0]["entry"]
        assert e["payload"][lo].tobytes() == e["payload"][hi].tobytes() and e["used"][lo] and e["used"][hi]
    # c: two different payloads with the same metric, the smaller index wins whichever was written first
    for first, second in ((70, 200), (450, 130)):
        name = f"c_{first}_{second}"
        fr, c = by[name]
        f, i = at[name]
        llr = oracle.llr(placed["mag"][f], placed["cands"][f, i])
        h, w = smt.so.hard_and_weights(llr)
        e = fr["state"][0]["entry"]
        m = [int(((smt.codeword(e["payload"][j].tobytes()) ^ h).astype(np.int64) * w).sum()) for j in (first, second)]
        assert e["payload"][first].tobytes() != e["payload"][second].tobytes() and m[0] == m[1] == info("open", name)["metric"]
        assert info("open", name)["index"] == min(first, second) and info("open", name)["nhard"] == c["nhard"]
    # e: tables by their number of live entries under max_age = AGE, dead and expired entries in between
    for nlive in (0, 1, 63, 64, 65, 511, 512):
        fr = next(fr for fr in cases if fr["name"] == f"e_{nlive}_live")
        live = smt.live_entries(fr["state"][0], mc.AGE)
        assert live.size == nlive and smt.live_entries(fr["state"][0], 0).size >= nlive
        e = fr["state"][0]["entry"]
        if nlive < 512:
            assert (e["used"] == 0).any() or nlive == 511
            assert smt.live_entries(fr["state"][0], 0).size > nlive or nlive == 511
        for c in fr["cands"]:
            i = info("aged", c["name"])
            if nlive == 0:
                assert i.tobytes() == bytes(8) and want["aged"][0][at[c["name"]]].tobytes() == placed["status_in"][at[c["name"]]].tobytes()
            elif "index_aged" in c:
                assert (i["result"], i["index"], i["nhard"]) == (1, c["index_aged"], 10), c["name"]
            else:
                assert i["index"] in live, c["name"]
            if "never" in c:
                assert info("open", c["name"])["index"] != c["never"] and info("open", c["name"])["nhard"] > 40
    # f: an age exactly at the limit is live, one beyond is not, across the wrap of the slot counter too; max_age 0 never expires
    for name, (fr, c) in by.items():
        if name.startswith("f_"):
            assert (info("open", name)["result"], info("open", name)["index"]) == (1, 77)
            i = info("aged", name)
            assert (i["index"] == 77 and i["nhard"] == 5) == c["live_aged"] and (i["index"] == 300) == (not c["live_aged"]), name
    assert by["f_wrapped_at_limit"][0]["state"][0]["entry"]["stamp"][77] > 0xFFFFFF00
    # g: every weight saturated: the metric is 174 * 255 at the complement; the all-zero payload is 5 and never accepted
    i = info("open", "g_all_saturated")
    assert (i["result"], i["nhard"], i["index"], i["metric"]) == (5, 174, 9, 174 * 255)
    assert (info("open", "g_zero_payload")["result"], info("gate_0", "g_zero_payload")["result"]) == (5, 5)
    # h: unpack77 refuses the payload; the gate comes first
    assert info("open", "h_unpack_refuses")["result"] == 4 and info("gate_0", "h_unpack_refuses")["result"] == 2
    # i: soft bits that are not finite: nothing is compared
    for name, (fr, c) in by.items():
        if name.startswith("i_"):
            i = info("open", name)
            if c.get("result") == 6:
                assert i.tobytes() == bytes([6, 0, 0, 0, 0, 0, 0, 0]), name
            else:
                assert (i["result"], i["index"]) == (1, 0), name
    # j: garbage in payload bits 77..79, used, kind, cursor and pad changes nothing; the accepted a91 has clean bits
    fr = next(fr for fr in cases if fr["name"] == "j_garbage")
    e = fr["state"][0]["entry"]
    assert (e["payload"][e["used"] != 0][:, 9] & 7).all() and (e["used"][e["used"] != 0] > 1).all() and fr["state"][0]["cursor"] >= 512
    for c in fr["cands"]:
        i, rec = info("open", c["name"]), status("open", c["name"])
        assert (i["result"], i["index"], i["nhard"]) == (1, c["index"], 6) and rec["text"].decode() == c["text"]
        assert rec["a91"][:10].tobytes() == smt.payload77(ft8.pack77(c["text"]))[:9] + bytes([rec["a91"][9]])
    # records that do not qualify are copied, their info is zero; records behind the counts keep their bytes
    st = placed["status_in"].view(ft8.STATUS_DTYPE).reshape(placed["cands"].shape)
    ncopied = 0
    for f in range(len(placed["counts"])):
        for i in range(placed["cands"].shape[1]):
            if i >= placed["counts"][f]:
                assert want["open"][1][f, i].tobytes() == bytes([mc.FILL]) * 8 and (want["open"][0][f, i] == mc.FILL).all()
            elif st[f, i]["ok"] != 0 or st[f, i]["ldpc_errors"] == 0:
                ncopied += 1
                assert want["open"][1][f, i].tobytes() == bytes(8) and want["open"][0][f, i].tobytes() == placed["status_in"][f, i].tobytes()
    assert ncopied >= 10
    results = {int(r) for name in want for f in range(len(placed["counts"])) for r in want[name][1][f, :placed["counts"][f]]["result"]}
    assert results == {0, 1, 2, 4, 5, 6}


# ---- the update rule -------------------------------------------------------------------------------------------------------------

def _find(ft8, st, text):
    """(index, kind, stamp, used) of the entry that holds text's payload, or None"""
    p = smt.payload77(ft8.pack77(text))
    e = st["entry"]
    for j in range(smt.ENTRIES):
        if e["used"][j] and smt.payload77(e["payload"][j].tobytes()) == p:
            return j, int(e["kind"][j]), int(e["stamp"][j]), int(e["used"][j])
    return None


@pytest.fixture(scope="module")
def update_records(oracle, ft8):
    return cc.frames(oracle, mc.update_layout(), 0x0DD)


def test_update_rule_on_fabricated_records(oracle, ft8, update_records):
    msgs, n_msgs, printed = update_records
    state = smt.update(msgs, n_msgs, derive=True)
    plain = smt.update(msgs, n_msgs, derive=False)
    assert (state["slot"] == 6).all() and (plain["slot"] == 6).all() and (state["pad"] == 0).all()
    st = state[0]
    # heard entries; a repeat refreshes the stamp and adds nothing
    assert _find(ft8, st, "CQ K1ABC FN42")[1:3] == (0, 3) and _find(ft8, plain[0], "CQ K1ABC FN42")[1:3] == (0, 3)
    # derived, refreshed by a later message of the same pair: "K1ABC W9XYZ R-09" (slot 1) derives "W9XYZ K1ABC RR73" again
    assert _find(ft8, st, "W9XYZ K1ABC RR73")[1] == 1 and _find(ft8, st, "W9XYZ K1ABC RR73")[2] == 3
    assert _find(ft8, plain[0], "W9XYZ K1ABC RR73") is None
    # heard over derived: "W9XYZ K1ABC RRR" was derived in slot 0 and heard in slot 1; derived over heard (slot 3) keeps 0
    assert _find(ft8, st, "W9XYZ K1ABC RRR")[1:3] == (0, 3)
    assert _find(ft8, st, "K1ABC W9XYZ 73")[1:3] == (0, 3)                      # derived in slot 0, heard in slot 3
    assert _find(ft8, st, "K1ABC W9XYZ RR73")[1] == 1
    # /R travels with its call; ir is 0 in what "R EM48" derives
    assert _find(ft8, st, "W9XYZ K1ABC/R RRR")[1] == 1 and _find(ft8, st, "W9XYZ/R K1ABC 73")[1] == 1
    # nothing else derives: CQ and the other tokens, hashed fields, i3 = 2, type 4, free text, telemetry
    for call in ("K1JT", "PJ4/K1ABC"):
        for j in np.flatnonzero(st["entry"]["used"]):
            rc, text = oracle.unpack77(st["entry"]["payload"][j].tobytes())
            assert not (st["entry"]["kind"][j] == 1 and call in text.split()), text
    derived_texts = sorted(oracle.unpack77(st["entry"]["payload"][j].tobytes())[1] for j in np.flatnonzero(st["entry"]["kind"] == 1))
    assert all(t.split()[-1] in ("RRR", "RR73", "73") and "<" not in t and "/P" not in t for t in derived_texts), derived_texts
    assert _find(ft8, st, "W9XYZ/P K1ABC/P RRR") is None
    # without derive the table holds exactly the distinct payloads heard; every written payload has clean bits 77..79
    heard = {smt.payload77(msgs[0, s, k]["a91"][:10].tobytes()) for s in range(6) for k in range(min(max(int(n_msgs[0, s]), 0), 50))}
    e = plain[0]["entry"]
    assert {e["payload"][j].tobytes() for j in np.flatnonzero(e["used"])} == heard and plain[0]["cursor"] == len(heard)
    assert (state["entry"]["payload"][..., 9] & 7 == 0).all()
    # counts outside [0, 50]: 70 reads 50 records (whatever bytes they hold), -3 reads none
    assert n_msgs[0, 4] == 70 and n_msgs[0, 5] == -3
    # the ring wraps past 512: receiver 1 wrote more than 512 new entries, the oldest are gone, the cursor is in 1..512
    st1 = state[1]
    assert (st1["entry"]["used"] == 1).all() and 1 <= st1["cursor"] <= 512
    assert set(np.unique(st1["entry"]["stamp"])) <= set(range(6)) and st1["entry"]["stamp"].min() > 0
    # a single slot at a time leaves the same bytes
    step = None
    for s in range(6):
        step = smt.update(msgs[:, s:s + 1], n_msgs[:, s:s + 1], step, derive=True)
    assert step.tobytes() == state.tobytes()


def test_update_refreshes_an_expired_entry_and_matching_sees_it_again(oracle, ft8):
    st = smt.new_state()
    smt.insert(st[0], ft8.pack77("CQ K1ABC FN42"), 0)
    st[0]["slot"] = 50
    assert smt.live_entries(st[0], 10).size == 0 and smt.live_entries(st[0], 0).size == 1 and st[0]["entry"]["used"][0] == 1
    smt.insert(st[0], ft8.pack77("CQ K1ABC FN42"), 1)
    assert smt.live_entries(st[0], 10).tolist() == [0] and st[0]["cursor"] == 1 and st[0]["entry"]["kind"][0] == 0


def test_host_helpers_equal_the_restatement(oracle, ft8):
    rng = np.random.default_rng(0x4E1)
    got, want = ft8.expect_state(), smt.new_state()
    got[:] = np.frombuffer(rng.integers(0, 256, smt.STATE_DTYPE.itemsize, dtype=np.uint8).tobytes(), ft8.EXPECT_STATE_DTYPE)
    ft8.expect_reset(got)
    assert got.tobytes() == want.tobytes()
    pool = [mc.random_payload(rng) for _ in range(300)]
    for step in range(1500):
        p = np.array(pool[int(rng.integers(0, len(pool)))] if rng.integers(0, 3) else mc.random_payload(rng))
        p[9] |= int(rng.integers(0, 8))
        kind = int(rng.integers(0, 2))
        if step % 97 == 0:
            got[0]["slot"] = want[0]["slot"] = int(rng.integers(0, 1 << 32))
        if step == 700:                                               # a caller-built state: cursor past 512, used above 1
            for s in (got, want):
                s[0]["cursor"] = 0xFFFFFDFF
                s[0]["entry"]["used"][5] = 0x80
        ft8.expect_insert(got, p, kind)
        smt.insert(want[0], p.tobytes(), kind)
    assert got.tobytes() == want.tobytes() and (want["entry"]["used"] != 0).sum() > 400
    for text in ("K1ABC W9XYZ RR73", "CQ DX K1JT FN20", "<K1ABC> W9XYZ -05", "TNX BOB 73 GL"):
        ft8.expect_insert_text(got, text)
        smt.insert(want[0], ft8.pack77(text), 0)
    assert got.tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        ft8.expect_insert_text(got, "THIS IS NO FT8 MESSAGE AT ALL")
    with pytest.raises(ValueError):
        ft8.expect_insert(got, pool[0], 2)
    assert got.tobytes() == want.tobytes()
    assert ft8.EXPECT_STATE_DTYPE == smt.STATE_DTYPE and ft8.MATCH_INFO_DTYPE == smt.INFO_DTYPE


def test_host_helpers_under_asan_ubsan(tmp_path):
    """a program of its own (tests/host_asan/expect_asan_main.c) linked with csrc/ft8_pack.c; nothing is loaded into python"""
    exe = str(tmp_path / "expect_asan")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_asan", "expect_asan_main.c"),
                           os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc", "ft8_pack.c"), "-lm", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "expect_asan ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


def test_struct_layouts_against_the_c_compiler(ft8, tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "ft8gpu.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(ft8gpu_expect_entry), offsetof(ft8gpu_expect_entry, stamp),
 sizeof(ft8gpu_expect_state), offsetof(ft8gpu_expect_state, cursor), offsetof(ft8gpu_expect_state, slot), sizeof(ft8gpu_match_info),
 offsetof(ft8gpu_match_info, metric), sizeof(ft8gpu_expect_params), FT8GPU_EXPECT_ENTRIES, FT8GPU_MATCH_MAX_HARD_ERRORS); return 0; }'''
    src, exe = tmp_path / "t.c", str(tmp_path / "t")
    src.write_text(prog)
    subprocess.check_call(["gcc", "-std=gnu17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    vals = list(map(int, subprocess.check_output([exe]).split()))
    s = ft8.EXPECT_STATE_DTYPE
    assert vals == [16, 12, 8208, s.fields["cursor"][1], s.fields["slot"][1], 8, 4, 12, ft8.EXPECT_ENTRIES, ft8.MATCH_MAX_HARD_ERRORS]
    assert C_sizeof(ft8.ExpectParams) == 12


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


# ---- radio frames ----------------------------------------------------------------------------------------------------------------

def radio_tables(ft8, planted, seed=0x7AB1E, unrelated=236):
    """one table per frame: the frame's planted messages and `unrelated` others, shuffled over the 512 entries"""
    rng = np.random.default_rng(seed)
    states = smt.new_state(len(planted))
    for f, texts in enumerate(planted):
        payloads = [ft8.pack77(t) for t in texts] + mc.unrelated_payloads(rng, unrelated, texts)
        for j, p in zip(rng.permutation(smt.ENTRIES)[:len(payloads)], payloads):
            mc.put(states[f], int(j), p)
    return states


def test_restatement_on_radio_frames_gains_and_accepts_nothing_outside(oracle, ft8):
    """the frames of ap_craft.RADIO_SEEDS with their planted messages and 236 unrelated ones in the table: at the recommended
    gate matching gains planted messages over BP and accepts nothing that is not planted; on the noise frames nothing at all"""
    iq, planted = ac.radio_frames(oracle)
    mag, cands, counts, status = sm.oracle_stages(oracle, iq)
    states = radio_tables(ft8, planted)
    out, info = smt.match_candidates(oracle, mag, cands, counts, status, states, 0, ft8.MATCH_MAX_HARD_ERRORS)
    st_in, st_out = status.view(ft8.STATUS_DTYPE).reshape(cands.shape), out.view(ft8.STATUS_DTYPE).reshape(cands.shape)
    gained = accepted = 0
    for f in range(len(planted)):
        bp = {st_in[f, i]["text"].decode() for i in range(counts[f]) if st_in[f, i]["ok"]}
        new = set()
        for i in range(counts[f]):
            if info[f, i]["result"] == 1:
                accepted += 1
                text = st_out[f, i]["text"].decode()
                assert text in planted[f], (f, i, text, info[f, i])
                assert info[f, i]["nhard"] <= ft8.MATCH_MAX_HARD_ERRORS
                new.add(text)
        gained += len(new - bp)
    print(f"radio frames: {accepted} candidates accepted, {gained} planted messages gained over BP")
    assert gained >= 1 and accepted >= gained
    assert {int(r) for f in range(len(planted)) for r in info[f, :counts[f]]["result"]} >= {0, 1, 2}
    noise, _ = ac.radio_frames(oracle, ac.NOISE_SEEDS, 0)
    nmag, ncands, ncounts, nstatus = sm.oracle_stages(oracle, noise)
    nstates = radio_tables(ft8, [[] for _ in ac.NOISE_SEEDS], unrelated=256)
    _out, ninfo = smt.match_candidates(oracle, nmag, ncands, ncounts, nstatus, nstates, 0, ft8.MATCH_MAX_HARD_ERRORS)
    nst = nstatus.view(ft8.STATUS_DTYPE).reshape(ncands.shape)
    failing = sum(int(((nst[f, :ncounts[f]]["ok"] == 0) & (nst[f, :ncounts[f]]["ldpc_errors"] != 0)).sum()) for f in range(len(ncounts)))
    tried = sum(int((ninfo[f, :ncounts[f]]["result"] != 0).sum()) for f in range(len(ncounts)))
    print(f"noise frames: {tried} candidates compared, none accepted")
    assert tried == failing > 0 and not any((ninfo[f, :ncounts[f]]["result"] == 1).any() for f in range(len(ncounts)))


# ---- the stream scenario ---------------------------------------------------------------------------------------------------------

def test_stream_scenario_gains_repeats_and_closings(oracle, ft8):
    """3 receivers x 4 slots (match_craft.scenario): slot 2 repeats slot 0 about 10 dB weaker and gains from the heard entries;
    slot 3 closes slot 1's messages and gains only with derive = 1; nothing that was not on the air is accepted"""
    iq, texts = mc.scenario(oracle)
    R, S = iq.shape[:2]
    stages = sm.oracle_stages(oracle, iq.reshape(R * S, 2, -1))
    with_derive = mc.scenario_gains(oracle, iq, texts, ft8.MATCH_MAX_HARD_ERRORS, True, stages)
    without = mc.scenario_gains(oracle, iq, texts, ft8.MATCH_MAX_HARD_ERRORS, False, stages)
    print("gained (planted, not planted) per slot: derive", with_derive, "no derive", without)
    assert with_derive[0] == (0, 0) and without[0] == (0, 0)                 # an empty table gains nothing
    assert with_derive[2][0] >= 1 and without[2][0] >= 1
    assert with_derive[3][0] >= 1 and without[3][0] == 0
    assert all(bad == 0 for _good, bad in with_derive + without)
    # one call over four slots leaves what four calls of one slot leave
    msgs, n, nbs, state = smt.decode_expected(oracle, iq, max_hard_errors=ft8.MATCH_MAX_HARD_ERRORS, stages=stages)
    st = None
    for s in range(S):
        sub = tuple(a.reshape(R, S, *a.shape[1:])[:, s] for a in stages)
        m1, n1, b1, st = smt.decode_expected(oracle, iq[:, s:s + 1], state=st, max_hard_errors=ft8.MATCH_MAX_HARD_ERRORS, stages=sub)
        assert m1.tobytes() == msgs[:, s:s + 1].tobytes() and np.array_equal(n1, n[:, s:s + 1]) and np.array_equal(b1, nbs[:, s:s + 1])
    assert st.tobytes() == state.tobytes()
    assert all(msgs[r, s, k]["pad"][2] == (1 if k >= nbs[r, s, 0] else 0) for r in range(R) for s in range(S) for k in range(n[r, s]))
