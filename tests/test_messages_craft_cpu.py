"""CPU proof that the constructed families of tests/messages_craft.py have the properties they are named for, through the numpy
restatements alone (tests/ft8_spec_messages.py, tests/ft8_spec_multipass.py), and that they discriminate: every wrong variant of
the rule (float32 arithmetic, > for >=, upper median, a counted sentinel, an unclamped freq_offset, sub-steps not taken mod 2,
tones from the payload with a recomputed CRC, a swapped Gray entry, a mask without the block-range test) changes at least one
record or cell of the family built against it.  tests/test_gpu_messages_constructed.py sends the same families through the
kernels."""
import json
import os
import subprocess

import numpy as np
import pytest

import ft8_spec_messages as sm
import ft8_spec_multipass as smp
import messages_craft as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc"), "-j8"])
    m.load_library()
    return m


def _filled(ft8, B):
    return np.full((B, 50 * 64), mc.FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(B, 50)


def _groups(name):
    return mc.family(name)["groups"]


def _differing(group, variant, kinds=None):
    """the cases (or, without case records, the (frame, slot) pairs) whose record changes under a wrong variant of the rule"""
    a, n = mc.collect(group)
    b, bn = mc.collect(group, variant=variant)
    assert np.array_equal(n, bn)
    bad = [(f, j) for f in range(len(n)) for j in range(int(n[f])) if a[f, j].tobytes() != b[f, j].tobytes()]
    if kinds is None:
        return bad
    by_place = {(c["frame"], c["index"]): c for c in group["cases"]}
    return [by_place[(f, int(a[f, j]["cand_index"]))] for f, j in bad if by_place[(f, int(a[f, j]["cand_index"]))].get("kind") in kinds]


@pytest.mark.parametrize("name", mc.FAMILIES)
def test_the_rule_of_the_generator_is_the_restatement(ft8, name):
    """variant None of messages_craft.collect / mask_cells == ft8_spec_messages.collect, ft8_spec_multipass.append / mask,
    byte for byte: the wrong variants below are wrong versions of the rule the device is held to, not of another one"""
    assert sum(len(g["counts"]) for g in _groups(name)) <= 16
    for g in _groups(name):
        B = len(g["counts"])
        a, an = mc.collect(g)
        b, bn = sm.collect(g["mags"], g["cands"], g["counts"], g["status"], min_score=g["min_score"], msgs=_filled(ft8, B))
        assert np.array_equal(an, bn) and a.tobytes() == b.tobytes(), sm.check(a, an, b, bn)
        if "append" in g:
            ap = g["append"]
            a, an = mc.collect(g, base=ap["base"], msgs=ap["msgs"], n_msgs=ap["n_msgs"])
            b, bn = smp.append(g["mags"], ap["base"], g["cands"], g["counts"], g["status"], ap["msgs"], ap["n_msgs"], min_score=g["min_score"])
            assert np.array_equal(an, bn) and a.tobytes() == b.tobytes(), sm.check(a, an, b, bn)


def _case_records(group):
    """(case, record) pairs: every case of these families is a unique decoded message, so record j of a frame is candidate j"""
    msgs, n = mc.collect(group)
    out = []
    for c in group["cases"]:
        r = msgs[c["frame"], c["index"]]
        assert c["index"] < n[c["frame"]] and int(r["cand_index"]) == c["index"]
        out.append((c, r))
    return out


def test_snr_steps_sit_on_every_threshold(ft8):
    """160 cases, two per threshold: S, evaluated as the rule does, is within 2^-24 of (nsym P[nb]) T[d] on the stated side; all
    80 values of snr_db occur; float32 arithmetic gets at least 40 of the 80 steps wrong; the order of the double sum none"""
    (g,) = _groups("snr_steps")
    base = sm.noise_baseline(g["mags"])
    P, T = sm.power_table(), sm.threshold_table()
    pairs = _case_records(g)
    assert len(pairs) == 160 and sorted({c["step"] for c, _ in pairs}) == list(range(80))
    gaps = {"above": [], "below": []}
    raw = g["status"].view(np.uint8).reshape(len(g["counts"]), g["cap"], 48)
    reversed_differs = 0
    for c, r in pairs:
        f, i, d = c["frame"], c["index"], c["step"]
        snr, S, nsym, nb = mc.snr_of(g["mags"][f], base[f], g["cands"][f, i], raw[f, i, 10:22].tobytes(), parts=True)
        assert (nsym, nb) == (c["nsym"], c["nb"]) and snr == int(r["snr_db"]) == c["want"], c
        X = (float(nsym) * float(P[nb])) * float(T[d])
        assert (S >= X) == (c["side"] == "above"), c
        gap = abs(S - X) / X
        assert gap <= 2.0 ** -24 and gap == c["gap"], c
        gaps[c["side"]].append(gap)
        # the same 79 powers summed in reverse order, in double
        tones = mc.tones_of(raw[f, i, 10:22].tobytes())
        cd = g["cands"][f, i]
        cells = [g["mags"][f][(int(cd["time_offset"]) + k) * 1024 + (int(cd["time_sub"]) & 1) * 512 + (int(cd["freq_sub"]) & 1) * 256
                              + int(cd["freq_offset"]) + int(tones[k])] for k in range(79) if 0 <= int(cd["time_offset"]) + k < 92]
        Sr = 0.0
        for v in reversed(cells):
            Sr = Sr + float(P[v])
        reversed_differs += sm.snr_db(Sr, nsym, nb) != snr
    assert {int(r["snr_db"]) for _, r in pairs} == set(range(-30, 50))
    assert {c["nsym"] for c, _ in pairs} >= {79, 67, 32} and {c["nb"] for c, _ in pairs} == {30, 90, 150, 210}
    wrong = _differing(g, "float32", kinds={None})
    steps = {c["step"] for c in wrong}
    print(f"snr_steps: worst gap above {max(gaps['above']):.3e}, below {max(gaps['below']):.3e} (bound {2.0 ** -24:.3e}); "
          f"float32 variant wrong on {len(wrong)} of 160 cases, {len(steps)} of 80 steps; reversed double sum differs on {reversed_differs}")
    assert len(steps) >= 40
    rec = json.load(open(os.path.join(ROOT, "profiles", "messages_constructed.json")))["snr_steps"]     # python tests/messages_craft.py
    assert (rec["worst_gap_above"], rec["worst_gap_below"]) == (max(gaps["above"]), max(gaps["below"]))
    assert (rec["float32_wrong_cases"], rec["float32_wrong_steps"]) == (len(wrong), len(steps))
    assert reversed_differs == 0                                   # the summation order in double is NOT observable here
    for v in ("gt", "upper_median", "sentinel_high", "sentinel_zero", "unclamped", "subs_raw", "payload_tones"):
        assert _differing(g, v) == []                              # nothing else moves these cases


def test_snr_range_pins_the_ends_and_the_empty_sum(ft8):
    (g,) = _groups("snr_range")
    pairs = _case_records(g)
    for c, r in pairs:
        if c["want"] is not None:
            assert int(r["snr_db"]) == c["want"], c
    assert {c["nsym"] for c, _ in pairs if c["kind"] == "one_symbol"} == {1}
    none = [(c, r) for c, r in pairs if c["kind"] == "no_symbol"]
    assert len(none) == 8 and all(c["nsym"] == 0 and int(r["snr_db"]) == 49 for c, r in none)
    mid = [int(r["snr_db"]) for c, r in pairs if c["kind"] == "one_symbol" and c["want"] is None]
    assert len(mid) == 2 and all(-30 < s < 49 for s in mid)
    # > for >=: the empty sums sit exactly on equality (0 >= 0 at every step); no case with a symbol inside the waterfall does
    wrong = _differing(g, "gt", kinds={"no_symbol", "top", "bottom", "equal", "one_symbol"})
    assert len(wrong) == 8 and {c["kind"] for c in wrong} == {"no_symbol"}
    print(f"snr_range: > for >= wrong on {len(wrong)} records")


def test_noise_window_sizes_clamps_and_medians(ft8):
    (g,) = _groups("noise_window")
    pairs = _case_records(g)
    assert {c["window_size"] for c, _ in pairs if c["kind"] == "size"} == set(range(16, 33))
    for c, r in pairs:                                              # freq_hz and dt_s from the raw values
        cd = g["cands"][c["frame"], c["index"]]
        assert float(r["freq_hz"]) == (int(cd["freq_offset"]) + int(cd["freq_sub"]) / 2) * 6.25
        assert r["dt_s"] == np.float32(np.float32(int(cd["time_offset"]) + int(cd["time_sub"]) / 2) / np.float32(6.25))
    assert sorted(c["fo"] for c, _ in pairs if c["kind"] == "clamp") == sorted(mc.CLAMPING_FO)
    assert {(int(g["cands"][c["frame"], c["index"]]["time_sub"]), int(g["cands"][c["frame"], c["index"]]["freq_sub"]))
            for c, _ in pairs if c["kind"] == "subs"} >= {(2, 3), (3, 2), (254, 255), (255, 254)}
    # two-valued windows of even size: lower median, upper median and mean give three different snr_db
    base = sm.noise_baseline(g["mags"])
    raw = g["status"].view(np.uint8).reshape(len(g["counts"]), g["cap"], 48)
    three = 0
    for c, r in pairs:
        if c["kind"] == "two_valued" and c["window_size"] % 2 == 0:
            f, i = c["frame"], c["index"]
            args = (g["mags"][f], base[f], g["cands"][f, i], raw[f, i, 10:22].tobytes())
            lower, S, nsym, nb = mc.snr_of(*args, parts=True)
            upper = mc.snr_of(*args, variant="upper_median")
            assert nb == 100 and lower == int(r["snr_db"])
            assert len({lower, upper, sm.snr_db(S, nsym, 120)}) == 3, c
            three += 1
    assert three >= 3
    # all 0 / all 255 with half the window outside the waterfall: the median of the 16 columns inside
    for c, r in pairs:
        if c["kind"] in ("all_0", "all_255"):
            assert c["window_size"] == 16
            f, i = c["frame"], c["index"]
            assert mc.snr_of(g["mags"][f], base[f], g["cands"][f, i], raw[f, i, 10:22].tobytes(), parts=True)[3] == (0 if c["kind"] == "all_0" else 255)
    kinds = {"size", "clamp", "two_valued", "all_0", "all_255", "subs"}
    found = {v: _differing(g, v, kinds=kinds) for v in ("upper_median", "sentinel_high", "sentinel_zero", "unclamped", "subs_raw")}
    print("noise_window: records wrong under " + ", ".join(f"{v} {len(w)}" for v, w in found.items()))
    assert {c["kind"] for c in found["upper_median"]} >= {"two_valued"}
    assert {c["kind"] for c in found["sentinel_high"]} >= {"two_valued", "size"}
    assert {c["kind"] for c in found["sentinel_zero"]} >= {"all_255"}
    assert {c["kind"] for c in found["unclamped"]} == {"clamp"} and len(found["unclamped"]) == len(mc.CLAMPING_FO)
    assert {c["kind"] for c in found["subs_raw"]} == {"subs"} and len(found["subs_raw"]) == 8
    # the foreign base is not the waterfall's own
    assert (g["append"]["base"] != base).mean() > 0.9


def test_tones_show_a_wrong_tone_at_every_symbol(ft8):
    (g,) = _groups("tones")
    pairs = _case_records(g)
    kinds = [c["kind"] for c, _ in pairs]
    assert kinds.count("walking") == 91 and {"zero", "ones", "random", "crc_match", "crc_mismatch", "junk", "junk_clean"} <= set(kinds)
    base = sm.noise_baseline(g["mags"])
    for c, r in pairs:
        a = bytes(r["a91"])
        if c["kind"] == "crc_mismatch":
            assert sm.crc_in_a91(a) != so_crc(a)
        if c["kind"] in ("crc_match", "junk_clean"):
            assert sm.crc_in_a91(a) == so_crc(a)
        if c["kind"] == "junk":
            assert a[11] & 0x1F and np.array_equal(mc.tones_of(a), mc.tones_of(a[:11] + bytes([a[11] & 0xE0])))
        assert -20 <= int(r["snr_db"]) <= 0                        # the right tones: the low cells only
    # one wrong tone at any one symbol position moves snr_db (every position of one record of each kind)
    seen = set()
    for c, r in pairs:
        if c["kind"] in seen:
            continue
        seen.add(c["kind"])
        f, i = c["frame"], c["index"]
        tones = mc.tones_of(bytes(r["a91"]))
        for k in range(79):
            t = tones.copy()
            t[k] = (t[k] + 1 + k % 7) & 7
            S, nsym, nb = sm.snr_parts(g["mags"][f], base[f], g["cands"][f, i], t)
            assert (sm.snr_db(S, nsym, nb) != int(r["snr_db"])) == (0 <= int(g["cands"][f, i]["time_offset"]) + k < 92), (c, k)
    all_kinds = set(kinds)
    pay = _differing(g, "payload_tones", kinds=all_kinds)
    gray = _differing(g, "gray_swap", kinds=all_kinds)
    print(f"tones: records wrong under payload_tones {len(pay)}, gray_swap {len(gray)}")
    assert {c["kind"] for c in pay} >= {"crc_mismatch", "walking", "ones"} and not {c["kind"] for c in pay} & {"crc_match", "junk", "junk_clean", "zero"}
    assert len(gray) >= 100


def so_crc(a91):
    import ft8_spec_osd as so
    return so.crc14(list(mc.bits_of(a91)[:77]))


def test_dedup_counts(ft8):
    """the expected counts of the dedup family, collect and append, as literals"""
    want = {1: ([1, 0], [1, 0]), 63: ([50, 50], [50, 50]), 64: ([50, 7], [50, 50]), 65: ([50, 0], [50, 1]),
            120: ([50, 15, 50, 41], [50, 15, 50, 42]), 129: ([23, 23, 50, 20], [23, 23, 50, 20])}
    assert [g["cap"] for g in _groups("dedup")] == [1, 63, 64, 65, 120, 129]
    for g in _groups("dedup"):
        msgs, n = mc.collect(g)
        ap = g["append"]
        amsgs, an = mc.collect(g, base=ap["base"], msgs=ap["msgs"], n_msgs=ap["n_msgs"])
        assert (list(n), list(an)) == want[g["cap"]], g["cap"]
        for f in range(len(n)):                                    # unique (hash, text as strcmp sees it)
            keys = [(int(r["hash"]), sm._c_text(r.tobytes()[:25])) for r in msgs[f, :n[f]]]
            assert len(set(keys)) == len(keys)
    by_cap = {g["cap"]: g for g in _groups("dedup")}
    # the seams: the 50th unique message is candidate 62 / 62 / 63 / 64, the 51st (dropped) follows it
    for cap, at in ((63, 62), (64, 62), (65, 63), (120, 64)):
        msgs, n = mc.collect(by_cap[cap])
        assert n[0] == 50 and int(msgs[0, 49]["cand_index"]) == at, cap
    # counts outside [0, cap]: -1 reads as 0 and cap + 5 as cap
    assert list(by_cap[1]["counts"]) == [6, -1] and by_cap[63]["counts"][1] == 68 and by_cap[129]["counts"][1] == 134
    assert by_cap[65]["counts"][1] == -1
    assert sorted(int(v) for g in _groups("dedup") for v in g["append"]["n_msgs"]) == [-3, 0, 0, 0, 0, 0, 1, 1, 2, 3, 3, 10, 49, 49, 50, 77]
    # the text cases: frame 1 of cap 120
    msgs, n = mc.collect(by_cap[120])
    texts = [r.tobytes()[:25] for r in msgs[1, :n[1]]]
    assert sum(t.startswith(b"HELLO\0") for t in texts) == 1 and sum(t.startswith(b"ABCDEFGHIJKLMNOPQRSTUVWX") for t in texts) == 3
    assert sum(t[0] == 0 for t in texts) == 2
    assert {int(r["hash"]) for r in msgs[1, :n[1]]} >= {0x3FFF, 0x4000, 0xFFFF, 0x1234, 0}
    # the append of cap 120: frame 2 reaches 50 at candidate 79, in the middle of the second chunk; frame 3 drops candidate
    # 104 (a repeat of the first chunk) and 105 (a repeat of a seed record)
    amsgs, an = mc.collect(by_cap[120], base=by_cap[120]["append"]["base"], msgs=by_cap[120]["append"]["msgs"], n_msgs=by_cap[120]["append"]["n_msgs"])
    assert int(amsgs[2, 49]["cand_index"]) == 79 and max(int(r["cand_index"]) for r in amsgs[3, 3:an[3]]) == 83
    # three chunks: the single lane of the third carries a new message
    msgs, n = mc.collect(by_cap[129])
    assert int(msgs[0, n[0] - 1]["cand_index"]) == 128


def test_mask_edges_every_masked_cell_is_visible(ft8):
    (g,) = _groups("mask_edges")
    mk = g["mask"]
    mag = g["mags"]
    rule = mc.mask_cells(mk["msgs"], mk["first"], mk["n_msgs"])
    want = smp.mask(mag, mk["base"], mk["msgs"], mk["first"], mk["n_msgs"])
    assert mag.max() <= 127 and mk["base"].min() >= 128
    for f, cells in enumerate(rule):
        assert sorted(np.flatnonzero(want[f] != mag[f]).tolist()) == cells, f          # changed cells == the rule's set, exactly
        cols = np.array(cells, np.int64) % 512
        assert np.array_equal(want[f][cells], mk["base"][f].reshape(512)[cols])
    assert [len(c) > 0 for c in rule] == [True, True, True, True, True, False, False, False]
    assert len(rule[3]) > 3000                                                         # 50 records through the 256-thread stride loop
    assert {int(r["cand"]["time_offset"]) for r in mk["msgs"][0, :9]} == set(mc.MASK_TIME_OFFSETS)
    assert list(mk["first"]) == [0, -4, 0, 0, 1, 8, 0, 4] and list(mk["n_msgs"]) == [9, 27, 77, 50, 3, 6, 0, 4]
    for v in ("no_block_test", "unclamped", "subs_raw", "payload_tones", "gray_swap"):
        other = mc.mask_cells(mk["msgs"], mk["first"], mk["n_msgs"], variant=v)
        frames = [f for f in range(len(rule)) if other[f] != rule[f]]
        print(f"mask_edges: {v} changes the cell set of frames {frames}")
        assert frames, v
