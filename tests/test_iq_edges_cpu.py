"""CPU tests of the constructions in tests/iq_edges_craft.py: with the restatements tests/ft8_spec_refine.py and
tests/ft8_spec_subtract.py every named case is shown to be what it is named for, scaling by a power of two is shown to commute
with both rules where nothing under- or overflows, a NaN is shown to appear in the restatements' outputs only where a sample is
not finite, and three mutants of the scans are each shown to change a named case.  tests/test_gpu_refine.py and
tests/test_gpu_subtract.py hold the device to the same restatements on the same inputs.  No GPU is used here."""
import os
import subprocess

import numpy as np
import pytest

import ft8_spec_refine as sr
import ft8_spec_subtract as ss
import iq_edges_craft as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
RECORD_SAMPLES = ss.SPAN                                                 # 40 448


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc"), "-j8"])
    m.load_library()
    return m


@pytest.fixture(scope="module")
def edges(ft8, oracle):
    batch = ec.edges(ft8)
    return batch, ec.edges_expected(oracle, batch)


def subnormal(v):
    v = np.asarray(v, F32)
    return (v != 0) & (np.abs(v) < ec.TINY)


def decisions(want, at):
    r, s = want["refined"][at], want["info"][at]
    return int(r["e_best"]), int(s["k4"]), int(s["s_best"]), int(s["d_best"]), int(s["t_best"]), int(s["valid"])


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- every sample times a power of two ----------------------------------------------------------------------------------------------------

def test_scaled_cases_are_what_they_are_named_for(ft8, edges):
    (iq, msgs, refined, first, n, where), want = edges
    ref, info, out = want["refined"], want["info"], want["out"]
    clean = decisions(want, where["clean"])
    assert clean == (0, 4 * 321 + 2, 2576, 2, 2, 1) and np.abs(iq[where["clean"][0]]).max() == 0.5
    powers = lambda at: (np.concatenate([info[at]["pf"], info[at]["pt"]]), np.concatenate([ref[at]["pt"], ref[at]["pf"], ref[at]["noise"][None]]))
    changed = lambda at: int((bits(out[at[0]]) != bits(iq[at[0]])).sum())

    at = where["scaled_subnormal_powers"]
    sub_p, ref_p = powers(at)
    assert subnormal(sub_p).all() and subnormal(ref_p).all()             # every power, not just one
    assert decisions(want, at) == clean and changed(at) > 80000

    at = where["scaled_few_bits_left"]                                   # powers below 2^-141: eight bits and fewer, and other decisions
    sub_p, ref_p = powers(at)
    assert subnormal(sub_p).all() and (sub_p < 2.0 ** -141).all() and subnormal(ref_p).any() and (ref_p == 0).any()
    assert decisions(want, at) != clean and decisions(want, at)[4] == 0 and changed(at) > 80000

    for name in ("scaled_zero_powers", "scaled_subnormal_samples"):
        at = where[name]
        sub_p, ref_p = powers(at)
        assert bits(sub_p).tolist() == [0] * 10 and bits(ref_p).tolist() == [0] * 9, name      # every power is +0
        assert decisions(want, at) == (-16, 4 * 321 - 2, 2560 - 16, -2, -2, 1), name
        assert changed(at) > 80000, name                                 # the amplitudes are not zero: something is still subtracted
    f = where["scaled_zero_powers"][0]
    assert not subnormal(iq[f]).any() and (iq[f] != 0).all()
    _i, _t, A = ss.estimate_record(iq[f, 0], iq[f, 1], msgs[f, 0]["cand"], msgs[f, 0]["a91"].tobytes(), refined[f, 0], ss.twiddles())
    assert (A[0] != 0).all() and (A[1] != 0).all()
    f = where["scaled_subnormal_samples"][0]
    assert (subnormal(iq[f]) | (iq[f] == 0)).all() and subnormal(iq[f]).sum() > 90000

    at = where["scaled_partly_inf_powers"]
    sub_p, ref_p = powers(at)
    assert np.isinf(sub_p).any() and np.isfinite(sub_p).any() and np.isinf(ref_p).any() and np.isfinite(ref_p).any()
    assert int(info[at]["d_best"]) + 2 == int(np.argmax(np.isinf(info[at]["pf"]))) == 1      # the first +inf is the first maximum
    assert np.isfinite(out[at[0]]).all()

    at = where["scaled_inf_powers"]
    sub_p, ref_p = powers(at)
    assert (sub_p == np.inf).all() and decisions(want, at) == (-16, 4 * 321 - 2, 2560 - 16, -2, -2, 1)
    f = at[0]
    with np.errstate(all="ignore"):
        _i, _t, A = ss.estimate_record(iq[f, 0], iq[f, 1], msgs[f, 0]["cand"], msgs[f, 0]["a91"].tobytes(), refined[f, 0], ss.twiddles())
    assert np.isfinite(A[0]).all() and np.isfinite(A[1]).all() and np.isfinite(out[f]).all() and np.isfinite(iq[f]).all()
    assert changed(at) > 80000


def test_scaling_commutes_where_nothing_under_or_overflows(edges):
    """decisions equal, powers times 2^-2k and residual times 2^-k equal bit for bit: both rules are homogeneous, and a power of
    two changes no rounding while every intermediate stays a normal float"""
    (iq, msgs, refined, first, n, where), want = edges
    c = where["clean"]
    for name, k in ec.EXACT_EXP.items():
        at = where[name]
        assert bits(iq[at[0]]).tolist() != bits(iq[c[0]]).tolist()
        for key in ("info", "pair_info"):
            a, b = want[key][at], want[key][c]
            assert [int(a[x]) for x in ("k4", "s_best", "d_best", "t_best", "valid")] == [int(b[x]) for x in ("k4", "s_best", "d_best", "t_best", "valid")]
            for x in ("pf", "pt"):
                assert bits(np.ldexp(a[x], -2 * k)).tolist() == bits(b[x]).tolist(), (name, key, x)
        a, b = want["refined"][at], want["refined"][c]
        assert a["e_best"] == b["e_best"]
        for x in ("pt", "pf", "noise"):
            assert bits(np.ldexp(a[x], -2 * k)).tolist() == bits(b[x]).tolist(), (name, x)
        for key in ("out", "pair_out"):
            assert bits(np.ldexp(want[key][at[0]], -k)).tobytes() == bits(want[key][c[0]]).tobytes(), (name, key)


# ---- samples that are not finite --------------------------------------------------------------------------------------------------------------

def test_not_finite_cases_are_what_they_are_named_for(edges, oracle):
    (iq, msgs, refined, first, n, where), want = edges
    ref, info, out = want["refined"], want["info"], want["out"]
    c = where["clean"]
    # one +inf: every power is +inf, every scan keeps its first value, and the NaNs are inf - inf in the samples around it
    at = where["inf_sample"]
    assert (info[at]["pf"] == np.inf).all() and (info[at]["pt"] == np.inf).all() and decisions(want, at)[3:5] == (-2, -2)
    assert ref[at]["e_best"] == -16 and (ref[at]["pf"] == np.inf).all()
    assert int(np.isnan(want["pair_out"][at[0]]).sum()) == 545           # 17 segments of 32 samples and the sample itself
    # -inf beside +inf: powers that are NaN beside powers that are +inf
    for key in ("info", "pair_info"):
        p = np.concatenate([want[key][where["inf_pair"]]["pf"], want[key][where["inf_pair"]]["pt"]])
        assert np.isnan(p).any() and (p == np.inf).any() and not np.isfinite(p).any()
    at = where["nan_sample"]
    assert np.isnan(info[at]["pf"]).all() and np.isnan(info[at]["pt"]).all() and np.isnan(ref[at]["pf"]).all()
    assert decisions(want, at)[3:5] == (-2, -2) and ref[at]["e_best"] == -16      # nothing is greater than the NaN the scans start from
    j = np.argwhere(np.isnan(iq[at[0]]))
    assert j.tolist() == [[1, ec.S_REC + 512 * 3 + 200]] and bits(iq[at[0]])[tuple(j[0])] == ec.NAN_BITS
    # the four cases with a sample inside the record: few NaNs, so the comparison still holds the device on 95 % of the record
    for name in ("inf_sample", "inf_pair", "nan_sample", "nan_at_window_edge_inside"):
        f = where[name][0]
        for key in ("out", "pair_out"):
            assert np.isnan(want[key][f]).sum() < 0.05 * RECORD_SAMPLES, (name, key)
        assert 0 < np.isnan(want["pair_out"][f]).sum()

    # a NaN that no window reads: every record and every other sample are the clean frame's
    def same_as_clean(name, j, comp, refine_too=True):
        at = where[name]
        f = at[0]
        assert np.argwhere(np.isnan(iq[f])).tolist() == [[comp, j]]
        for key in ("info", "pair_info") if refine_too else ("info",):
            assert want[key][at].tobytes() == want[key][c].tobytes(), (name, key)
        if refine_too:
            assert ref[at].tobytes() == ref[c].tobytes(), name
        for key in ("out", "pair_out") if refine_too else ("out",):
            differ = np.argwhere(bits(want[key][f]) != bits(want[key][c[0]]))
            assert differ.tolist() == [[comp, j]] and bits(want[key][f])[comp, j] == ec.NAN_BITS, (name, key)    # the NaN itself is copied bit for bit

    same_as_clean("nan_outside", 47000, 0)
    lo, hi = ec.WINDOW
    assert (lo, hi) == (2048, 43520)
    same_as_clean("nan_at_window_edge_outside", lo - 1, 0)
    same_as_clean("nan_behind_window_edge_outside", hi, 1)
    # one sample further in, the first and the last power of the refine search are NaN
    same_as_clean("nan_at_window_edge_inside", lo, 0, refine_too=False)   # the subtraction at the hand-made e_best = 0 does not reach it
    at = where["nan_at_window_edge_inside"]
    r = ref[at]
    assert r["e_best"] == -16 and np.isnan(r["pt"][1]) and np.isnan(r["pf"]).all() and r["pt"][0] == 0 and np.isfinite(r["pt"][2])
    p = want["pair_info"][at]                                            # ... and the pair run follows the refine rule there
    assert (p["s_best"], p["d_best"], p["t_best"]) == (lo - 16, -2, -2) and np.isnan(p["pt"][:3]).all() and np.isfinite(p["pt"][3:]).all()
    at = where["nan_behind_window_edge_inside"]
    same_as_clean("nan_behind_window_edge_inside", hi - 1, 1)            # P(0, 16) is a NaN, is passed over, and is not an output
    pt_all = pt_all_of(iq[at[0]], msgs[at], sr.twiddles(oracle))
    assert np.isnan(pt_all[32]) and not np.isnan(pt_all[:32]).any()


def test_a_nan_appears_only_where_a_sample_is_not_finite(edges):
    """so the NaN-tolerant comparison of the GPU tests is byte for byte everywhere else"""
    (iq, msgs, refined, first, n, where), want = edges
    may = {where[name][0] for name in ec.NAN_OUTPUT_CASES}
    ustar = where["ustar_all_nan"][0]
    floats_of = lambda a: np.concatenate([np.ascontiguousarray(a[x], F32).reshape(-1) for x in a.dtype.names if a.dtype[x].base == F32])
    for f in range(len(n)):
        recs = slice(0, int(n[f]))
        nans = sum(int(np.isnan(floats_of(want[key][f, recs])).sum()) for key in ("refined", "info", "pair_info"))
        res = [int(np.isnan(want[key][f]).sum()) - int(np.isnan(iq[f]).sum()) for key in ("out", "pair_out")]   # beside the input's own
        if f in may:
            assert nans > 0 or max(res) > 0, f
        else:
            assert nans == 0 and res == [0, 0], f
    assert np.isnan(refined[ustar]["pf"]).any() and ustar not in may     # the NaNs of the u* cases are inputs and reach no output
    names = {v[0]: k for k, v in where.items()}
    assert {names[f] for f in may} == set(ec.NAN_OUTPUT_CASES)


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------------

def pt_all_of(x, m, tw):
    """the 33 powers of the refine rule's time search, as refine_record forms them"""
    T = 2 * int(m["cand"]["time_offset"]) + int(m["cand"]["time_sub"])
    Fq = 2 * int(m["cand"]["freq_offset"]) + int(m["cand"]["freq_sub"])
    tones = sr.tones_of_a91(m["a91"].tobytes())
    sym = 256 * T + sr.LEAD + 512 * np.arange(79, dtype=np.int64)
    with np.errstate(all="ignore"):
        return sr.powers(*sr.segment_sums(np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1]), tw, Fq + 2 * tones, sym - sr.STEP * sr.RANGE,
                                          sr.SYM_SEGS + 2 * sr.RANGE))


def tied_maximum(v):
    """(index of the first maximum, how many values equal it)"""
    v = np.asarray(v, F32)
    assert not np.isnan(v).any()
    return int(np.argmax(v)), int((v == v.max()).sum())


def test_tie_cases_are_what_they_are_named_for(edges, oracle):
    (iq, msgs, refined, first, n, where), want = edges
    tw = sr.twiddles(oracle)
    at = where["refine_tie"]
    pt_all = pt_all_of(iq[at[0]], msgs[at], tw)
    assert bits(pt_all[20:]).tolist() == [bits(pt_all[20:21])[0]] * 13 and (pt_all[:20] == 0).all() and pt_all[20] > 0   # thirteen equal maxima from e = 4 on
    assert want["refined"][at]["e_best"] == 4 and want["refined"][at]["pt"].tolist() == [0.0, pt_all[20], pt_all[20]]
    at = where["time_tie"]
    s = want["info"][at]
    assert tied_maximum(s["pt"]) == (1, 4) and s["pt"][0] == 0 and s["pt"][1] > 0 and s["t_best"] == -1
    assert s["pt"][2] == s["pt"][1] and bits(s["pt"][2:3])[0] == bits(s["pf"][2:3])[0]       # pt[2], taken from the frequency search, is one of the tied
    assert tied_maximum(s["pf"]) == (2, 2) and s["d_best"] == 0 and s["k4"] == 496 and (s["k4"] + 8 * 2) % 512 == 0
    for name, first_at, count in (("freq_tie", 1, 2), ("freq_tie_late", 3, 2)):
        s = want["info"][where[name]]
        assert tied_maximum(s["pf"]) == (first_at, count) and s["pf"][first_at] > 0 and s["d_best"] == first_at - 2, name
    # the pair run meets ties too: the refine rule's own e_best on an impulse, then both fine searches
    assert tied_maximum(want["pair_info"][where["refine_tie"]]["pf"])[1] >= 2


def test_ustar_cases_take_the_first_largest(edges):
    (iq, msgs, refined, first, n, where), want = edges
    seen = set()
    for name, (pf, us) in ec.USTAR.items():
        at = where[name]
        s = want["info"][at]
        assert bits(refined[at]["pf"][1:4]).tolist() == bits(np.array(pf, F32)).tolist()
        assert s["valid"] == 1 and int(s["k4"]) - int(s["d_best"]) == 4 * (ec.F_SIG + us - 2), (name, s)
        assert not np.isnan(s["pf"]).any() and not np.isnan(s["pt"]).any()
        seen.add(us)
    assert seen == {1, 2, 3}
    nan_at = [int(np.argmax(np.isnan(np.array(pf, F32)))) for name, (pf, _us) in ec.USTAR.items() if np.isnan(np.array(pf, F32)).sum() == 1]
    assert sorted(set(nan_at)) == [0, 1, 2]                              # a NaN in each position in turn
    assert bits(refined[where["ustar_nan_1"]]["pf"][1:2])[0] == ec.NAN_BITS
    assert np.signbit(refined[where["ustar_minus_zero_first"]]["pf"][1]) and not np.signbit(refined[where["ustar_plus_zero_first"]]["pf"][1])


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------------

def test_mutants_of_the_scans_change_a_named_case(edges, oracle):
    """the rule's scans, restated here, reproduce every decision of the restatements from their own powers; a scan with >= for >,
    a scan that lets a NaN win, and a u* that takes the last largest each change at least one named case"""
    (iq, msgs, refined, first, n, where), want = edges
    tw = sr.twiddles(oracle)

    def scan(v, rule):
        at, best = 0, v[0]
        for i in range(1, len(v)):
            take = {"strict": v[i] > best, "ge": v[i] >= best, "nan_wins": not (v[i] <= best)}[rule]
            if take:
                at, best = i, v[i]
        return at

    def ustar(pf, rule):
        us = 1
        for u in (2, 3):
            if {"strict": pf[u] > pf[us], "last_largest": pf[u] >= pf[us]}[rule]:
                us = u
        return us

    def decided(rule, u_rule="strict"):
        out = {}
        for name, at in where.items():
            s, R = want["info"][at], refined[at]
            with np.errstate(all="ignore"):
                out[name] = (scan(pt_all_of(iq[at[0]], msgs[at], tw), rule) - 16, scan(s["pf"], rule) - 2, scan(s["pt"], rule) - 2, ustar(R["pf"], u_rule))
        return out

    rule = decided("strict")
    for name, at in where.items():
        s = want["info"][at]
        Fq = 2 * int(msgs[at]["cand"]["freq_offset"]) + int(msgs[at]["cand"]["freq_sub"])
        assert rule[name] == (want["refined"][at]["e_best"], s["d_best"], s["t_best"], (int(s["k4"]) - int(s["d_best"])) // 4 - Fq + 2), name
    changed = lambda other: sorted(k for k in rule if other[k] != rule[k])
    ge, nan_wins, last = changed(decided("ge")), changed(decided("nan_wins")), changed(decided("strict", "last_largest"))
    print("changed by >=:", ge, "\nchanged by a NaN that wins:", nan_wins, "\nchanged by the last largest u*:", last)
    assert {"refine_tie", "time_tie", "freq_tie", "freq_tie_late", "scaled_zero_powers", "scaled_inf_powers"} <= set(ge)
    assert {"nan_behind_window_edge_inside", "inf_pair"} <= set(nan_wins) and "clean" not in nan_wins and "clean" not in ge
    assert {"ustar_equal_12", "ustar_equal_13", "ustar_all_equal", "ustar_inf_12", "ustar_plus_zero_first"} <= set(last)
    assert all(k.startswith("ustar_") for k in last)
    # the NaN mutant of u*: a NaN behind the largest would be taken
    assert ustar(refined[where["ustar_nan_3"]]["pf"], "strict") == 2
    assert scan(list(refined[where["ustar_nan_3"]]["pf"][1:4]), "nan_wins") + 1 == 3


# ---- late firsts and the pieces' layout -----------------------------------------------------------------------------------------------------------

def test_late_firsts_are_what_they_are_named_for(ft8):
    late = ec.late_firsts(ft8)
    iq, msgs, refined, first, n, names = late
    out, info = ec.late_expected(late)
    raw = info.view(np.uint8).reshape(len(n), 50, 64)
    assert [(int(a), int(b)) for a, b in zip(first, n)] == [(4, 8), (5, 11), (8, 9), (49, 50), (48, 50), (50, 50), (12, 12)]
    for f, name in enumerate(names):
        lo, hi = int(first[f]), int(n[f])
        written = [i for i in range(50) if (raw[f, i] != ec.FILL).any()]
        assert written == list(range(lo, hi)), name                      # records outside [first, n_msgs) keep the caller's 0xA5
        if hi > lo:
            assert (bits(out[f]) != bits(iq[f])).sum() > 80000, name
        else:
            assert out[f].tobytes() == iq[f].tobytes(), name
    assert all(f >= 4 for f in first)                                    # the estimate kernel's first workgroup is skipped whole in every case
    k = names.index("late_48_50_invalid_48")
    assert info[k, 48].tobytes() == bytes(64) and info[k, 49]["valid"] == 1 and refined[k, 48]["valid"] == 0
    assert out[k].tobytes() == out[names.index("late_49_50")].tobytes()  # the skipped record subtracts nothing
    assert len({msgs[0, i].tobytes() + refined[0, i].tobytes() for i in range(50)}) == 7
    # a workgroup skipped in part: records 5 .. 7 of workgroup 4 .. 7, then 8 .. 10 of 8 .. 11
    assert (int(first[1]) % 4, int(n[1]) % 4) == (1, 3)


def test_pieces_put_work_on_both_sides_of_frame_256(ft8):
    iq, msgs, refined, first, n = ec.pieces_stage(ft8)
    assert ec.STAGE_AT == (0, 1, 128, 255, 256, 257, 258) and ec.PIECES_FRAMES == 259 and ec.PIECES_CONTEXT == 260
    clamp = lambda v: min(max(int(v), 0), 50)
    work = {p: clamp(n[k]) - clamp(first[k]) for k, p in enumerate(ec.STAGE_AT)}
    assert work[255] == 50 and work[256] == 6 and work[0] == 3 and work[258] == 3 and work[1] == 0 and work[257] < 0
    assert iq[3].tobytes() != iq[4].tobytes() and msgs[3].tobytes() != msgs[4].tobytes()          # frames 255 and 256 differ
    full = ec.placed(first, ec.STAGE_AT)
    assert full.shape == (259,) and full[255] == -3 and full[256] == 5 and full[2] == 0
    m = ec.placed(msgs, ec.STAGE_AT, fill=ec.FILL)
    assert m.shape == (259, 50) and m[128].tobytes() == msgs[2].tobytes() and (m[127].view(np.uint8) == ec.FILL).all()


# ---- the comparison itself ---------------------------------------------------------------------------------------------------------------------

def test_the_comparison_accepts_a_nan_for_a_nan_and_nothing_else():
    want = np.zeros(3, ss.INFO_DTYPE)
    want["pf"][1] = (1.0, np.nan, np.inf, -0.0, 5.0)
    got = want.copy()
    assert ec.compare(got, want) == (1, None)
    got["pf"][1, 1] = np.array([0x7FC00000], np.uint32).view(F32)[0]     # another sign and payload
    assert ec.compare(got, want) == (1, None)
    for field, at, value in (("pf", (1, 3), 0.0), ("pf", (1, 1), 1.0), ("pf", (1, 0), np.nan), ("pf", (1, 2), np.nan), ("k4", 2, 1), ("pad", (0, 11), 1),
                             ("d_best", 1, -1), ("valid", 0, 1)):
        bad = got.copy()
        bad[field][at] = value
        assert ec.compare(bad, want)[1] is not None, (field, at, value)  # -0 for +0, a number for a NaN, a NaN for a number, any integer
    x = np.array([[1.0, np.nan], [np.nan, 2.0]], F32)
    y = x.copy()
    assert ec.compare(y, x) == (2, None)
    y[1, 1] = np.nextafter(F32(2.0), F32(3.0))
    assert ec.compare(y, x)[1] is not None
