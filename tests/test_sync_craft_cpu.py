"""The constructed waterfalls of tests/sync_craft.py are what they are named for (no GPU): the oracle's score map and candidate
lists equal the numpy restatements on every family; every property the families claim -- the peak equals the amplitude, the
off-site scores stay below the threshold used, the extremes +-255 / +-19125 are reached, every residue of every navg class
occurs beyond |num| 8192, what the heap has to do at each order -- is counted with the oracle and the restatements alone; the
two integer arguments sync.hip rests on (the float quotient, the threshold on the numerator in a saturating int16) are checked
by exhaustion over the attainable range; and three mutants of the restated rule show that the families tell a wrong rule
from the right one."""
import numpy as np
import pytest

import ft8_spec_decode as spec
import sync_craft as sc

PREVIOUS_CONFIGS = ((120, 10), (128, 10), (7, 10), (1, 10), (33, 0), (120, -5), (64, 30))     # test_heap_forms_are_exact


def score_maps(name):
    return [sc.scores_of(n) for n in sc.family_numerators(name)]


def reached(name):
    nums = sc.family_numerators(name)
    s = score_maps(name)
    return (min(int(n.min()) for n in nums), max(int(n.max()) for n in nums), min(int(x.min()) for x in s), max(int(x.max()) for x in s))


@pytest.fixture(scope="module")
def previous():
    """numerators of the random-byte frames the sync tests used before"""
    return [sc.numerators(m) for m in sc.random_byte_frames(70)]


def test_navg_classes_and_the_numerator_bound():
    assert sc.NAVG_SET == (50, 52, 56, 60, 63, 67, 71, 75) and sc.MAX_NUM == 19125
    assert sorted(sc.seam_scores()) == [436, 437, 655, 656]               # derived from the classes, stated here once
    for n in sc.NAVG_SET:                                                 # a cell of the collapsed maps sums at most 3 x 4 terms
        assert n <= 3 * (7 * 4 - 3)


@pytest.mark.parametrize("name", sc.FAMILIES)
def test_oracle_equals_the_restatements(oracle, name):
    fam = sc.family(name)
    for k, mag in enumerate(fam["mags"]):
        mine = score_maps(name)[k]
        assert np.array_equal(mine, spec.score_map(mag)), (name, k)
        assert np.array_equal(oracle.score_map(mag), mine.astype(np.int16)), (name, k)
        for cap, ms in fam["configs"]:
            want = sc.select(sc.family_numerators(name)[k], cap, ms)
            assert sc.as_list(oracle.find_sync(mag, cap, ms)) == want, (name, k, cap, ms)
            if name in ("full_scale", "heap_orders") or (cap, ms) in ((120, 100), (1024, 0), (120, -1)):
                assert [tuple(c) for c in spec.find_sync(mag, cap, ms, scores=mine)] == want, (name, k, cap, ms)


def test_full_scale_reaches_both_ends_at_every_class():
    fam = sc.family("full_scale")
    nums = sc.family_numerators("full_scale")
    seen = set()
    for k, sites in enumerate(fam["sites"]):
        s = sc.scores_of(nums[k])
        for ts, fs, t0, f0, a in sites:
            assert abs(a) == 255 and s[ts, fs, t0 - sc.T0_MIN, f0] == a
            assert nums[k][ts, fs, t0 - sc.T0_MIN, f0] == a * sc.navg_of(t0)
            seen.add((ts, fs, t0, a))
    assert {(t0, a) for _, _, t0, a in seen} == {(t0, a) for t0 in range(-12, 24) for a in (-255, 255)}      # every t0 in both signs
    assert {(ts, fs, t0 < 6, a) for ts, fs, t0, a in seen} == {(ts, fs, h, a) for ts, fs in sc.SLICES for h in (False, True) for a in (-255, 255)}
    f0s = {f0 for sites in fam["sites"] for _, _, _, f0, _ in sites}
    assert {0, 248} <= f0s and {f % 4 for f in f0s} == {0, 1, 2, 3} and {f // 4 for f in f0s} == set(range(63))   # lanes 0..62
    flat = np.concatenate([n.reshape(4, 36, 249) for n in nums], axis=2)
    for n in sc.NAVG_SET:
        at = flat[:, sc.NAVG == n, :]
        assert at.max() == 255 * n and at.min() == -255 * n
    assert reached("full_scale") == (-19125, 19125, -255, 255)
    assert (flat[:, sc.NAVG == 50, :] == 12750).any() and (flat[:, sc.NAVG == 50, :] == -12750).any()


def test_quotients_hold_every_residue_beyond_8192():
    fam = sc.family("quotients")
    nums = sc.family_numerators("quotients")
    want = {(n, s, r) for n in sc.NAVG_SET for s in (-1, 1) for r in (-1, 0, 1)}
    assert sc.quotient_coverage(nums) == want
    for k, sites in enumerate(fam["sites"]):
        at = nums[k][sc.site_index(sites)]
        assert (np.abs(at) > 8192).all()
    # truncation and floor part ways on them: negative numerators beyond 8192 that are no multiple of navg
    far = sum(int(((n < -8192) & (n % sc.NAVG[None, None, :, None] != 0)).sum()) for n in nums)
    assert far > 1000
    lo, hi, slo, shi = reached("quotients")
    assert lo < -18000 and hi > 18000 and slo <= -250 and shi >= 250


def test_lattice_scores_are_the_amplitudes_and_nothing_else_reaches_the_threshold():
    idx = sc.site_index(sc.lattice_sites())
    worst = -999
    for name in ("thresholds", "heap_orders"):
        for k, amps in enumerate(sc.family(name)["amps"]):
            s = score_maps(name)[k].copy()
            assert np.array_equal(s[idx], amps), (name, k)
            s[idx] = -999
            worst = max(worst, int(s.max()))
            want = [(int(a),) + (t0, f0, ts, fs) for (ts, fs, t0, f0), a in zip(sc.lattice_sites(), amps) if a >= sc.HEAP_MIN_SCORE]
            got = sc.select(sc.family_numerators(name)[k], 1024, sc.HEAP_MIN_SCORE)
            assert sorted(got) == sorted(want), (name, k)
    assert worst < sc.HEAP_MIN_SCORE, worst
    assert worst <= 70                                                     # 67 here; the survivors at 100 are exactly the dictated sites


def test_thresholds_frame_meets_every_branch_of_the_threshold():
    num = sc.family_numerators("thresholds")[0]
    s = sc.scores_of(num)
    amps = sc.family("thresholds")["amps"][0]
    assert set(amps.tolist()) == set(range(1, 256))
    navg = np.broadcast_to(sc.NAVG[None, None, :, None], num.shape)
    # min_score 0 and -1: numerators -1 .. -(navg - 1) truncate to 0 and stay; a threshold of min_score * navg drops them
    assert ((num < 0) & (num > -navg)).sum() > 100
    assert ((num <= -navg) & (num > -2 * navg)).sum() > 100
    scores = sc.threshold_scores()
    assert {0, 1, -1, 100, 255, 256, -255, -256, 436, 437, 655, 656, -436, -437, -655, -656} <= set(scores)
    for ms in scores:
        st = {}
        got = sc.select(num, 1024, ms, stats=st)
        assert st["survivors"] == (s >= ms).sum() and len(got) == min(1024, st["survivors"])
        if ms > 255 or ms <= s.min():
            assert st["survivors"] == (0 if ms > 255 else s.size)         # never / always
    assert (s >= 255).sum() == (amps == 255).sum() == 3 and (s >= 256).sum() == 0
    # the seam: the packed threshold is saturated at some time offsets of the frame and not at others
    for ms in (437, 655, -436, -654):
        sat = {abs(sc.packed_threshold(ms, n)) >= 32767 for n in sc.NAVG_SET}
        assert sat == {True, False}, ms
    for ms, all_sat in ((436, False), (656, True), (-435, False), (-655, True)):
        assert all(abs(sc.packed_threshold(ms, n)) >= 32767 for n in sc.NAVG_SET) == all_sat
        assert any(abs(sc.packed_threshold(ms, n)) >= 32767 for n in sc.NAVG_SET) == all_sat


def test_threshold_on_the_numerator_by_exhaustion():
    """num >= T, T in a saturating int16, decides trunc(num / navg) >= min_score for every attainable numerator, every class and
    every threshold of the family plus all of -300 .. 300 and the ends of the parameter's range; and num - T, saturated to int16,
    has the sign of the exact difference"""
    num = np.arange(-sc.MAX_NUM, sc.MAX_NUM + 1)
    for n in sc.NAVG_SET:
        q = sc.trunc_div(num, n)
        for ms in sorted(set(sc.threshold_scores()) | set(range(-300, 301)) | {-32768, 32767, 2 ** 31 - 1, -2 ** 31}):
            T = sc.packed_threshold(ms, n)
            sat = np.clip(num - T, -32768, 32767)
            assert np.array_equal(sat >= 0, q >= ms), (n, ms)


def test_quotient_rule_by_exhaustion():
    """(int)(float(num) * fl(1 / navg) + copysign(0.004f, num)) is C's num / navg on -19125 .. 19125 for every class: float32,
    one rounding per operation (the build has -ffp-contract=off)"""
    F = np.float32
    num = np.arange(-sc.MAX_NUM, sc.MAX_NUM + 1)
    checked = 0
    for n in sc.NAVG_SET:
        r = F(1.0) / F(n)
        f = num.astype(F)
        prod = (f * r).astype(F)
        got = np.trunc((prod + np.copysign(F(0.004), f)).astype(F)).astype(np.int64)
        bad = np.flatnonzero(got != sc.trunc_div(num, n))
        assert bad.size == 0, (n, num[bad[:5]])
        checked += num.size
    assert checked == 8 * 38251


def test_heap_orders_make_the_heap_do_what_they_are_named_for():
    fam = sc.family("heap_orders")
    nums = sc.family_numerators("heap_orders")
    by = dict(zip(fam["names"], range(len(fam["names"]))))
    st = {}

    def run(name, cap):
        sc.select(nums[by[name]], cap, sc.HEAP_MIN_SCORE, stats=st)
        return st["survivors"], st["replaced"], st["tied"]

    for cap in sc.HEAP_CAPS:
        n, rep, tied = run("ascending", cap)
        assert n == 156 and rep == max(0, n - cap) and tied == 0          # every survivor after the first `cap` replaces the minimum
        n, rep, tied = run("descending", cap)
        assert n == 156 and rep == 0 and tied == 0
        n, rep, tied = run("equal", cap)
        assert n == 512 and rep == 0 and tied == max(0, n - cap)          # all tied at the heap minimum
        n, rep, tied = run("falling_plateaus", cap)
        # the survivors behind the first `cap` that lie on the plateau [16 k - 8, 16 k + 8) of survivor cap - 1 tie with the minimum
        assert n == 512 and rep == 0 and tied == {1: 7, 7: 1, 64: 8, 120: 0, 128: 8, 480: 8, 1024: 0}[cap]
        n, rep, tied = run("rising_plateaus", cap)
        if cap == 1:
            assert (n, rep, tied) == (512, 32, 511 - 32)                   # one replacement per step up, a tie otherwise
        elif cap == 7:
            assert n == 512 and rep > 0 and tied > 0                       # a plateau is longer than the heap
        else:
            assert (n, rep, tied) == (512, max(0, n - cap), 0)             # the minimum lies a plateau or more back
        for name in ("sawtooth", "shuffled"):
            n, rep, tied = run(name, cap)
            assert n == 512 and (cap >= n or rep > 0) and (cap > 128 or tied > 0), (name, cap)
    amps = fam["amps"][by["falling_plateaus"]]
    for k in range(64, 512, 64):                                           # the runs of ties straddle every multiple of 64 survivors
        assert amps[k - 8] == amps[k - 1] == amps[k] == amps[k + 7] != amps[k + 8]


def test_mutants_are_told_apart(previous):
    """the three wrong rules give another candidate list than the specification on the family made for them.  The random-byte
    frames used before tell them apart only where min_score <= 0 or through ties -- at the product's positive thresholds the
    two arithmetic mutants are invisible to them, and no numerator of theirs lies beyond 8192, so a rule that is wrong only
    out there passes on all 70"""
    for name, mutant in (("thresholds", "threshold"), ("quotients", "floor"), ("heap_orders", "replace_ge")):
        fam = sc.family(name)
        told = [(k, cap, ms) for k, num in enumerate(sc.family_numerators(name)) for cap, ms in fam["configs"]
                if sc.select(num, cap, ms, mutant) != sc.select(num, cap, ms)]
        assert told, (name, mutant)
        if mutant == "threshold":
            assert sorted(set(ms for _, _, ms in told)) == [-1, 0]
        if mutant == "replace_ge":
            assert {fam["names"][k] for k, _, _ in told} >= {"equal", "falling_plateaus", "rising_plateaus", "sawtooth"}
            assert not any(fam["names"][k] in ("ascending", "descending") for k, _, _ in told)      # no ties: nothing to tell
    assert max(int(np.abs(n).max()) for n in previous) < 8192
    told = {m: set() for m in ("threshold", "floor", "replace_ge")}
    for num in previous[:4]:
        for cap, ms in PREVIOUS_CONFIGS:
            want = sc.select(num, cap, ms)
            for m in told:
                if sc.select(num, cap, ms, m) != want:
                    told[m].add((cap, ms))
    assert told["threshold"] and told["floor"] and told["replace_ge"]     # all three, but ...
    assert all(ms <= 0 for _, ms in told["threshold"] | told["floor"])    # ... the arithmetic ones only at thresholds <= 0


def test_ranges_reached(previous):
    """what DESIGN.md "Sync search" and the tests' docstrings state: (min numerator, max numerator, min score, max score)"""
    prev = (min(int(n.min()) for n in previous), max(int(n.max()) for n in previous),
            min(int(sc.scores_of(n).min()) for n in previous), max(int(sc.scores_of(n).max()) for n in previous))
    assert prev == (-6297, 6695, -105, 101)
    assert reached("full_scale") == (-19125, 19125, -255, 255)
    assert reached("quotients") == (-18856, 18868, -251, 252)
    assert reached("thresholds") == (-6120, 19125, -85, 255)
    assert reached("heap_orders") == (-6120, 19125, -85, 255)
