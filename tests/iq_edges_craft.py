"""Constructed frames and records for the float edges, the ties, the late firsts and the 256-frame pieces of the refine and
subtraction stages (tests only; tests/test_iq_edges_cpu.py proves with the restatements that every named case is what it is named
for, tests/test_gpu_refine.py and tests/test_gpu_subtract.py hold the device to the restatements on them).  Everything is built
on the signal frame and the signal's own record of tests/subtract_craft.constructed (T_sig = 9, F_sig = 321, STRONG_TEXT; the
signal starts at sample 2576, the record's e = 0 at 2560):

  scaled       the base frame with every sample times a power of two: subnormal powers, powers that underflow to +0 under
               amplitudes that do not, subnormal samples, infinite powers under finite amplitudes; and exponents at which nothing
               under- or overflows, where scaling must commute with both rules bit for bit
  non-finite   +inf, -inf beside +inf and a NaN with a sign and a payload inside the record; a NaN that no window reads; a NaN
               one sample either side of the first sample the refine search reads, and of the last
  ties         single impulses in frames of zeros, placed so that the first-strict-maximum scans of e_best, d* and t* see equal
               non-zero maxima whose first member is not index 0 (the placements were searched on the CPU, see beside them)
  ustar        the base frame with records whose R.pf[1 .. 3] hold equal pairs, three equal values, a NaN in each position, +inf,
               -inf and zeros of both signs (several records on one frame: the only such frame of edges())
  late firsts  the base frame under 50 records drawn from a handful, with first / n_msgs that skip whole workgroups of the
               estimate kernel and parts of one
  pieces       259 frames for a context of 260: all zeros but a few placed frames on both sides of frame 256

SCALED_EXP and EXACT_EXP were chosen from what the restatements return on the CPU (the walk is described beside them)."""
import numpy as np

import ft8_spec_refine as sr
import ft8_spec_subtract as ss
import subtract_craft as sc

NSAMPLES = sc.NSAMPLES
FILL = sc.FILL
F32 = np.float32
TINY = np.finfo(np.float32).tiny
T_SIG, F_SIG = 9, 2 * 160 + 1
S_REC = 256 * T_SIG + sr.LEAD                 # the record's first sample at e = 0; the signal itself starts 16 samples later
WINDOW = (S_REC - 512, S_REC + ss.SPAN + 512)  # the union of the refine search's windows: e = -16 .. 16
NAN_BITS = 0xFFC00001                        # a quiet NaN with its sign set and a payload
PF = {1: (1.0, 9.0, 5.0, 2.0, 1.0), 2: (1.0, 5.0, 9.0, 5.0, 1.0), 3: (1.0, 2.0, 5.0, 9.0, 1.0)}

# ---- every sample times a power of two ------------------------------------------------------------------------------------------
# The base frame's largest sample is 0.5 and its powers are 2e5 .. 5e5.  k was walked over -150 .. 126 with both restatements
# (ldexp: exact wherever the product is a normal float).  Downwards: at -70 every power but the refine rule's noise is still
# normal, at -72 the first are subnormal, from -73 to -77 all are and every decision is still the unscaled frame's; at -80 so few
# bits are left that new ties appear (t* moves from 2 to 0, three of the refine rule's pf are +0); from -85 on every power is +0
# while the amplitudes stay non-zero down to -145 (-90: all 2528 components); from -130 every non-zero sample is subnormal (-140:
# 95 503 of 96 000 are still non-zero).  Upwards: through 40 nothing overflows, at 55 the powers from the first large one on are
# +inf, from 58 to 100 every fine-search power is +inf with every amplitude and the residual finite (62: the largest sample is
# 2^61), at 126 the segment sums overflow and the powers are NaN.
SCALED_EXP = {"scaled_subnormal_powers": -75, "scaled_few_bits_left": -80, "scaled_zero_powers": -90, "scaled_subnormal_samples": -140,
              "scaled_partly_inf_powers": 55, "scaled_inf_powers": 62}
EXACT_EXP = {"scaled_exact_down": -40, "scaled_exact_up": 40}           # nothing under- or overflows: scaling commutes, bit for bit

# ---- ties -----------------------------------------------------------------------------------------------------------------------
# One impulse in a frame of zeros: every sum of either rule then has one non-zero term, so a power is |x w|^2 of one table entry.
#   refine_tie  the impulse lies 100 samples behind the record's last symbol at e = 0: it is outside the span for e < 4 and inside
#               symbol 78 for e = 4 .. 16.  (k j) mod 1024 counts from the absolute j, so the thirteen powers are one product.
#   time_tie    K = k4* + 8 tone[78] = 496 + 16 is a multiple of 512, so theta at the impulse does not move with t; the impulse
#               lies 14 samples before the end of the span at t = 0: outside it for t = -2, inside for the later t.  The sample
#               (-0.3, 0.9) is the first of a list of hand-picked and then seeded values at which d = 0 is the first maximum of pf
#               (index 2, tied with index 4), so that k4* is the 496 the construction needs.
#   freq_tie    searched with x = (1, 0) over every position j of the record at F = 321: the powers are 1 to an ulp either way,
#               and 7975 of the 40 448 positions give a maximum that is shared and does not start at index 0.  The two below are
#               the first with the maximum first at index 1 (pf = lo, hi, hi, 1, 1) and the first with it first at index 3.
TIES = {"refine_tie": (S_REC + ss.SPAN + 100, (0.25, 0.0), T_SIG, F_SIG, 4),            # name: (j, (I, Q), T, F, R.e_best)
        "time_tie": (S_REC + ss.SPAN - 14, (-0.3, 0.9), T_SIG, 124, 0),
        "freq_tie": (2608, (1.0, 0.0), T_SIG, F_SIG, 0),
        "freq_tie_late": (2568, (1.0, 0.0), T_SIG, F_SIG, 0)}

# ---- u* -------------------------------------------------------------------------------------------------------------------------
NAN = np.array([NAN_BITS], np.uint32).view(F32)[0]
INF = F32(np.inf)
USTAR = {  # name: (R.pf[1 .. 3], the u* of the rule)
    "ustar_equal_12": ((9.0, 9.0, 5.0), 1), "ustar_equal_23": ((5.0, 9.0, 9.0), 2), "ustar_equal_13": ((9.0, 5.0, 9.0), 1),
    "ustar_all_equal": ((9.0, 9.0, 9.0), 1), "ustar_nan_1": ((NAN, 5.0, 9.0), 1), "ustar_nan_2": ((5.0, NAN, 9.0), 3),
    "ustar_nan_3": ((5.0, 9.0, NAN), 2), "ustar_nan_2_behind_the_largest": ((9.0, NAN, 5.0), 1), "ustar_all_nan": ((NAN, NAN, NAN), 1),
    "ustar_inf_23": ((1.0, INF, INF), 2), "ustar_inf_12": ((INF, INF, 1.0), 1), "ustar_inf_3": ((1.0, 2.0, INF), 3),
    "ustar_all_minus_inf": ((-INF, -INF, -INF), 1), "ustar_minus_zero_first": ((-0.0, 0.0, 0.0), 1),
    "ustar_plus_zero_first": ((0.0, -0.0, -0.0), 1), "ustar_negative": ((-3.0, -2.0, -1.0), 3)}

# the only cases in which a restatement writes a NaN that is not a copy of an input sample (the NaNs of USTAR are inputs and reach
# no output; the NaN of nan_behind_window_edge_inside makes P(0, 16) a NaN, which the scan passes over and no record holds)
NAN_OUTPUT_CASES = ("inf_sample", "inf_pair", "nan_sample", "nan_at_window_edge_inside")


def base(ft8):
    """(the signal frame [2][48000], its own message record, its hand-made R) of subtract_craft.constructed"""
    iq, msgs, refined, _first, _n, where = sc.constructed(ft8)
    f, i = where["f3_truth"]
    return iq[f].copy(), msgs[f, i].copy(), refined[f, i].copy()


def record(m0, R0, T, F, e_best=0, us=2, pf123=None, valid=1):
    """a copy of (m0, R0) moved to cell (T, F), with R.e_best, R.valid and R.pf set by hand"""
    m, R = m0.copy(), R0.copy()
    c = m["cand"]
    c["score"], c["time_offset"], c["time_sub"], c["freq_offset"], c["freq_sub"] = 20, T >> 1, T & 1, F >> 1, F & 1
    R["e_best"], R["valid"], R["pf"] = e_best, valid, PF[us]
    if pf123 is not None:
        R["pf"][1:4] = np.array(pf123, F32)
    return m, R


def scaled(x, k):
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(x, k).astype(F32)


def impulse_frame(j, value):
    x = np.zeros((2, NSAMPLES), F32)
    x[0, j], x[1, j] = value
    return x


def edges(ft8):
    """the scaled, non-finite, tie and u* cases as one batch: iq [B][2][48000], msgs [B][50], refined [B][50] (hand-made R),
    first [B] (zeros), n_msgs [B], where {name: (frame, slot)}.  Every frame holds one record but the frame of the u* cases."""
    x0, m0, R0 = base(ft8)
    own = record(m0, R0, T_SIG, F_SIG)
    frames, lists, where = [], [], {}

    def frame(x, recs):
        f = len(frames)
        frames.append(np.asarray(x, F32))
        lists.append([r for _n, r in recs])
        for i, (name, _r) in enumerate(recs):
            assert name not in where
            where[name] = (f, i)

    frame(x0, [("clean", own)])
    for name, k in list(SCALED_EXP.items()) + list(EXACT_EXP.items()):
        frame(scaled(x0, k), [(name, own)])

    def with_samples(name, *puts):
        x = x0.copy()
        for comp, j, v in puts:
            x[comp, j] = v
        frame(x, [(name, own)])

    j = S_REC + 512 * 40 + 200                                          # inside data symbol 40
    with_samples("inf_sample", (0, j, np.inf))
    with_samples("inf_pair", (0, j, -np.inf), (0, j + 1, np.inf))
    with_samples("nan_sample", (1, S_REC + 512 * 3 + 200, NAN))         # inside the first Costas array
    with_samples("nan_outside", (0, 47000, NAN))                        # behind everything either kernel stages
    with_samples("nan_at_window_edge_outside", (0, WINDOW[0] - 1, NAN))
    with_samples("nan_at_window_edge_inside", (0, WINDOW[0], NAN))      # P(0, -16) of the refine rule, the scan's first value
    # the amplitude pass stages whole chunks of 1024 samples, 16 + 496 samples past the record's end: read and not used
    with_samples("nan_behind_window_edge_outside", (1, WINDOW[1], NAN))
    with_samples("nan_behind_window_edge_inside", (1, WINDOW[1] - 1, NAN))   # P(0, 16) only: a NaN the scan must pass over

    for name, (j, value, T, F, e_best) in TIES.items():
        frame(impulse_frame(j, value), [(name, record(m0, R0, T, F, e_best=e_best))])

    frame(x0, [(name, record(m0, R0, T_SIG, F_SIG, pf123=pf)) for name, (pf, _us) in USTAR.items()])

    B = len(frames)
    iq = np.stack(frames)
    msgs = np.full((B, 50 * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(B, 50)
    refined = np.full((B, 50 * 48), FILL, np.uint8).view(sr.REFINED_DTYPE).reshape(B, 50)
    for f, l in enumerate(lists):
        for i, (m, R) in enumerate(l):
            msgs[f, i], refined[f, i] = m, R
    return iq, msgs, refined, np.zeros(B, np.int32), np.array([len(l) for l in lists], np.int32), where


def filled(dtype, B):
    """[B][50] records of `dtype`, every byte FILL"""
    return np.full((B, 50 * dtype.itemsize), FILL, np.uint8).view(dtype).reshape(B, 50)


def edges_expected(oracle, batch):
    """the restatements on edges(): refined (the refine rule, FILL behind the counts), out / info (the subtraction with the
    hand-made R), pair_out / pair_info (the subtraction with the refine rule's own records, as the pass loop pairs them)"""
    iq, msgs, refined, first, n, _where = batch
    tw, w4 = sr.twiddles(oracle), ss.twiddles()
    B = len(n)
    with np.errstate(all="ignore"):
        ref = sr.refine(iq, msgs, n, tw, refined=filled(sr.REFINED_DTYPE, B))
        out, info = ss.subtract(iq, msgs, refined, first, n, w4, info=filled(ss.INFO_DTYPE, B))
        pair_out, pair_info = ss.subtract(iq, msgs, ref, first, n, w4, info=filled(ss.INFO_DTYPE, B))
    return {"refined": ref, "out": out, "info": info, "pair_out": pair_out, "pair_info": pair_info}


def late_expected(late):
    iq, msgs, refined, first, n, _names = late
    return ss.subtract(iq, msgs, refined, first, n, ss.twiddles(), info=filled(ss.INFO_DTYPE, len(n)))


# ---- late firsts ----------------------------------------------------------------------------------------------------------------
# (first, n_msgs, the record whose R.valid is cleared or None).  The estimate kernel works a frame off in workgroups of four
# records: (4, 8) skips one whole and fills the next, (5, 11) skips a wave at the front of one and leaves the last ragged, ...
LATE = ((4, 8, None), (5, 11, None), (8, 9, None), (49, 50, None), (48, 50, 48), (50, 50, None), (12, 12, None))


def late_name(first, n, invalid):
    return f"late_{first}_{n}" + ("" if invalid is None else f"_invalid_{invalid}")


def late_records(ft8):
    """(the base frame, msgs [50], refined [50]): 50 records drawn in turn from seven distinct ones"""
    x0, m0, R0 = base(ft8)
    other = m0.copy()
    other["a91"] = np.random.default_rng(0x1A7E).integers(0, 256, 12, dtype=np.uint8)       # another message in the signal's cell
    distinct = [record(m0, R0, T_SIG, F_SIG), record(other, R0, T_SIG, F_SIG), record(m0, R0, T_SIG, F_SIG + 3, e_best=1),
                record(m0, R0, T_SIG, F_SIG, us=3), record(m0, R0, T_SIG, F_SIG + 1, e_best=1, us=1),
                record(m0, R0, -24, 0, e_best=-16), record(m0, R0, 2 * 300, 40)]
    msgs = np.zeros(50, ft8.MESSAGE_DTYPE)
    refined = np.zeros(50, sr.REFINED_DTYPE)
    for i in range(50):
        msgs[i], refined[i] = distinct[i % len(distinct)]
    return x0, msgs, refined


def late_firsts(ft8):
    """one copy of the frame per case of LATE: iq [7][2][48000], msgs [7][50], refined [7][50], first [7], n_msgs [7], names"""
    x0, m, R = late_records(ft8)
    B = len(LATE)
    iq = np.stack([x0] * B)
    msgs, refined = np.stack([m] * B), np.stack([R] * B)
    for f, (_first, _n, invalid) in enumerate(LATE):
        if invalid is not None:
            refined[f, invalid]["valid"] = 0
    return (iq, msgs, refined, np.array([c[0] for c in LATE], np.int32), np.array([c[1] for c in LATE], np.int32),
            [late_name(*c) for c in LATE])


# ---- pieces -----------------------------------------------------------------------------------------------------------------------
PIECES_FRAMES, PIECES_CONTEXT = 259, 260      # one chunk on a context of 260 frames: pieces of 256 and 3
STAGE_AT = (0, 1, 128, 255, 256, 257, 258)   # where the seven frames of pieces_stage go
# which frame goes where: frames 3, 1, 2 and 0 of subtract_craft.constructed, the late-firsts frame (5, 11), then frames 4 and 5.
# Frame 255, the last of the first piece, holds the 50 records of frame 0; frame 256, the first of the second, the late firsts.
STAGE_ORDER = (3, 1, 2, 0, "late", 4, 5)
WHOLE_AT = (0, 130, 255, 256, 258)           # where five radio frames go for the whole-path entries


def pieces_stage(ft8):
    """the seven distinct frames in the order of STAGE_AT: iq [7][2][48000], msgs [7][50], refined [7][50], first [7], n_msgs [7]"""
    iq, msgs, refined, first, n, _where = sc.constructed(ft8)
    l_iq, l_m, l_R, l_first, l_n, names = late_firsts(ft8)
    k = names.index("late_5_11")
    pick = lambda a, l: np.stack([l[k] if s == "late" else a[s] for s in STAGE_ORDER])
    return pick(iq, l_iq), pick(msgs, l_m), pick(refined, l_R), pick(first, l_first).astype(np.int32), pick(n, l_n).astype(np.int32)


def placed(distinct, at, total=PIECES_FRAMES, fill=0):
    """an array of `total` leading entries, every byte `fill`, with distinct[k] at index at[k]"""
    distinct = np.asarray(distinct)
    out = np.zeros((total,) + distinct.shape[1:], distinct.dtype)
    out.view(np.uint8)[...] = fill
    for k, p in enumerate(at):
        out[p] = distinct[k]
    return out


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def compare(got, want):
    """Byte for byte, except that where `want` holds a NaN in a float32 field `got` must hold a NaN of any sign and payload.
    got / want: float32 arrays, or record arrays whose float32 fields are compared this way and every other field exactly.
    Returns (how many values were compared as NaN against NaN, None or a description of the first difference)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.names is None:
        assert got.dtype == F32
        fields = [(None, got, want)]
    else:
        fields = [(name, np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])) for name in got.dtype.names]
    nans = 0
    for name, g, w in fields:
        if g.dtype.base == F32:
            wn = np.isnan(w)
            bad = np.where(wn, ~np.isnan(g), g.view(np.uint32) != w.view(np.uint32))
            nans += int(wn.sum())
        else:
            bad = g != w
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            return nans, f"{int(bad.sum())} values of {name or 'the samples'} differ, the first at {list(map(int, at))}: {g[at]!r} != {w[at]!r}"
    return nans, None


def hold(got, want, where):
    """got / want: the [B][50] records or the [B][2][48000] samples of edges().  The frames of NAN_OUTPUT_CASES go through
    compare(), every other frame is held byte for byte.  Returns {case: values compared as NaN against NaN}."""
    loose = {where[name][0]: name for name in NAN_OUTPUT_CASES}
    names = {}
    for name, (f, _i) in where.items():
        names.setdefault(f, name)
    counts = {}
    for f in range(len(want)):
        if f in loose:
            counts[loose[f]], diff = compare(got[f], want[f])
            assert diff is None, (loose[f], diff)
        else:
            assert got[f].tobytes() == want[f].tobytes(), (names[f], compare(got[f], want[f])[1])
    return counts
