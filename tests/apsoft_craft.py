"""Soft-bit rows made to order for AP on a soft-bit array (tests only): candidates of three rows each, built from the vectors of
tests/ap_craft.py (their normalised soft bits are ordinary rows), placed in frames with fabricated status records.  No I/Q is
involved: the array goes straight into ft8gpu_ap_soft_candidates.  tests/test_demod_ap_cpu.py proves with the restatement that
each candidate is what it is named for.

  set1 / set2 / set3   a CQ codeword BP misses and "CQ ? ?" recovers in row 1; behind one failing row; behind two
  zero_between         an all-zero row (unusable, code 6) between a failing row and the recoverable one
  unusable             a row with a NaN, one with +infinity, one with -infinity beside +infinity: result 6, set 0
  nan_then_good        an unusable row, then the recoverable one
  edge_* / scaled_*    the recoverable row with its smallest nonzero value put at 2^-57, 2^-59 and a subnormal (the division guard's
                       bound is 2^-58), as one replaced element and as the whole row scaled by a power of two; times 2^100
  dx                   "CQ DX K1JT FN20": accepted under hypothesis 3 of ap_craft's table of four
  no_cq / crc / unpack / all_negative   ap_craft's cases b, c, d, e: codes 7 (8 under b_one_wrong), 3, 4 (under d_all_77), 7
  copied_ok / copied_no_errors          records that do not qualify"""
import numpy as np

import ap_craft as ac
import ft8_spec_apsoft as sx

F32 = np.float32
CAP = 24
FILL = 0xA5
NAMES = ("set1", "set2", "set3", "zero_between", "unusable", "nan_then_good", "edge_m57", "edge_m59", "edge_sub", "scaled_m57",
         "scaled_m59", "scaled_sub", "scaled_p100", "dx", "no_cq", "no_cq_clean", "crc", "unpack", "all_negative", "copied_ok",
         "copied_no_errors", "a1_set1")


def _smallest(row):
    a = np.abs(row)
    return int(np.flatnonzero(a == a[a > 0].min())[0])


def _edge(row, value):
    """the row with its smallest nonzero element at +-value"""
    out = row.copy()
    k = _smallest(row)
    out[k] = np.copysign(F32(value), row[k])
    return out


def _scaled(row, exponent):
    """the row times the power of two that puts its smallest nonzero magnitude into [2^exponent, 2^(exponent + 1)), that element
    then set to 2^exponent exactly"""
    k = _smallest(row)
    _m, e = np.frexp(np.abs(row[k]))                               # |row[k]| = m 2^e, m in [0.5, 1)
    out = row.astype(np.float64) * 2.0 ** (exponent - (int(e) - 1))
    out[k] = np.copysign(2.0 ** exponent, row[k])
    out = out.astype(F32)
    assert np.abs(out[out != 0]).min() == F32(2.0 ** exponent)
    return out


def candidates(oracle):
    """{name: float32 [3][176]} in the order of NAMES"""
    by = {c["name"]: ac.llr_of(c["v"]).astype(F32) for c in ac.build_cases(oracle) if c["case"] != "f"}
    good, fail, clean = by["a_0"], by["b_noise"], by["b_clean"]
    zero = np.zeros(174, F32)
    nan, pinf, both = good.copy(), good.copy(), good.copy()
    nan[100] = np.nan
    pinf[3] = np.inf
    both[0], both[173] = -np.inf, np.inf
    rows = {
        "set1": (good, zero, zero), "set2": (fail, good, zero), "set3": (fail, clean, good), "zero_between": (fail, zero, by["a_1"]),
        "unusable": (nan, pinf, both), "nan_then_good": (nan, good, zero),
        "edge_m57": (_edge(good, 2.0 ** -57), zero, zero), "edge_m59": (_edge(good, 2.0 ** -59), zero, zero),
        "edge_sub": (_edge(good, 2.0 ** -140), zero, zero),
        "scaled_m57": (_scaled(good, -57), zero, zero), "scaled_m59": (_scaled(good, -59), zero, zero),
        "scaled_sub": (_scaled(good, -140), zero, zero), "scaled_p100": ((good.astype(np.float64) * 2.0 ** 100).astype(F32), zero, zero),
        "dx": (by["a_2"], zero, zero), "no_cq": (fail, by["b_flips"], zero), "no_cq_clean": (clean, zero, zero),
        "crc": (by["c_wrong_crc"], zero, zero), "unpack": (by["d_unpack_refuses"], zero, zero),
        "all_negative": (by["e_all_negative"], zero, zero), "copied_ok": (good, zero, zero), "copied_no_errors": (good, zero, zero),
        "a1_set1": (by["a_1"], zero, zero),
    }
    out = {}
    for name in NAMES:
        a = np.zeros((3, sx.STRIDE), F32)
        for n, r in enumerate(rows[name]):
            a[n, :174] = r
        out[name] = a
    return out


def build(ft8, oracle, cap=CAP, counts=None):
    """(soft [B][cap][3][176], counts [B], status [B][cap], where {name: (frame, index)}): frame 0 holds the named candidates
    in order (as many as fit), the other frames cycle through them from other starts; records behind a count are FILL bytes"""
    cands = candidates(oracle)
    order = [n for n in NAMES]
    counts = np.array((min(cap, len(order)), 0, 3, cap, min(cap, 17)) if counts is None else counts, np.int32)
    B = len(counts)
    soft = np.full((B, cap, 3 * sx.STRIDE * 4), FILL, np.uint8).view(F32).reshape(B, cap, 3, sx.STRIDE)
    status = np.full((B, cap * 48), FILL, np.uint8).view(ft8.STATUS_DTYPE).reshape(B, cap)
    where = {}
    for f in range(B):
        for i in range(int(counts[f])):
            name = order[(i + 5 * f) % len(order)]
            soft[f, i] = cands[name]
            rec = np.zeros(1, ft8.STATUS_DTYPE)[0]
            rec["ldpc_errors"], rec["iters"] = 3 + (i % 40), 20
            if name == "copied_ok":
                rec["ok"], rec["ldpc_errors"] = 1, 0
            if name == "copied_no_errors":
                rec["ldpc_errors"] = 0
            status[f, i] = rec
            where.setdefault(name, (f, i))
    for a in (soft, counts, status):
        a.setflags(write=False)
    return soft, counts, status, where
