"""Soft bits made to order for ordered-statistics decoding (tests only).  ft8gpu_osd_candidates takes the waterfall, the
candidates and status_in from the caller, so a test can hand the kernel any vector of 174 integers in -255..255 as raw soft
bits: write_candidate() inverts ft8_extract_likelihood (the arithmetic osd.hip restates) cell by cell.  On top of that the
constructed cases of DESIGN.md "Ordered-statistics decoding": vectors that reach what synthesised radio frames never do
(a pivot in the third 64-column slot, saturated weights, every result code, the seams of the pattern index, tied metrics),
the frames that carry them with fabricated status records, and the tallies that say what a run reached.

Everything is generated from fixed seeds; tests/test_osd_constructed_cpu.py proves each case has the property it is named
for, with the oracle and the restatement (tests/ft8_spec_osd.py) alone."""
import numpy as np

import ft8_spec_osd as so

GRAY = (0, 1, 3, 2, 5, 6, 4, 7)
MAG_ARRAY, NBLOCKS, NBIN, BLOCK_STRIDE = 94208, 92, 256, 1024
CAP = 45                                   # max_candidates of the constructed frames: no multiple of the four waves of a workgroup
PER_FRAME = 31                             # disjoint 8-bin ranges below bin 256
FILL = 0xA5
GATES = (83, 27, 20)
F_ERRORS = (1, 20, 27, 83)                 # case f: hard errors outside the basis; gates e (accepted) and e - 1 (refused)
CONFIGS = [(order, gate) for order in (0, 1, 2) for gate in sorted(set(GATES) | set(F_ERRORS) | set(e - 1 for e in F_ERRORS))]
G_SINGLES = (0, 63, 64, 90)
G_PAIRS = ((0, 1), (0, 64), (0, 90), (1, 2), (45, 46), (62, 63), (63, 64), (64, 65), (89, 90))
G_PATTERNS = (0, 1, 64, 65, 91, 92, 155, 181, 182, 3152, 3781, 3809, 3836, 4186)
CAND_DTYPE = np.dtype([("score", "<i2"), ("time_offset", "<i2"), ("freq_offset", "<i2"), ("time_sub", "u1"), ("freq_sub", "u1")])


def sym_of(k):
    return k + 7 if k < 29 else k + 14


def effective(v, time_offset):
    """the raw soft bits a candidate at time_offset reads: v, with 0 for the symbols whose block lies outside 0..91"""
    v = np.array(v, np.int16, copy=True)
    for k in range(58):
        if not 0 <= int(time_offset) + sym_of(k) < NBLOCKS:
            v[3 * k:3 * k + 3] = 0
    return v


def write_candidate(mag, v, cand):
    """the eight tone cells of the 58 data symbols of `cand` in mag uint8 [94208] such that ft8_extract_likelihood returns v:
    255 in the cell of the symbol's three signs, 255 - |v| in the three cells one sign away, 0 in the other four"""
    to, fo, ts, fs = int(cand["time_offset"]), int(cand["freq_offset"]), int(cand["time_sub"]), int(cand["freq_sub"])
    assert 0 <= fo <= NBIN - 8 and ts in (0, 1) and fs in (0, 1)
    v = np.asarray(v, np.int64)
    assert v.shape == (174,) and np.abs(v).max() <= 255
    for k in range(58):
        sym = sym_of(k)
        if not 0 <= to + sym < NBLOCKS:
            continue
        b = v[3 * k:3 * k + 3] > 0
        d = np.abs(v[3 * k:3 * k + 3])
        j = 4 * int(b[0]) + 2 * int(b[1]) + int(b[2])
        start = ((to * 2 + ts) * 2 + fs) * NBIN + fo + sym * BLOCK_STRIDE
        assert 0 <= start and start + 8 <= MAG_ARRAY and not mag[start:start + 8].any()       # no candidate shares a cell
        mag[start + GRAY[j]] = 255
        mag[start + GRAY[j ^ 4]] = 255 - d[0]
        mag[start + GRAY[j ^ 2]] = 255 - d[1]
        mag[start + GRAY[j ^ 1]] = 255 - d[2]


# ---- the cases -------------------------------------------------------------------------------------------------------------

def _codeword(rng):
    return ((rng.integers(0, 2, so.K) @ so.generator_matrix().astype(np.int64)) & 1).astype(np.uint8)


def _signed(cw, mags):
    return np.where(np.asarray(cw) == 1, mags, -np.asarray(mags)).astype(np.int16)


def _order_of(v):
    return so.sort_order(np.abs(np.asarray(v)).astype(np.float32))     # the normalisation keeps the order of distinct integers


def last_pivot(v):
    """(sorted position of the 91st pivot, the generator row that takes it, h at that position)"""
    order = _order_of(v)
    piv_row, piv_col, _ = so.eliminate(order)
    return piv_col[-1], piv_row[-1], int(v[order[piv_col[-1]]] > 0)


def saturated(llr):
    return int((so.hard_and_weights(llr)[1] == 255).sum())


def _payload_codeword(bits77):
    bits = np.concatenate([np.asarray(bits77, np.uint8), [(so.crc14(bits77) >> (13 - i)) & 1 for i in range(14)]]).astype(np.int64)
    return ((bits @ so.generator_matrix().astype(np.int64)) & 1).astype(np.uint8)


def _case_a(cases):
    """a low-weight codeword's support least reliable: the other columns have rank < 91, the last pivot lies in the support"""
    G = so.generator_matrix()
    low = [G[32] ^ G[47]] + [G[r] for r in range(so.K) if G[r].sum() <= 46]
    assert low[0].sum() == 22 and len(low) == 81
    rng = np.random.default_rng(0xA)
    found = {}
    for trial in range(400):
        lw = low[0] if trial == 0 else low[1 + int(rng.integers(0, 80))]
        mags = np.where(lw == 1, rng.integers(1, 4, 174), rng.integers(40, 200, 174))
        v = _signed(_codeword(rng), mags)
        pos, row, h = last_pivot(v)
        assert pos >= 128 and (trial > 0 or pos == 152)
        found.setdefault((row >= 64, h), (v, pos, row))
        if len(found) == 4:
            break
    assert len(found) == 4, sorted(found)
    for (high, h), (v, pos, row) in sorted(found.items()):
        cases.append(dict(case="a", name=f"a_row{'64_90' if high else '0_63'}_h{h}", v=v, last_pivot=pos, pivot_row=row, pivot_h=h))


def _case_b(cases):
    rng = np.random.default_rng(0xB)
    for nbig in (1, 2, 3, 4, 5):
        v = (rng.integers(0, 3, 174) * rng.choice([-1, 1], 174)).astype(np.int16)
        v[rng.choice(174, nbig, replace=False)] = 255 * rng.choice([-1, 1], nbig)
        cases.append(dict(case="b", name=f"b_{nbig}_of_255", v=v, saturated=nbig if nbig < 5 else 0))


def _case_cd(cases):
    cases.append(dict(case="c", name="c_all_zero", v=np.zeros(174, np.int16), result=6))
    cases.append(dict(case="c", name="c_all_minus_7", v=np.full(174, -7, np.int16), result=6))
    cases.append(dict(case="c", name="c_all_plus_255", v=np.full(174, 255, np.int16), result=6))
    rng = np.random.default_rng(0xD)
    cases.append(dict(case="d", name="d_all_negative", v=(-rng.permutation(np.arange(1, 256))[:174]).astype(np.int16), result=5, pattern=0,
                      metric=0, nhard=0))


def _case_e(cases, oracle):
    rng = np.random.default_rng(0xE)
    for _ in range(64):
        bits = rng.integers(0, 2, 77).astype(np.uint8)
        rc, _text = oracle.unpack77(np.packbits(np.concatenate([bits, np.zeros(3, np.uint8)])).tobytes())
        if rc < 0:
            break
    else:
        raise AssertionError("no payload that unpack77 refuses")
    cw = _payload_codeword(bits)
    cases.append(dict(case="e", name="e_unpack_refuses", v=_signed(cw, rng.integers(20, 200, 174)), result=4, pattern=0, nhard=0,
                      payload=bits, codeword=cw))


def _case_f(cases, oracle):
    rng = np.random.default_rng(0xF)
    for e, text in zip(F_ERRORS, ("CQ K1ABC FN42", "CQ K1JT FN20", "W9XYZ K1ABC -11", "K1ABC W9XYZ RR73")):
        rc, a77 = oracle.pack77(text)
        assert rc == 0, text
        cw = _payload_codeword(np.unpackbits(a77)[:77])
        mags = rng.integers(100, 180, 174)
        basis, _ = so.reduced_basis(_order_of(mags))
        outside = [int(p) for p in _order_of(mags) if p not in set(basis.tolist())]      # most reliable first
        weak = outside[len(outside) - e:]
        mags[weak] = rng.integers(1, 5, e)           # moving columns outside the basis to the end leaves the basis as it is
        v = _signed(cw, mags)
        v[weak] = -v[weak]
        cases.append(dict(case="f", name=f"f_{e}_errors", v=v, errors=e, pattern=0, nhard=e, codeword=cw, text=text))


def _case_g(cases):
    rng = np.random.default_rng(0x6)
    cw = _codeword(rng)
    clean = _signed(cw, rng.integers(100, 180, 174))
    basis, _ = so.reduced_basis(_order_of(clean))
    flips = [()] + [(k,) for k in G_SINGLES] + list(G_PAIRS)
    for fl, pat in zip(flips, G_PATTERNS):
        v = clean.copy()
        for k in fl:
            v[basis[k]] = -v[basis[k]]
        cases.append(dict(case="g", name="g_flip_" + ("none" if not fl else "_".join(map(str, fl))), v=v, pattern=pat, nhard=len(fl),
                          codeword=cw, order=len(fl)))


def _case_h(cases):
    rng = np.random.default_rng(0x8)
    for i in range(40):
        cases.append(dict(case="h", name=f"h_{i}", v=(rng.integers(1, 3, 174) * rng.choice([-1, 1], 174)).astype(np.int16)))


def _case_i(cases, n=240):
    rng = np.random.default_rng(0x1)
    edge = (-12, -10, -8, 21, 24, 30)                                  # head before block 0 / tail past block 91
    for i in range(n):
        kind = i % 3
        if kind == 0:
            v = rng.integers(0, 3, 174)
        elif kind == 1:
            v = rng.integers(0, 256, 174)
        else:
            v = rng.integers(0, 4, 174)
            big = rng.choice(174, int(rng.integers(1, 9)), replace=False)
            v[big] = rng.integers(30, 256, len(big))
        c = dict(case="i", name=f"i_{i}", v=(v * rng.choice([-1, 1], 174)).astype(np.int16))
        if i % 4 == 3:
            c["time_offset"] = edge[(i // 4) % len(edge)]
        cases.append(c)


_cases = {}


def build_cases(oracle, sweep=240):
    """the list of cases a..i (dicts: case, name, v int16 [174], and the properties the CPU test holds them to)"""
    if sweep not in _cases:
        cases = []
        _case_a(cases)
        _case_b(cases)
        _case_cd(cases)
        _case_e(cases, oracle)
        _case_f(cases, oracle)
        _case_g(cases)
        _case_h(cases)
        _case_i(cases, sweep)
        for c in cases:
            c["v"].setflags(write=False)
        _cases[sweep] = cases
    return _cases[sweep]


# ---- frames ----------------------------------------------------------------------------------------------------------------

def build_frames(cases, seed=0x5EED, cap=CAP):
    """places the cases: up to 31 attempted candidates per frame at disjoint freq_offset ranges, all four (time_sub, freq_sub),
    records that are only copied (ok != 0, or ldpc_errors == 0) in between, ragged counts, one frame without candidates ->
    dict(cands [B][cap], counts [B], status_in uint8 [B][cap][48], vec int16 [B][cap]: index into cases, -1 = copied only)"""
    rng = np.random.default_rng(seed)
    nframes = (len(cases) + PER_FRAME - 1) // PER_FRAME
    B = nframes + 1
    empty = 1 if B > 2 else B - 1                                      # a frame with count 0 among the others
    cands = np.zeros((B, cap), CAND_DTYPE)
    counts = np.zeros(B, np.int32)
    status = rng.integers(0, 256, (B, cap, 48)).astype(np.uint8)     # junk: an accepted record has to be composed afresh
    vec = np.full((B, cap), -1, np.int16)
    it = iter(range(len(cases)))
    for f in [f for f in range(B) if f != empty]:
        ranges = rng.permutation(PER_FRAME)
        slot = placed = 0
        while slot < cap and placed < PER_FRAME:
            rec = status[f, slot]
            if rng.integers(0, 4) == 0 and slot < cap - 1:           # copied only; the candidate is not looked at
                cands[f, slot] = (int(rng.integers(0, 60)), int(rng.integers(-12, 24)), int(rng.integers(0, 249)), slot & 1, (slot >> 1) & 1)
                if rng.integers(0, 2):
                    rec[9] = (1, 255, 0x40)[int(rng.integers(0, 3))]   # ok != 0, ldpc_errors whatever
                else:
                    rec[9], rec[0], rec[1] = 0, 0, 0                   # BP converged, CRC or unpack77 failed: not OSD's business
                slot += 1
                continue
            ci = next(it, None)
            if ci is None:
                break
            c = cases[ci]
            to = c.get("time_offset", int(rng.integers(-7, 21)))       # -7..20: every data symbol inside the waterfall
            cands[f, slot] = (int(rng.integers(0, 60)), to, 8 * int(ranges[placed]), (slot + f) & 1, ((slot + f) >> 1) & 1)
            rec[9] = 0
            rec[0:2] = np.frombuffer(np.array([1 if ci & 1 else 83], "<i2").tobytes(), np.uint8)
            rec[2:4] = np.frombuffer(np.array([int(rng.integers(0, 51))], "<i2").tobytes(), np.uint8)
            vec[f, slot] = ci
            slot += 1
            placed += 1
        counts[f] = slot
    assert next(it, None) is None
    status[np.arange(cap)[None, :] >= counts[:, None]] = FILL           # behind the counts: bytes nobody may read as records
    return dict(cands=cands, counts=counts, status_in=status, vec=vec)


def waterfalls(vectors, frames):
    """the waterfalls of build_frames' placements, uint8 [B][94208]; vectors: int [n][174]"""
    B = len(frames["counts"])
    mag = np.zeros((B, MAG_ARRAY), np.uint8)
    for f in range(B):
        for i in range(int(frames["counts"][f])):
            if frames["vec"][f, i] >= 0:
                write_candidate(mag[f], vectors[frames["vec"][f, i]], frames["cands"][f, i])
    return mag


def vectors_of(cases):
    return np.stack([c["v"] for c in cases]).astype(np.int16)


def slots(frames):
    """(frame, slot) of every case, by case index"""
    out = {}
    for f, i in np.argwhere(frames["vec"] >= 0):
        out[int(frames["vec"][f, i])] = (int(f), int(i))
    return [out[k] for k in range(len(out))]


def tallies(oracle, cases, frames, mag, infos):
    """what a run reached, from the restatement's answers: infos = {(order, gate): INFO_DTYPE [B][cap]}"""
    where = slots(frames)
    results = sorted(set(int(r) for inf in infos.values() for f in range(len(inf)) for r in inf[f, :frames["counts"][f]]["result"]))
    by_case = {}
    for (order, gate), inf in sorted(infos.items()):
        for ci, (f, i) in enumerate(where):
            by_case.setdefault(cases[ci]["case"], set()).add(int(inf[f, i]["result"]))
    g = sorted(set(int(infos[(c["order"], 83)][where[ci]]["pattern"]) for ci, c in enumerate(cases) if c["case"] == "g"))
    piv, sat = [], {}
    for ci, c in enumerate(cases):
        f, i = where[ci]
        v = effective(c["v"], frames["cands"][f, i]["time_offset"])
        llr = oracle.llr(mag[f], frames["cands"][f, i])
        if np.isfinite(llr).all():
            piv.append(last_pivot(v)[0])
            n = saturated(llr)
            sat[n] = sat.get(n, 0) + 1
    return dict(candidates=len(cases), frames=len(frames["counts"]), results_seen=results,
                results_by_case={k: sorted(v) for k, v in sorted(by_case.items())}, case_g_patterns=g,
                max_last_pivot=int(max(piv)), last_pivots_at_or_past_128=int(sum(p >= 128 for p in piv)),
                saturated_weight_counts={str(k): v for k, v in sorted(sat.items())})


def fixture_status(d, order, gate):
    """the expected status_out of the frozen fixture d (tests/golden/osd_constructed.npz) at (order, gate)"""
    st = np.array(d["status_in"], copy=True)
    hit = d[f"rewritten_o{order}_g{gate}"]
    st[hit[:, 0], hit[:, 1]] = d[f"status_o{order}_g{gate}"]
    return st
