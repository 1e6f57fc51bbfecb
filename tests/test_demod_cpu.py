"""CPU tests of the demodulation from the I/Q samples (include/ft8gpu.h "demodulation from the I/Q samples"): the record and
parameter layouts against gcc, the properties of the restatement tests/ft8_spec_demod.py on noiseless signals that start off
the grid, the first-strict-maximum rule, frames of zeros and with a NaN, the hand-made inputs of tests/demod_craft.py (which the
device is held to in tests/test_gpu_demod.py), the constructed signals and long lists of tests/demod_edges_craft.py, each named
case asserted by name (results 3 and 4, acceptance by set 2 and set 3, the soft-bit bounds around the division guard, the float
edges of the powers, extreme records and the frame's edges), and a seeded sensitivity row.  No GPU is used here."""
import os
import subprocess

import numpy as np
import pytest

import combine_craft as cc
import demod_craft as dc
import demod_edges_craft as de
import ft8_spec_combine as sc
import ft8_spec_demod as sdm
import ft8_spec_osd as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc"), "-j8"])
    m.load_library()
    return m


@pytest.fixture(scope="module")
def w4(ft8):
    return sdm.twiddles()


def test_layouts_against_gcc(ft8, tmp_path):
    fields = ("result", "set", "nhard", "e_best", "d_best", "pad0", "psync", "pad")
    pfields = ("sets", "max_hard_errors", "max_per_frame")
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ft8gpu.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(ft8gpu_demod_info));', 'printf("psize %zu\\n", sizeof(ft8gpu_demod_params));']
    lines += [f'printf("{f} %zu\\n", offsetof(ft8gpu_demod_info, {f}));' for f in fields]
    lines += [f'printf("p_{f} %zu\\n", offsetof(ft8gpu_demod_params, {f}));' for f in pfields]
    lines += ['printf("consts %d %d %d %d %d\\n", FT8GPU_DEMOD_TSTEP, FT8GPU_DEMOD_TRANGE, FT8GPU_DEMOD_FRANGE, '
              'FT8GPU_DEMOD_MAX_HARD_ERRORS, FT8GPU_DEMOD_SETS);', 'return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=gnu17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    want = {"size": "16", "psize": "12", "result": "0", "set": "1", "nhard": "2", "e_best": "3", "d_best": "4", "pad0": "5", "psync": "8",
            "pad": "12", "p_sets": "0", "p_max_hard_errors": "4", "p_max_per_frame": "8",
            "consts": f"{sdm.TSTEP} {sdm.TRANGE} {sdm.FRANGE} {sdm.MAX_HARD_ERRORS} {sdm.SETS}"}
    assert got == want
    for dt in (ft8.DEMOD_INFO_DTYPE, sdm.INFO_DTYPE):
        assert dt.itemsize == 16 and [dt.fields[f][1] for f in fields] == [int(want[f]) for f in fields]
    assert ft8.DEMOD_INFO_DTYPE == sdm.INFO_DTYPE and (ft8.DEMOD_MAX_HARD_ERRORS, ft8.DEMOD_SETS) == (sdm.MAX_HARD_ERRORS, sdm.SETS)
    import ctypes as C
    assert C.sizeof(ft8.DemodParams) == 12 and [getattr(ft8.DemodParams, f).offset for f in pfields] == [0, 4, 8]
    assert sdm.C8.tobytes() == np.uint32(0x3F3504F3).tobytes()


def test_the_dft_and_the_butterfly_are_what_they_are_named_for():
    rng = np.random.default_rng(1)
    y = rng.normal(size=(5, 8)) + 1j * rng.normal(size=(5, 8))
    ur, ui = sdm.dft8(y.real.astype(F32), y.imag.astype(F32))
    assert np.allclose(ur + 1j * ui, np.fft.fft(y, axis=-1), atol=1e-5)
    v = rng.normal(size=(3, 64)).astype(F32)
    assert np.allclose(sdm.butterfly(v), v.astype(np.float64).sum(axis=-1), atol=1e-4)


def test_blocks_partition_the_data_symbols():
    data = list(range(7, 36)) + list(range(43, 72))
    for n, sizes in ((1, [1] * 29), (2, [2] * 14 + [1]), (3, [3] * 9 + [2])):
        b = sdm.blocks(n)
        assert [len(x) for x in b] == sizes + sizes
        assert [m for x in b for m in x] == data
    assert sorted(3 * sdm.data_index(m) + k for m in data for k in range(3)) == list(range(174))


# (time_offset, time_sub, freq_offset, freq_sub, samples past the candidate's own start, Hz above its own frequency)
OFF_GRID = [(6, 0, 100, 1, 0, 0.0), (6, 1, 41, 0, 37, 0.0), (3, 0, 200, 0, -77, 0.5), (10, 1, 150, 1, 100, -1.3), (4, 0, 77, 1, -128, 1.5)]


@pytest.mark.parametrize("case", OFF_GRID)
def test_restatement_properties_on_noiseless_signals(oracle, ft8, w4, case):
    to, ts, fo, fs, dt, df = case
    frame = np.zeros((2, dc.NSAMPLES))
    tones = dc.place(oracle, frame, dc.TEXTS[2], to, ts, fo, fs, dt=dt, df=df, phase0=1.1)
    I, Q = frame.astype(F32)
    T, Fq = 2 * to + ts, 2 * fo + fs
    e, d, psync, pt, pf = sdm.fine_sync(I, Q, w4, T, Fq)
    assert abs(e - dt / 32.0) <= 1.0 and abs(d - df / 0.78125) <= 1.0, (e, d)
    assert psync == pf[d + sdm.FRANGE] and psync == pf.max() and pt[e + sdm.TRANGE] == pt.max()
    zr, zi = sdm.spectra(I, Q, w4, T, Fq, e, d)
    own = zr[np.arange(79), tones] + 1j * zi[np.arange(79), tones]
    # Common phase.  The residual frequency r turns the phase by 2 pi r 512 / 3200 per symbol, 78 symbols in all; a window
    # that starts s samples off the true start reads tone t at a phase 2 pi 6.25 t s / 3200 from tone 0's, t <= 7, and takes
    # in |s| / 512 of a neighbouring symbol, which turns the sum by at most asin(|s| / (512 - |s|)); float32 noise is far below.
    r, s = df - 0.78125 * d, dt - 32 * e
    assert abs(r) <= 0.78125 / 2 + 1e-9 and abs(s) <= 16
    ph = np.unwrap(np.angle(own))
    drift = 2 * np.pi * r * 512 / 3200 * np.arange(79)
    tol = 2 * np.pi * 6.25 * 7 * abs(s) / 3200 + 2 * np.arcsin(abs(s) / (512 - abs(s))) + 1e-3
    assert np.ptp(ph - drift) <= tol, (np.ptp(ph - drift), tol)
    cw = np.array([b for k in list(range(7, 36)) + list(range(43, 72)) for b in np.unpackbits(np.uint8(sdm.GRAY.index(int(tones[k]))))[5:]])
    for n in (1, 2, 3):
        llr = sdm.soft_bits(zr, zi, n)
        assert ((llr > 0) == cw.astype(bool)).all() and np.isfinite(llr).all(), n
    cand = np.array([(20, to, fo, ts, fs)], ft8.CAND_DTYPE)[0]
    info, win = sdm.demod_one(oracle, I, Q, cand, w4, 7, 0, bp=oracle.bp_decode)
    assert (info["result"], info["set"], info["nhard"]) == (1, 1, 0) and win[4] == dc.TEXTS[2].encode()


def test_first_strict_maximum_on_tied_powers():
    f = lambda *p: sdm.first_strict_max(np.array(p, F32))
    assert f(1, 1, 1) == 0 and f(1, 2, 2, 1) == 1 and f(0, 0, 3, 3, 3) == 2 and f(5, 4, 5) == 0
    assert f(np.nan, 9, 1) == 0 and f(1, np.nan, 2) == 2 and f(0.0, -0.0) == 0


def test_zeros_and_a_nan_give_result_6(oracle, ft8, w4):
    cand = np.array([(20, 5, 100, 1, 0)], ft8.CAND_DTYPE)[0]
    z = np.zeros(dc.NSAMPLES, F32)
    info, win = sdm.demod_one(oracle, z, z, cand, w4, 7, 174, bp=oracle.bp_decode)
    assert win is None and (info["result"], info["set"], info["e_best"], info["d_best"]) == (6, 3, -4, -2)
    assert info["psync"].tobytes() == bytes(4)
    frame = np.zeros((2, dc.NSAMPLES))
    dc.place(oracle, frame, dc.TEXTS[0], 5, 1, 100, 0)
    I, Q = frame.astype(F32)
    Q[20000] = np.nan
    for sets in range(1, 8):
        info, win = sdm.demod_one(oracle, I, Q, cand, w4, sets, 174, bp=oracle.bp_decode)
        assert win is None and info["result"] == 6 and info["set"] == sets.bit_length()
        assert info["psync"].view(np.uint32) == 0x7FC00000 or np.isfinite(info["psync"])


def test_hand_made_candidates_are_what_they_are_named_for(oracle, ft8):
    iq, cands, counts, status, where = dc.constructed(ft8, oracle)
    cache = {}
    st, info = sdm.demod_candidates(oracle, iq, cands, counts, status, 7, 174, bp=oracle.bp_decode, cache=cache)
    for name, e, d in (("truth_at_e+4_d+2", 4, 2), ("truth_at_e-4_d-2", -4, -2), ("truth_at_e+4_d-2", 4, -2), ("truth_at_e-4_d+2", -4, 2),
                       ("before_the_frame", 0, 0), ("past_the_frame", 0, 0)):
        r = info[where[name]]
        assert (r["result"], r["e_best"], r["d_best"]) == (1, e, d), name
        assert st.view(ft8.STATUS_DTYPE).reshape(4, -1)[where[name]]["ok"] == 1
    assert 256 * sc.position(cands[where["before_the_frame"]])[0] + 256 < -5000
    assert 256 * sc.position(cands[where["past_the_frame"]])[0] + 256 + 79 * 512 > dc.NSAMPLES + 4000
    assert info[where["already_decoded"]].tobytes() == bytes(16) and info[where["bp_left_no_errors"]].tobytes() == bytes(16)
    assert st[where["already_decoded"]].tobytes() == status[where["already_decoded"]].tobytes()
    assert info[where["noise_only"]]["result"] == 7
    assert (info[1, :3]["result"] == 6).all() and (info[2, 20:]["result"] == 6).all() and (info[2, :20]["result"] != 6).all()
    assert (info[3].view(np.uint8) == 0).all() and (st[3] == 0).all()                       # behind the count: what the arrays held
    results = set()
    for sets, gate, mpf in ((7, 0, dc.CAP), (2, 174, dc.CAP), (4, 174, 1)):
        _st, inf = sdm.demod_candidates(oracle, iq, cands, counts, status, sets, gate, mpf, bp=oracle.bp_decode, cache=cache)
        results |= set(int(r) for f in range(4) for r in inf[f, :counts[f]]["result"])
        if mpf == 1:
            assert [(inf[f]["set"] != 0).sum() for f in range(4)] == [1, 1, 1, 0]
    assert {0, 1, 2, 6, 7} <= results


def test_tones_of_any_codeword_are_the_encoder_s(oracle, ft8):
    for text in dc.TEXTS:
        tones, _payload = dc.tones_of(oracle, text)
        assert (de.tones_of_codeword(cc.codeword_of(text)) == np.asarray(tones)).all(), text
    word = de.word_with_crc(np.ones(77, np.uint8), flip=0)
    assert int("".join(map(str, word[77:91])), 2) == so.crc14(word[:77]) ^ 0x2000
    assert not (so.parity_check_matrix().astype(np.int64) @ word & 1).any()


@pytest.fixture(scope="module")
def edges(oracle, ft8):
    iq, cands, counts, status, where = de.constructed(ft8, oracle)
    return dict(iq=iq, cands=cands, counts=counts, status=status, where=where, cache={})


def test_constructed_edges_are_what_they_are_named_for(oracle, ft8, edges):
    """every named case of tests/demod_edges_craft.py, by name, with the restatement and the library's twiddles"""
    x = edges
    where, nh = x["where"], x["where"]["nhard"]
    B = len(x["iq"])

    def run(sets=7, gate=174):
        st, info = sdm.demod_candidates(oracle, x["iq"], x["cands"], x["counts"], x["status"], sets, gate, bp=oracle.bp_decode, cache=x["cache"])
        return st.view(ft8.STATUS_DTYPE).reshape(B, -1), info

    def sets_of(name):
        """what each set gives at gate 174: {n: (result, nhard)} and {n: x}"""
        _e, _d, _psync, per_set = x["cache"][(where[name][0], x["cands"][where[name]].tobytes())]
        out = {}
        for n, (_llr, xs, plain, errors) in per_set.items():
            out[n] = (6, 0) if xs is None else sdm.judge(oracle, plain, errors, xs, 174)[:2]
        return out, {n: per_set[n][1] for n in per_set}

    def bits_of(v):
        return int(np.float32(v).view(np.uint32))

    st7, info7 = run()
    results = set(int(r) for f in range(B) for r in info7[f, :x["counts"][f]]["result"])
    accepted = set(int(r["set"]) for f in range(B) for r in info7[f, :x["counts"][f]] if r["result"] == 1)
    assert all(r["set"] != 0 or name == "does_not_qualify" for name, at in where.items() if name != "nhard" for r in [info7[at]])
    assert info7[where["does_not_qualify"]].tobytes() == bytes(16)

    # (a) BP converges and a check behind it refuses, whichever sets are tried; the all-zero word is never counted
    for sets in (1, 2, 4, 7):
        st, info = run(sets)
        last = sets.bit_length()
        for name, code in (("crc_refuses", 3), ("crc_refuses_last", 3), ("unpack_refuses", 4), ("all_zero_word", 7)):
            r = info[where[name]]
            assert (r["result"], r["set"], r["nhard"]) == (code, last, 0), (name, sets, r)
            assert st[where[name]].tobytes() == x["status"][where[name]].tobytes()
        r = info[where["good_behind_a_refusal"]]
        assert (r["result"], r["set"], r["nhard"]) == (1, (sets & -sets).bit_length(), 0)
        assert st[where["good_behind_a_refusal"]]["text"] == dc.TEXTS[1].encode() and st[where["good_behind_a_refusal"]]["ok"] == 1
        results |= set(int(r) for f in range(B) for r in info[f, :x["counts"][f]]["result"])
    for name in ("crc_refuses", "crc_refuses_last", "unpack_refuses"):
        assert [sets_of(name)[0][n][0] for n in (1, 2, 3)] == [3 if "crc" in name else 4] * 3, name
    assert where["crc_refuses"][0] == where["good_behind_a_refusal"][0] and where["crc_refuses"][1] < where["good_behind_a_refusal"][1]

    # (b) the named set accepts after the sets before it found no codeword; the gate at its nhard and one below
    per2, per3 = sets_of("set2_accepts")[0], sets_of("set3_accepts")[0]
    assert (per2[1], per2[2], per2[3]) == ((7, 0), (1, nh["set2_accepts"]), (7, 0))
    assert (per3[1], per3[2], per3[3]) == ((7, 0), (7, 0), (1, nh["set3_accepts"]))
    for name, n, after in (("set2_accepts", 2, (7, 3, 0)), ("set3_accepts", 3, (2, 3, nh["set3_accepts"]))):
        r = info7[where[name]]
        assert (r["result"], r["set"], r["nhard"]) == (1, n, nh[name]), (name, r)
        st, info = run(7, nh[name])
        r = info[where[name]]
        assert (r["result"], r["set"], r["nhard"]) == (1, n, nh[name]) and st[where[name]]["ok"] == 1, (name, r)
        st, info = run(7, nh[name] - 1)
        r = info[where[name]]
        assert (r["result"], r["set"], r["nhard"]) == after and st[where[name]]["ok"] == 0, (name, r)
        _st, info = run(1 << (n - 1), nh[name] - 1)
        assert (info[where[name]]["result"], info[where[name]]["nhard"]) == (2, nh[name])
        results |= set(int(r) for f in range(B) for r in info[f, :x["counts"][f]]["result"])
    assert nh["set2_accepts"] >= 1 and nh["set3_accepts"] >= 1

    # (c) set 1's smallest nonzero normalised soft bit against the guard's 2^-58; the symbol's soft bits in sets 2 and 3 are zeros
    own = slice(3 * sdm.data_index(de.TINY_SYMBOL), 3 * sdm.data_index(de.TINY_SYMBOL) + 3)
    for name, lo, hi in (("soft_bits_just_above", 2.0 ** -58, 2.0 ** -57), ("tiny_soft_bits", 2.0 ** -59, 2.0 ** -58),
                         ("tiny_soft_bits_deepest", 2.0 ** -82, 2.0 ** -80), ("tiny_soft_bits_below_tanh_domain", 2.0 ** -126, 2.0 ** -82),
                         ("subnormal_soft_bit", 2.0 ** -149, 2.0 ** -126)):
        per, xs = sets_of(name)
        a = np.abs(xs[1].astype(np.float64))
        assert (a != 0).all() and lo <= a.min() < hi and a[own].min() == a.min(), (name, a.min())
        assert np.sort(a)[3] > 1.0, "only the scaled symbol's three soft bits are small"
        assert (xs[2][own] == 0).all() and (xs[3][own] == 0).all() and (xs[2] != 0).sum() == 171 and (xs[3] != 0).sum() == 171
        r = info7[where[name]]
        assert (r["result"], r["set"], r["nhard"], r["e_best"], r["d_best"]) == (1, 1, 0, 0, 0) and per[2][0] == 1 and per[3][0] == 1, name

    # (d) every sample times a power of two
    def scaled(name):
        r = info7[where["scaled_" + name]]
        return int(r["result"]), int(r["e_best"]), int(r["d_best"]), bits_of(r["psync"]), float(r["psync"])
    res, e, d, bits, p = scaled("accepted_tiny_psync")
    assert res == 1 and (e, d) == (1, -1) and 0x00800000 <= bits and p < 2.0 ** -100
    res, e, d, bits, p = scaled("subnormal_psync")
    assert res == 6 and (e, d) == (1, -1) and 0 < bits < 0x00800000
    res, e, d, bits, p = scaled("last_nonzero_psync")
    assert res == 6 and 0 < bits < 0x00000100
    res, e, d, bits, p = scaled("accepted_top")
    assert res == 1 and (e, d) == (1, -1) and 2.0 ** 120 < p < np.inf
    res, e, d, bits, p = scaled("variance_overflows")
    assert res == 7 and (e, d) == (1, -1) and np.isfinite(p)
    for n, (llr, xs, _plain, errors) in x["cache"][(where["scaled_variance_overflows"][0], x["cands"][where["scaled_variance_overflows"]].tobytes())][3].items():
        assert np.isfinite(llr).all() and (np.abs(llr) > 2.0 ** 50).all() and (xs == 0).all() and errors != 0, "finite soft bits, a norm factor of zero"
    res, e, d, bits, p = scaled("not_finite")
    assert res == 6 and (e, d) == (1, -1) and np.isfinite(p)
    res, e, d, bits, p = scaled("inf_psync")
    assert res == 6 and e > -4 and bits == 0x7F800000
    res, e, d, bits, p = scaled("nan_psync")
    assert res == 6 and (e, d) == (-4, -2) and bits == 0x7FC00000
    f = where["scaled_nan_psync"][0]
    assert np.isfinite(x["iq"][f]).all(), "the NaN comes from the arithmetic, not from a sample"
    assert st7[where["scaled_accepted_tiny_psync"]]["text"] == st7[where["scaled_accepted_top"]]["text"] == dc.TEXTS[1].encode()

    # (e) a NaN with a sign and a payload, and -inf beside +inf, inside a Costas symbol: one canonical NaN
    f, i = where["nan_payload"]
    assert (x["iq"][f].view(np.uint32) == de.NAN_BITS).sum() == 1
    for name in ("nan_payload", "inf_beside_minus_inf"):
        r = info7[where[name]]
        assert bits_of(r["psync"]) == 0x7FC00000 and (r["e_best"], r["d_best"]) == (-4, -2), (name, r)

    # (f) extreme fields and the frame's edges
    out_of_reach = [f"field_extremes_{k}" for k in range(len(de.EXTREMES))] + [f"edge_T{T}_fo{fo}" for T in (-160, 187) for fo in (0, 255)]
    for name in out_of_reach:
        r = info7[where[name]]
        assert (r["result"], r["set"], r["e_best"], r["d_best"], bits_of(r["psync"])) == (6, 3, -4, -2, 0), (name, r)
    for T in (-159, 186):
        for fo in (0, 255):
            r = info7[where[f"edge_T{T}_fo{fo}"]]
            assert r["psync"] > 0 and (r["e_best"] >= 1 if T < 0 else r["e_best"] <= 3), (T, fo, r)      # the e whose window is inside
    assert [tuple(int(v) for v in x["cands"][where[f"field_extremes_{k}"]].tolist()) for k in range(4)] == [tuple(r) for r in de.EXTREMES]

    assert {0, 1, 2, 3, 4, 6, 7} <= results and 5 not in results and accepted == {1, 2, 3}, (results, accepted)


def test_long_lists_are_what_they_are_made_for(ft8):
    for cap, counts in de.LONG.items():
        iq, cands, got_counts, status = de.long_lists(ft8, cap)
        assert tuple(got_counts) == counts and cands.shape == (len(counts), cap)
        for f, n in enumerate(counts):
            q = (status[f, :n]["ok"] == 0) & (status[f, :n]["ldpc_errors"] != 0)
            assert (~q).sum() == n // 3 and not q[2::3].any() and len(set(c.tobytes() for c in cands[f, :n])) <= len(de.LONG_RECORDS)
            assert (status[f, n:].view(np.uint8) == dc.FILL).all() and (cands[f, n:].view(np.uint8) == dc.FILL).all()
        assert (status[0]["ok"] == 1).any() and ((status[0]["ok"] == 0) & (status[0]["ldpc_errors"] == 0)).any()
    iq, cands, counts, status = de.long_lists(ft8, 70)
    q = np.flatnonzero((status[0]["ok"] == 0) & (status[0]["ldpc_errors"] != 0))
    assert len(q) == 47 and q[42] == 63 and q[43] == 64, "max_per_frame = 43 ends with the first chunk of 64, 44 begins the second"
    assert not iq[0].any() and iq[1].any()


def test_seeded_sensitivity_row(oracle, ft8, w4):
    """32 frames of one station at -19 dB, where tools/demod_gain.py found BP nearest one half (15 of 64 at -19 dB, 49 of 64 at
    -18 dB: equally far; the lower one), seeds 3500 .. 3531 of its row"""
    import ft8_spec_messages as sm
    import synth_util as S
    enc = S.oracle_encode_fn(oracle)
    frames = [S.make_frame(seed, 1, enc, snr_range=(-19.0, -19.0)) for seed in range(3500, 3532)]
    iq = np.stack([np.ascontiguousarray(f[0], F32) for f in frames])
    out, n, nbs = sdm.decode_demod(oracle, iq, sdm.SETS, sdm.MAX_HARD_ERRORS, nthreads=4, bp=oracle.bp_decode)
    assert (nbs[:, 1] - nbs[:, 0]).sum() >= 1, nbs.tolist()
    for f in range(len(frames)):
        for m in out[f, :n[f]]:
            assert m["text"].decode() in frames[f][1], (f, m["text"])
        assert all(1 <= int(m["pad"][3]) <= 3 for m in out[f, nbs[f, 0]:n[f]])
