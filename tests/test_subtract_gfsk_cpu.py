"""CPU tests of the GFSK reference of the subtraction in the I/Q samples (include/ft8gpu.h "GFSK reference"): the restatement
tests/ft8_spec_subtract_gfsk.py against unbounded integers and against the synthesiser's own phase, the envelope, shape 0 against
tests/ft8_spec_subtract.py, how deep the two references cancel a GFSK signal whose waveform is known, and order, skipping and
clamping under shape 1.  The device is held to the same restatement in tests/test_gpu_subtract_gfsk.py.  No GPU is used here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ft8_spec_gfsk as sgf
import ft8_spec_subtract as ss
import ft8_spec_subtract_gfsk as sg
import subtract_craft as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F32 = np.float32


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc"), "-j8"])
    m.load_library()
    return m


def tone_patterns():
    """the four records of the issue: all tones equal, alternating 0 and 7, and the two whose end tones reach e[0] and e[80]"""
    rng = np.random.default_rng(11)
    first7, last7 = rng.integers(0, 7, 79), rng.integers(0, 7, 79)
    first7[0], last7[78] = 7, 7
    return {"all_equal": np.full(79, 5), "alternating": np.array([0, 7] * 39 + [0]), "tone0_is_7": first7, "tone78_is_7": last7}


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------

def test_shaped_entries_are_exported_and_refuse_a_null_context(ft8):
    lib = ft8.load_library()
    assert lib.ft8gpu_subtract_messages_shaped(None, None, None, None, None, None, 1, None, None, 1, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_decode_messages_subtracted_shaped(None, None, 1, 2, None, None, None, None, 1, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()
    for name in ("ft8gpu_subtract_messages_shaped", "ft8gpu_decode_messages_subtracted_shaped"):
        assert name in ft8.ABI_SYMBOLS
    assert (ft8.SUBTRACT_CPFSK, ft8.SUBTRACT_GFSK) == (sg.CPFSK, sg.GFSK) == (0, 1)
    src = 'int a[FT8GPU_SUBTRACT_CPFSK == 0 && FT8GPU_SUBTRACT_GFSK == 1 ? 1 : -1];'
    subprocess.run(["gcc", "-std=gnu17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-include", "ft8gpu.h", "-x", "c", "-"],
                   input=src, text=True, check=True)


# ---- (b') the phase ---------------------------------------------------------------------------------------------------------------------

def test_tables_are_the_synthesisers(ft8):
    Q, ramp = sg.tables()
    assert Q.tobytes() == sgf.pulse(512).tobytes() and ramp.tobytes() == sgf.ramp(512).tobytes()
    assert Q[0] == 0 and ramp[0] == 0.0 and ramp.max() < 1.0             # a ramped sample is never one the rule leaves unramped


@pytest.mark.parametrize("k4", [0, 1, 4095, 4096 + 5, -7])
def test_phase_against_python_integers_and_the_synthesiser(ft8, k4):
    """theta from unbounded integers reduced once at the end, and from the synthesiser's own phase at step = k4 * 2^20; a negative
    k4 and 4096 + 5 go through the uint32 wrap"""
    Q = [int(v) for v in sg.tables()[0]]
    for name, tones in tone_patterns().items():
        S = -1234
        j, th = sg.theta(S, k4, tones)
        assert j.reshape(-1).tolist() == list(range(S, S + 79 * 512)) and th.min() >= 0 and th.max() < 4096
        e = [int(tones[0])] + [int(t) for t in tones] + [int(tones[78])]
        assert len(e) == 81 and sg.extended(tones).tolist() == e
        want = []
        for n in range(79 * 512):
            m, k = divmod(n, 512)
            phi = (k4 * (1 << 20)) * n + e[m] * Q[k + 1024] + e[m + 1] * Q[k + 512] + e[m + 2] * Q[k]
            want.append((((phi % (1 << 32)) + (1 << 19)) >> 20) & 4095)
        assert th.reshape(-1).tolist() == want, (name, k4)
        synth = sgf.phase(tones, (k4 << 20) & 0xFFFFFFFF, sgf.IQ)
        assert synth.dtype == np.uint32 and (sg.phi(k4, tones, sg.tables()[0]) == synth).all(), (name, k4)
        assert ((((synth.astype(np.int64) + (1 << 19)) >> 20) & 4095) == th.reshape(-1)).all(), (name, k4)


def test_end_tones_reach_the_phase(ft8):
    """e[0] and e[80] are part of the rule: changing tone[0] moves the phase of the first symbol by more than its own step, and
    tone[78] likewise at the far end; a record of equal tones is a plain complex exponential up to the table's rounding"""
    pats = tone_patterns()
    _j, th = sg.theta(0, 100, pats["all_equal"])
    lin = ((100 + 8 * 5) * np.arange(79 * 512, dtype=np.int64)) % 4096   # e sums to the tone where the pulse's three parts do
    d = (th.reshape(-1) - lin) % 4096
    d = np.minimum(d, 4096 - d)
    assert d.max() <= 1 + 8 * 5 and (d[512:] == d[512]).all()            # a constant behind the first symbol's start-up
    a, b = pats["tone0_is_7"].copy(), pats["tone0_is_7"].copy()
    b[0] = 0
    assert (sg.theta(0, 100, a)[1][0] != sg.theta(0, 100, b)[1][0]).any()
    a, b = pats["tone78_is_7"].copy(), pats["tone78_is_7"].copy()
    b[78] = 0
    assert (sg.theta(0, 100, a)[1][78] != sg.theta(0, 100, b)[1][78]).any()
    assert (sg.theta(0, 100, a)[1][:77] == sg.theta(0, 100, b)[1][:77]).all()      # a tone reaches one symbol back, not two


# ---- (e') the envelope ------------------------------------------------------------------------------------------------------------------

def test_envelope_and_the_unramped_middle(ft8):
    env = sg.envelope()
    assert env.dtype == F32 and env.tobytes() == sgf.envelope(sgf.IQ).tobytes()
    assert (env[64:40384] == 1.0).all() and (env[:64] != 1.0).all() and (env[40384:] != 1.0).all()
    assert env[0] == 0.0 and env[40447] == 0.0 and env[63] == env[40384]
    # a record with a made-up amplitude, applied with the ramp and with another ramp: samples 64 .. 40383 never see either
    rng = np.random.default_rng(5)
    w4 = ss.twiddles()
    tones = tone_patterns()["alternating"]
    info = np.zeros(1, ss.INFO_DTYPE)[0]
    info["s_best"], info["k4"], info["valid"] = 1000, 1286, 1
    A = (rng.normal(0, 1, ss.NSEG).astype(F32), rng.normal(0, 1, ss.NSEG).astype(F32))
    x = rng.normal(0, 1, (2, ss.NSAMPLES)).astype(F32)
    got, other, plain = x.copy(), x.copy(), x.copy()
    sg.apply_record(got[0], got[1], info, tones, A, w4, sg.GFSK)
    sg.apply_gfsk(other[0], other[1], info, tones, A, w4, ramp=np.full(64, 2.0, F32))
    step_e = ss.apply_record
    with sg.rule(sg.GFSK):                                               # step (e) as it is, on the phase of (b'): no ramp at all
        step_e(plain[0], plain[1], info, tones, A, w4)
    lo, hi = 1000 + 64, 1000 + 40384
    assert got[:, lo:hi].tobytes() == other[:, lo:hi].tobytes() == plain[:, lo:hi].tobytes()
    assert (got[:, 1000:lo] != plain[:, 1000:lo]).mean() > 0.9 and (got[:, hi:hi + 64] != plain[:, hi:hi + 64]).mean() > 0.9
    assert got[:, :1001].tobytes() == x[:, :1001].tobytes()              # r[0] = 0: the record's first sample keeps its value
    assert got[:, hi + 64:].tobytes() == x[:, hi + 64:].tobytes() and (got[:, lo:hi] != x[:, lo:hi]).mean() > 0.99
    # an infinite amplitude under r[0] = 0 is a NaN, by IEEE
    A_inf = (A[0].copy(), A[1].copy())
    A_inf[0][0] = np.inf
    bad = x.copy()
    sg.apply_record(bad[0], bad[1], info, tones, A_inf, w4, sg.GFSK)
    assert np.isnan(bad[0, 1000]) and np.isnan(bad[1, 1000])


# ---- shape 0, and the module it borrows from ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def constructed(ft8):
    iq, msgs, refined, first, n, where = sc.constructed(ft8)
    fill = np.full((6, 50 * 64), sc.FILL, np.uint8).view(ss.INFO_DTYPE).reshape(6, 50)
    w4 = ss.twiddles()
    before = (ss.theta, ss.apply_record, ss.subtract, ss.estimate_record)
    out1, info1 = sg.subtract(iq, msgs, refined, first, n, w4, sg.GFSK, info=fill)
    assert (ss.theta, ss.apply_record, ss.subtract, ss.estimate_record) == before
    return iq, msgs, refined, first, n, where, fill, w4, out1, info1


def test_shape_0_is_the_existing_restatement_and_its_module_is_left_alone(constructed):
    iq, msgs, refined, first, n, where, fill, w4, out1, info1 = constructed
    before = (ss.theta, ss.apply_record, ss.subtract, ss.estimate_record, ss.decode_passes_subtracted)
    want_out, want_info = ss.subtract(iq, msgs, refined, first, n, w4, info=fill)
    got_out, got_info = sg.subtract(iq, msgs, refined, first, n, w4, sg.CPFSK, info=fill)
    assert got_out.tobytes() == want_out.tobytes() and got_info.tobytes() == want_info.tobytes()
    assert out1.tobytes() != want_out.tobytes() and info1.tobytes() != want_info.tobytes()          # shape 1 is another rule
    for bad in (2, -1, None):
        with pytest.raises(ValueError):
            sg.subtract(iq, msgs, refined, first, n, w4, bad)
    with pytest.raises(ZeroDivisionError):                               # an exception inside does not leave the module altered either
        with sg.rule(sg.GFSK):
            assert ss.theta is not before[0]
            1 / 0
    assert (ss.theta, ss.apply_record, ss.subtract, ss.estimate_record, ss.decode_passes_subtracted) == before
    again, _ = ss.subtract(iq[5:6], msgs[5:6], refined[5:6], first[5:6], n[5:6], w4)
    assert again.tobytes() == want_out[5:6].tobytes()


# ---- order, skipping, clamping under shape 1 ---------------------------------------------------------------------------------------------

def test_order_skipping_and_clamping_under_shape_1(constructed):
    iq, msgs, refined, first, n, where, fill, w4, out, info = constructed
    raw = info.view(np.uint8).reshape(6, 50, 64)
    assert (raw[0] != sc.FILL).any(axis=1).all()                         # first = -3 and n_msgs = 70 are 0 and 50
    assert (raw[1] == sc.FILL).all() and (raw[2, 3:] == sc.FILL).all() and (raw[3, :2] == sc.FILL).all() and (raw[4] == sc.FILL).all()
    for name in ("not_valid", "not_valid_random"):
        assert info[where[name]].tobytes() == bytes(64)                  # R.valid = 0: skipped, the info all zero
    skipped, _ = sg.subtract(iq[:1], msgs[:1], refined[:1], [where["not_valid"][1]], [where["not_valid"][1] + 1], w4, sg.GFSK)
    assert skipped.tobytes() == iq[:1].tobytes()
    for f in (1, 2, 4):
        assert out[f].tobytes() == iq[f].tobytes()
    f = 5                                                                # three records that overlap on the same samples
    fwd, _ = sg.subtract(iq[f:f + 1], msgs[f:f + 1], refined[f:f + 1], [0], [3], w4, sg.GFSK)
    rev, _ = sg.subtract(iq[f:f + 1], msgs[f:f + 1], refined[f:f + 1], [0], [3], w4, sg.GFSK, order=lambda r: r[::-1])
    assert fwd.tobytes() == out[f:f + 1].tobytes()
    assert (fwd != rev).sum() > 0 and np.abs(fwd - rev).max() < 1e-6     # the order is part of the rule, in the last bits
    # every estimate comes from the input frame
    two, info2 = sg.subtract(iq[f:f + 1], msgs[f:f + 1], refined[f:f + 1], [0], [2], w4, sg.GFSK)
    one, info1 = sg.subtract(iq[f:f + 1], msgs[f:f + 1], refined[f:f + 1], [1], [2], w4, sg.GFSK)
    assert info2[0, 1].tobytes() == info1[0, 1].tobytes()


# ---- depth on GFSK signals -------------------------------------------------------------------------------------------------------------------

def test_gfsk_reference_cancels_a_gfsk_signal_deeper(oracle, ft8):
    """16 noiseless single-signal GFSK frames (subtract_craft.suppression_frames under tools/gfsk_effect.waveform, a seed other
    than the profile's), decoded by the oracle, refined, and subtracted with either reference: |x' - (x - s)|^2 / |s|^2 in dB, s the
    synthesiser's noiseless GFSK waveform.  On every frame the GFSK reference leaves less than the CPFSK reference leaves on the
    same frame; its worst case is below the -19 dB the CPFSK stage is held to on its own waveform, and within 3 dB of the worst
    case of 64 frames in profiles/subtract_gfsk_accuracy.json (the margin covers seeds, as in tests/test_subtract_cpu.py)."""
    from gfsk_effect import waveform
    with open(os.path.join(ROOT, "profiles", "subtract_gfsk_accuracy.json")) as f:
        doc = json.load(f)
    committed = {(r["set"], r["shape"]): r for r in doc["sets"]}
    assert doc["waveform"] == "gfsk" and doc["frames_per_set"] == 64 and len(committed) == 6
    with waveform("gfsk"):
        iq, s, _f0, _start = sc.suppression_frames(oracle, 16, None, 20261201)
    db = {}
    for shape in (sg.CPFSK, sg.GFSK):
        with sg.rule(shape):
            db[shape] = sc.suppression_db(oracle, iq, s)
    print(json.dumps({str(k): [round(float(v), 2) for v in d] for k, d in db.items()}))
    assert len(db[0]) == 16 and len(db[1]) == 16                         # every frame decodes, so the two lists pair up
    assert (db[1] < db[0]).all(), (db[0] - db[1]).min()
    worst = float(db[1].max())
    assert worst < -19.0
    assert worst <= committed[("noiseless", 1)]["worst_db"] + 3.0
    assert committed[("noiseless", 1)]["worst_db"] < -19.0 and committed[("noiseless", 1)]["decoded"] == 64
    assert committed[("noiseless", 1)]["median_db"] < committed[("noiseless", 0)]["median_db"]
