"""CPU tests of the subtraction in the I/Q samples (include/ft8gpu.h "subtraction in the I/Q samples"): the info layout against
gcc, the table of the host helper, the restatement tests/ft8_spec_subtract.py against direct evaluations and on the hand-made
records of tests/subtract_craft.py (which the device is held to in tests/test_gpu_subtract.py), how well the rule cancels a signal
whose waveform is known, and the frames on which subtraction uncovers a message that masking does not.  No GPU is used here."""
import json
import os
import subprocess

import numpy as np
import pytest

import ft8_spec_refine as sr
import ft8_spec_subtract as ss
import subtract_craft as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc"), "-j8"])
    m.load_library()
    return m


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------

def test_info_layout_against_gcc(ft8, tmp_path):
    fields = ("k4", "s_best", "d_best", "t_best", "valid", "pad0", "pf", "pt", "pad")
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ft8gpu.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(ft8gpu_subtract_info));']
    lines += [f'printf("{f} %zu\\n", offsetof(ft8gpu_subtract_info, {f}));' for f in fields]
    lines += ['printf("consts %d %d %d %d\\n", FT8GPU_SUBTRACT_TABLE, FT8GPU_SUBTRACT_SMOOTH, FT8GPU_SUBTRACT_RANGE, FT8GPU_SUBTRACT_TSTEP);',
              'return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=gnu17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    want = {"size": "64", "k4": "0", "s_best": "4", "d_best": "8", "t_best": "9", "valid": "10", "pad0": "11", "pf": "12", "pt": "32",
            "pad": "52", "consts": f"{ss.TABLE} {ss.SMOOTH} {ss.RANGE} {ss.TSTEP}"}
    assert got == want
    for dt in (ft8.SUBTRACT_INFO_DTYPE, ss.INFO_DTYPE):
        assert dt.itemsize == 64 and [dt.fields[f][1] for f in fields] == [int(want[f]) for f in fields]
    assert ft8.SUBTRACT_INFO_DTYPE == ss.INFO_DTYPE and (ss.TABLE, ss.SMOOTH, ss.RANGE, ss.TSTEP) == (4096, 8, 2, 8)


def test_entries_refuse_bad_arguments_before_touching_a_gpu(ft8):
    lib = ft8.load_library()
    assert lib.ft8gpu_subtract_messages(None, None, None, None, None, None, 1, None, None, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_decode_messages_subtracted(None, None, 1, 2, None, None, None, None, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()
    for name in ("ft8gpu_subtract_messages", "ft8gpu_decode_messages_subtracted", "ft8gpu_subtract_twiddles"):
        assert name in ft8.ABI_SYMBOLS
    lib.ft8gpu_subtract_twiddles(None)                                   # a NULL table is ignored


def test_kernels_are_listed_without_scratch():
    """tools/kernel_resources.py on subtract.hip alone (tests/test_kernel_resources.py runs it on every source): both kernels are
    there, neither has a scratch segment or a scratch instruction, and the estimate kernel's LDS leaves room for two workgroups
    per CU (160 KB)"""
    import re
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as K
    text = K.assemble(os.path.join(K.CSRC, "subtract.hip"))
    ks = K.kernels_of(text)
    by_name = dict(zip(K.demangle([k["symbol"] for k in ks]), ks))
    for name in ("ft8_subtract_estimate_kernel", "ft8_subtract_apply_kernel"):
        assert name in by_name, sorted(by_name)
        assert by_name[name]["scratch_bytes_per_lane"] == 0
    assert not re.findall(r"^\s*scratch_(load|store)", text, re.M) and K.cmpx_dpp_hazards(text) == []
    assert 2 * by_name["ft8_subtract_estimate_kernel"]["lds_bytes"] <= 160 * 1024
    assert K.waves_per_simd(by_name["ft8_subtract_estimate_kernel"]) >= 2


# ---- (a) the table --------------------------------------------------------------------------------------------------------------------

def test_table_is_the_quarter_step_circle(ft8, oracle):
    w4 = ft8.subtract_twiddles()
    i = np.arange(4096)
    a = 2.0 * np.pi * i / 4096.0
    assert w4.dtype == F32 and w4.shape == (4096, 2)
    assert np.abs(w4[:, 0] - np.cos(a)).max() < 1e-7 and np.abs(w4[:, 1] + np.sin(a)).max() < 1e-7
    assert (w4[:, 0] == np.cos(a).astype(F32)).mean() > 0.99 and (w4[:, 1] == (-np.sin(a)).astype(F32)).mean() > 0.99   # libm against numpy
    assert w4[::4].tobytes() == sr.twiddles(oracle).tobytes()             # w4[4 i] == tw[i]: the refine rule's table is every fourth entry
    assert w4[0].tolist() == [1.0, -0.0] or w4[0].tolist() == [1.0, 0.0]
    assert w4[1024, 1] == -1.0 and w4[2048, 0] == -1.0 and w4[3072, 1] == 1.0
    # the symmetries of the circle hold to an ulp of 1.0 (cos and sin of the double angle are rounded independently)
    k = np.arange(1, 2048)
    assert np.abs(w4[k, 0] - w4[4096 - k, 0]).max() <= 2.0 ** -23 and np.abs(w4[k, 1] + w4[4096 - k, 1]).max() <= 2.0 ** -23
    assert np.abs(w4[k, 0] + w4[k + 2048, 0]).max() <= 2.0 ** -23 and np.abs(w4[k, 1] + w4[k + 2048, 1]).max() <= 2.0 ** -23
    k = np.arange(0, 3072)
    assert np.abs(w4[k, 0] + w4[k + 1024, 1]).max() <= 2.0 ** -23        # the stored -sin a quarter turn on is -cos
    assert np.abs((w4[:, 0].astype(np.float64) ** 2 + w4[:, 1].astype(np.float64) ** 2) - 1.0).max() < 2e-7
    assert (ss.INV[1:] == np.array([F32(1.0 / (32 * n)) for n in range(1, 18)], F32)).all() and ss.INV[17] == F32(1.0 / 544.0)


# ---- (b) the reference phase --------------------------------------------------------------------------------------------------------------

def test_phase_against_python_integers():
    rng = np.random.default_rng(3)
    for k4 in (0, 1, 1286, 4095, -7, 263159, -262140):
        tones = rng.integers(0, 8, 79)
        S = int(rng.integers(-6000, 13000))
        j, th = ss.theta(S, k4, tones)
        big = ss.big_theta(k4, tones)
        # direct: the phase advances by K of the symbol before each sample, counted in unbounded integers from the first sample on
        acc, want = 0, []
        for m in range(79):
            K = k4 + 8 * int(tones[m])
            assert big[m] == acc % 4096 == (512 * m * k4) % 4096       # the closed form the kernels use
            for r in range(512):
                want.append(acc % 4096)
                acc += K
        assert th.reshape(-1).tolist() == want and j.reshape(-1).tolist() == list(range(S, S + 79 * 512))
        assert th.min() >= 0 and th.max() < 4096
        # the same residues from 32-bit wrapping arithmetic, as the device forms them
        m = np.arange(79, dtype=np.uint32)[:, None]
        K32 = (np.uint32(k4 & 0xFFFFFFFF) + np.uint32(8) * tones.astype(np.uint32))[:, None]
        dev = (np.uint32(512) * m * np.uint32(k4 & 0xFFFFFFFF) + K32 * np.arange(512, dtype=np.uint32)[None, :]) & np.uint32(4095)
        assert (dev.astype(np.int64) == th).all()


def test_tones_of_a_record_are_the_encoders(ft8, oracle):
    import refine_craft as rc
    for text in (sc.STRONG_TEXT, sc.WEAK_TEXT, "K1ABC W9XYZ -05"):
        tones, payload = sc.tones_of_text(oracle, text)
        assert (sr.tones_of_a91(rc.a91_of_payload(payload)) == tones).all() and (ft8.encode(ft8.pack77(text)) == tones).all()


# ---- the restatement on the hand-made records ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def constructed(ft8):
    iq, msgs, refined, first, n, where = sc.constructed(ft8)
    fill = np.full((6, 50 * 64), sc.FILL, np.uint8).view(ss.INFO_DTYPE).reshape(6, 50)
    out, info = ss.subtract(iq, msgs, refined, first, n, ss.twiddles(), info=fill)
    return iq, msgs, refined, first, n, where, out, info


def test_constructed_records_are_what_they_are_named_for(constructed):
    iq, msgs, refined, first, n, where, out, info = constructed
    at = lambda name: info[where[name]]
    raw = info.view(np.uint8).reshape(6, 50, 64)
    assert (raw[1] == sc.FILL).all() and (raw[2, 3:] == sc.FILL).all() and (raw[4] == sc.FILL).all()         # outside [first, n_msgs): untouched
    assert (raw[3, :2] == sc.FILL).all() and (raw[3, 5:] == sc.FILL).all() and (raw[5, 3:] == sc.FILL).all()
    assert (raw[0] != sc.FILL).any(axis=1).all()                                                               # -3 and 70 are 0 and 50
    for name, d, t in (("truth_d+2_t+2", 2, 2), ("truth_d-2_t-2", -2, -2), ("truth_d+2_t-2_u1", 2, -2), ("truth_d-2_t+2_u3", -2, 2)):
        r = at(name)
        assert (r["valid"], r["d_best"], r["t_best"], r["k4"], r["s_best"]) == (1, d, t, 4 * 321 + 2, 2576), (name, r)
        assert r["pf"][d + 2] == max(r["pf"]) and r["pt"][t + 2] == max(r["pt"]) and r["pt"][2] == r["pf"][d + 2]   # pt at t = 0 is pf at d*
        assert (r["pad"] == 0).all() and r["pad0"] == 0
    for name in ("not_valid", "not_valid_random"):
        assert at(name).tobytes() == bytes(64)
    for name in ("far_before_the_frame", "far_behind_the_frame", "field_extremes", "zeros_0", "zeros_1", "zeros_2"):
        r = at(name)                                                     # nothing but zeros under every window: every power is +0
        assert r["valid"] == 1 and (r["d_best"], r["t_best"]) == (-2, -2) and r.tobytes()[12:] == bytes(52), name
    edge = [k for k in where if k.startswith("edge_")]
    assert len(edge) == 16 and all(at(k)["valid"] == 1 and at(k)["pf"].max() > 0 for k in edge)   # windows that leave the frame still see samples
    assert {int(refined[where[k]]["e_best"]) for k in edge} == {-16, 0, 16}
    assert at("edge_to-12_fo0_ts0_fs0")["s_best"] < 0 and at("edge_to23_fo248_ts1_fs1")["s_best"] + ss.SPAN > ss.NSAMPLES
    # frames without records to subtract come back bit for bit; so does everything outside the records of frame 3
    for f in (1, 2, 4):
        assert out[f].tobytes() == iq[f].tobytes()
    for f, recs in ((3, (2, 3, 4)), (5, (0, 1, 2))):
        lo = min(int(info[f, i]["s_best"]) for i in recs)
        hi = max(int(info[f, i]["s_best"]) for i in recs) + ss.SPAN
        assert 2576 - 48 <= lo <= 2576 and hi <= 2576 + 48 + ss.SPAN
        assert out[f, :, :lo].tobytes() == iq[f, :, :lo].tobytes() and out[f, :, hi:].tobytes() == iq[f, :, hi:].tobytes()
        assert (out[f, :, lo + 96:hi - 96] != iq[f, :, lo + 96:hi - 96]).mean() > 0.99


def test_samples_outside_every_record_are_untouched_and_the_order_matters(constructed):
    iq, msgs, refined, first, n, where, out, info = constructed
    w4 = ss.twiddles()
    f = 5                                                                # three records that overlap on the same samples
    fwd, _ = ss.subtract(iq[f:f + 1], msgs[f:f + 1], refined[f:f + 1], [0], [3], w4)
    rev, _ = ss.subtract(iq[f:f + 1], msgs[f:f + 1], refined[f:f + 1], [0], [3], w4, order=lambda r: r[::-1])
    assert fwd.tobytes() == out[f:f + 1].tobytes()
    lo, hi = 2576 - 48, 2576 + 48 + ss.SPAN
    assert rev[0, :, :lo].tobytes() == iq[f, :, :lo].tobytes() and rev[0, :, hi:].tobytes() == iq[f, :, hi:].tobytes()
    differ = (fwd[0, :, lo:hi] != rev[0, :, lo:hi]).sum()
    assert differ > 0                                                    # float subtraction does not commute: the rule fixes the order
    assert np.abs(fwd - rev).max() < 1e-6                                # ... and the two orders differ in the last bits only
    # two overlapping records, estimated from the input frame: the second is not estimated from what the first left
    two, info2 = ss.subtract(iq[f:f + 1], msgs[f:f + 1], refined[f:f + 1], [0], [2], w4)
    one, info1 = ss.subtract(iq[f:f + 1], msgs[f:f + 1], refined[f:f + 1], [1], [2], w4)
    assert info2[0, 1].tobytes() == info1[0, 1].tobytes()


# ---- suppression against the synthesiser's own waveform -----------------------------------------------------------------------------------

def test_suppression_of_a_known_waveform(oracle, ft8):
    """Single-signal frames from ft8o_synth_cpfsk with off-grid f0 and start, decoded by the oracle, refined and subtracted by
    the restatements: |x' - (x - s)|^2 / |s|^2 in dB, where s is the synthesiser's own noiseless waveform (nothing cancels better
    than subtracting the truth).  tools/subtract_accuracy.py runs 64 frames per set and writes profiles/subtract_accuracy.json;
    here 16 frames of other seeds.  The noiseless worst case must stay within 3 dB of the committed one (the margin covers
    seeds), and below the -19 dB that the 3.125 Hz grid alone could give (sinc of 0.27: a quarter of a cycle per symbol).
    With noise the amplitude estimate carries the noise of 17 segments, 544 samples: at -18 dB in 2500 Hz that alone is
    1 / (544 * 0.0124) = -8.3 dB, so those sets are reported and bounded loosely, not compared with the noiseless one."""
    with open(os.path.join(ROOT, "profiles", "subtract_accuracy.json")) as f:
        committed = {r["set"]: r for r in json.load(f)["sets"]}
    got = {}
    for name, snr, seed in (("noiseless", None, 20261101), ("0dB", 0.0, 20261102), ("-18dB", -18.0, 20261103)):
        iq, s, _f0, _start = sc.suppression_frames(oracle, 16, snr, seed)
        db = sc.suppression_db(oracle, iq, s)
        got[name] = {"decoded": len(db), "median_db": round(float(np.median(db)), 2), "worst_db": round(float(db.max()), 2)}
    print(json.dumps(got))
    assert got["noiseless"]["decoded"] == 16 and got["0dB"]["decoded"] == 16 and got["-18dB"]["decoded"] >= 4
    assert got["noiseless"]["worst_db"] <= committed["noiseless"]["worst_db"] + 3.0
    assert got["noiseless"]["worst_db"] < -19.0 and committed["noiseless"]["worst_db"] < -19.0
    assert got["0dB"]["worst_db"] < -19.0                                # noise of 544 samples at 0 dB: 1 / (544 * 0.78) = -26 dB
    assert got["-18dB"]["worst_db"] < -5.0                               # -8.3 dB of estimate noise, with 3 dB for the spread


# ---- uncovering ------------------------------------------------------------------------------------------------------------------------------

def test_subtraction_uncovers_what_masking_does_not(oracle, ft8):
    """two-signal frames, the weak one 3 to 9 Hz and a few symbols away from one 15 to 20 dB stronger: on every committed seed
    pass 1 decodes the strong signal only, the restated subtraction path decodes the weak one in pass 2, and masking
    (ft8_spec_multipass.decode_passes at 2 passes) does not"""
    assert len(sc.UNCOVER_SEEDS) >= 8
    iq = np.stack([sc.uncover_frame(oracle, s) for s in sc.UNCOVER_SEEDS])
    facts, (msgs, n, nbp, res) = sc.uncover_facts(oracle, iq)
    for seed, (strong_only, weak_by_subtraction, not_by_masking) in zip(sc.UNCOVER_SEEDS, facts):
        assert strong_only, seed
        assert weak_by_subtraction, seed
        assert not_by_masking, seed
    assert (nbp[:, 0] == 1).all() and (nbp[:, 1] == 2).all() and (n == 2).all()
    # the residual has lost the strong signal, which carries 40 % and more of these frames' power
    power = lambda a: float((a.astype(np.float64) ** 2).sum())
    assert all(power(res[f]) < 0.9 * power(iq[f]) for f in range(len(n)))
