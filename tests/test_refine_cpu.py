"""CPU tests of the refined time and frequency (include/ft8gpu.h "refined time and frequency"): the record layout against gcc,
the host helper ft8gpu_refined_estimate and the table against the restatement tests/ft8_spec_refine.py on hand-made powers, the
restatement's tones against the encoder, its properties on the constructed records of tests/refine_craft.py (which the device
is held to in tests/test_gpu_refine.py), and the accuracy of the rule against known truth.  No GPU is used here."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ft8_spec_refine as sr
import refine_craft as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc"), "-j8"])
    m.load_library()
    return m


# ---- (b) ABI ------------------------------------------------------------------------------------------------------------------------

def test_record_layout_against_gcc(ft8, tmp_path):
    fields = ("e_best", "valid", "pad0", "pt", "pf", "noise", "pad")
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ft8gpu.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(ft8gpu_refined));']
    lines += [f'printf("{f} %zu\\n", offsetof(ft8gpu_refined, {f}));' for f in fields]
    lines += ['printf("consts %d %d %d\\n", FT8GPU_REFINE_LEAD, FT8GPU_REFINE_STEP, FT8GPU_REFINE_RANGE);', 'return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=gnu17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    want = {"size": "48", "e_best": "0", "valid": "2", "pad0": "3", "pt": "4", "pf": "16", "noise": "36", "pad": "40",
            "consts": f"{sr.LEAD} {sr.STEP} {sr.RANGE}"}
    assert got == want
    for dt in (ft8.REFINED_DTYPE, sr.REFINED_DTYPE):
        assert dt.itemsize == 48 and [dt.fields[f][1] for f in fields] == [int(want[f]) for f in fields]
    assert ft8.REFINED_DTYPE == sr.REFINED_DTYPE and (sr.LEAD, sr.STEP, sr.RANGE) == (256, 32, 16)


# ---- (a) the host helper against numpy ------------------------------------------------------------------------------------------------

def _pair(ft8, to, ts, fo, fs, e_best, pt, pf, noise, valid=1):
    m = np.zeros(1, ft8.MESSAGE_DTYPE)
    m["cand"]["time_offset"], m["cand"]["time_sub"], m["cand"]["freq_offset"], m["cand"]["freq_sub"] = to, ts, fo, fs
    m["text"], m["snr_db"], m["dt_s"], m["freq_hz"] = b"CQ K1ABC FN42", -7, 0.08 * (2 * to + ts), 3.125 * (2 * fo + fs)
    r = np.zeros(1, sr.REFINED_DTYPE)
    r["e_best"], r["valid"], r["pt"], r["pf"], r["noise"] = e_best, valid, pt, pf, noise
    return m, r


HAND_MADE = {
    # name: (to, ts, fo, fs, e_best, pt, pf, noise)
    "plain": (5, 1, 160, 0, 3, (80.0, 100.0, 90.0), (10.0, 60.0, 100.0, 70.0, 12.0), 2.0),
    "equal_neighbours": (5, 0, 160, 1, -2, (90.0, 100.0, 90.0), (1.0, 50.0, 100.0, 50.0, 1.0), 1.0),
    "all_equal": (0, 0, 10, 0, 0, (7.0, 7.0, 7.0), (7.0, 7.0, 7.0, 7.0, 7.0), 7.0),
    "clamp": (2, 1, 30, 1, 0, (101.0, 100.0, 0.0), (0.0, 0.0, 100.0, 99.9999, 0.0), 3.0),        # no device output: pt[1] is a maximum there
    "no_maximum": (2, 0, 30, 0, 1, (100.0, 50.0, 100.0), (0.0, 100.0, 50.0, 100.0, 0.0), 3.0),
    "edge_low_neighbour_is_the_zero": (-12, 0, 0, 0, -16, (0.0, 100.0, 99.0), (1.0, 20.0, 100.0, 30.0, 1.0), 0.5),
    "edge_high_neighbour_is_the_zero": (23, 1, 248, 1, 16, (99.0, 100.0, 0.0), (1.0, 30.0, 100.0, 20.0, 1.0), 0.5),
    "peak_one_bin_down": (4, 0, 100, 0, 0, (50.0, 100.0, 50.0), (60.0, 100.0, 70.0, 10.0, 1.0), 2.0),
    "peak_one_bin_up": (4, 0, 100, 0, 0, (50.0, 100.0, 50.0), (1.0, 10.0, 70.0, 100.0, 90.0), 2.0),
    "tie_takes_the_first": (4, 0, 100, 0, 0, (50.0, 100.0, 50.0), (1.0, 100.0, 100.0, 100.0, 1.0), 2.0),
    "noise_above_signal": (4, 0, 100, 0, 0, (50.0, 100.0, 50.0), (1.0, 10.0, 100.0, 10.0, 1.0), 150.0),
    "noise_equals_signal": (4, 0, 100, 0, 0, (50.0, 100.0, 50.0), (1.0, 10.0, 100.0, 10.0, 1.0), 100.0),
    "noise_zero_signal_positive": (4, 0, 100, 0, 0, (50.0, 100.0, 50.0), (1.0, 10.0, 100.0, 10.0, 1.0), 0.0),
    "all_zero": (4, 0, 100, 0, -16, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0, 0.0), 0.0),
    "snr_ceiling": (4, 0, 100, 0, 0, (50.0, 1e30, 50.0), (1.0, 10.0, 1e30, 10.0, 1.0), 1e-3),
    "not_finite": (4, 0, 100, 0, 0, (np.inf, np.inf, 1.0), (np.nan, 1.0, np.inf, 1.0, 1.0), np.nan),
}


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_host_helper_equals_the_restatement(ft8, name):
    m, r = _pair(ft8, *HAND_MADE[name])
    dt, hz, snr, ok = ft8.refined_estimate(m, r)
    want = sr.estimate(m[0]["cand"], r[0])
    assert ok[0]
    got = np.array([dt[0], hz[0], snr[0]], F32)
    # both sides evaluate the same double expressions; log10 may differ in the last place of a double before the cast to float
    assert np.allclose(got, np.array(want, F32), rtol=3e-7, atol=0.0), (name, got, want)
    assert -30.0 <= snr[0] <= 49.0 and np.isfinite(got).all()


def test_host_helper_values_by_hand(ft8):
    """figures worked out on paper, not by the restatement"""
    est = lambda name: [float(v[0]) for v in ft8.refined_estimate(*_pair(ft8, *HAND_MADE[name]))[:3]]
    dt, hz, snr = est("equal_neighbours")                                 # vertex 0 in time and frequency
    assert dt == pytest.approx((256 * 10 + 256 + 32 * -2) / 3200.0, abs=1e-6) and hz == pytest.approx(3.125 * 321, abs=1e-4)
    assert snr == pytest.approx(10 * np.log10(99.0 * 6.25 / 2500.0), abs=1e-4)
    dt, hz, snr = est("plain")                                            # vertex 0.5 * (80 - 90) / (80 - 200 + 90) = 1 / 6
    assert dt == pytest.approx((256 * 11 + 256 + 32 * (3 + 1 / 6)) / 3200.0, abs=1e-6)
    assert hz == pytest.approx(3.125 * (320 + 0.5 * (60 - 70) / (60 - 200 + 70)), abs=1e-4)
    dt, hz, snr = est("clamp")                                            # the time vertex past half a step, the frequency's just short of it
    assert dt == pytest.approx((256 * 5 + 256 - 16) / 3200.0, abs=1e-6) and hz == pytest.approx(3.125 * 61.5, abs=1e-4)
    dt, hz, snr = est("edge_low_neighbour_is_the_zero")                   # no interpolation against the out-of-range zero
    assert dt == pytest.approx((256 * -24 + 256 - 512) / 3200.0, abs=1e-6)
    dt, hz, snr = est("edge_high_neighbour_is_the_zero")
    assert dt == pytest.approx((256 * 47 + 256 + 512) / 3200.0, abs=1e-6)
    assert est("peak_one_bin_down")[1] == pytest.approx(3.125 * (200 - 1 + 0.5 * (60 - 70) / (60 - 200 + 70)), abs=1e-4)
    assert est("tie_takes_the_first")[1] == pytest.approx(3.125 * 199.5, abs=1e-4)   # u* = -1, vertex of (1, 100, 100) = 0.5
    assert est("noise_above_signal")[2] == -30.0 and est("noise_equals_signal")[2] == -30.0 and est("all_zero")[2] == -30.0
    assert est("noise_zero_signal_positive")[2] == 49.0 and est("snr_ceiling")[2] == 49.0
    m, r = _pair(ft8, *HAND_MADE["plain"], valid=0)                       # not written yet: refused, outputs untouched
    assert not ft8.refined_estimate(m, r)[3][0] and sr.estimate(m[0]["cand"], r[0]) is None
    lib = ft8.load_library()
    assert lib.ft8gpu_refined_estimate(None, None, None, None, None) == -1


def test_table_formatter(ft8):
    ms, rs = zip(*[_pair(ft8, *HAND_MADE[k]) for k in ("plain", "equal_neighbours")])
    m, r = np.concatenate(ms + (_pair(ft8, *HAND_MADE["plain"], valid=0)[0],)), np.concatenate(rs + (np.zeros(1, sr.REFINED_DTYPE),))
    text = ft8.format_messages_refined(m, r, 3)
    want = []
    for k in range(2):
        dt, hz, snr = sr.estimate(m[k]["cand"], r[k])
        want.append("%3d %5.2f %6.1f ~  CQ K1ABC FN42\n" % (int(np.rint(snr)), dt, hz))
    want.append("%3d %5.2f %6.1f ~  CQ K1ABC FN42\n" % (-7, m[2]["dt_s"], m[2]["freq_hz"]))      # valid == 0: the record's own values
    assert text == "".join(want) and text.splitlines()[0] == " -9  0.99 1000.2 ~  CQ K1ABC FN42"
    lib = ft8.load_library()
    buf = C.create_string_buffer(20)
    assert lib.ft8gpu_format_messages_refined(m.ctypes.data, r.ctypes.data, 3, buf, 20) == len(text) and buf.value.decode() == text[:19]
    assert lib.ft8gpu_format_messages_refined(None, None, 2, None, 0) == -1
    assert lib.ft8gpu_format_messages_refined(m.ctypes.data, r.ctypes.data, 0, buf, 20) == 0 and buf.value == b""


def test_entries_refuse_bad_arguments_before_touching_a_gpu(ft8):
    lib = ft8.load_library()
    assert lib.ft8gpu_refine_messages(None, None, None, None, 1, None, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_decode_messages_refined(None, None, 1, None, None, None, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()


def test_host_helpers_under_asan_ubsan(tmp_path):
    """a program of its own (tests/host_asan/refine_asan_main.c) linked with csrc/ft8_refine.c; nothing is loaded into python"""
    exe = str(tmp_path / "refine_asan")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_asan", "refine_asan_main.c"),
                           os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc", "ft8_refine.c"), "-lm", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "refine_asan ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------

def test_tones_of_a_record_are_the_encoders(ft8, oracle):
    rng = np.random.default_rng(5)
    for text in ("CQ K1ABC FN42", "K1ABC W9XYZ -05", "W9XYZ K1ABC RR73", "TNX BOB 73 GL"):
        payload = ft8.pack77(text)
        assert (sr.tones_of_a91(rc.a91_of_payload(payload)) == ft8.encode(payload)).all(), text
    for _ in range(8):
        payload = rng.integers(0, 256, 10, dtype=np.uint8)
        payload[9] &= 0xF8
        assert (sr.tones_of_a91(rc.a91_of_payload(payload)) == oracle.encode(payload)).all()
    tw = sr.twiddles(oracle)
    i = np.arange(1024)
    assert tw.dtype == F32 and np.abs(tw[:, 0] - np.cos(2 * np.pi * i / 1024)).max() < 1e-7
    assert np.abs(tw[:, 1] + np.sin(2 * np.pi * i / 1024)).max() < 1e-7


@pytest.fixture(scope="module")
def constructed(ft8, oracle):
    iq, msgs, n, where = rc.constructed(ft8)
    ref = sr.refine(iq, msgs, n, sr.twiddles(oracle), refined=np.full((3, 50 * 48), rc.FILL, np.uint8).view(sr.REFINED_DTYPE))
    return iq, msgs, n, where, ref


def test_constructed_records_are_what_they_are_named_for(ft8, constructed):
    iq, msgs, n, where, ref = constructed
    at = lambda name: ref[where[name]]
    assert list(n) == [50, 0, 3] and len([k for k in where if where[k][0] == 0]) == 50
    assert (ref[1].view(np.uint8) == rc.FILL).all() and (ref[2, 3:].view(np.uint8) == rc.FILL).all()     # behind the counts: untouched
    assert (ref[0]["valid"] == 1).all() and (ref[0]["pad0"] == 0).all() and (ref[0]["pad"] == 0).all()
    r = at("truth_at_plus16")
    assert r["e_best"] == 16 and r["pt"][2] == 0.0 and r["pt"][0] > 0 and r["pt"][1] > r["pt"][0] and r["pf"][2] == r["pt"][1]
    r = at("truth_at_minus16")
    assert r["e_best"] == -16 and r["pt"][0] == 0.0 and r["pt"][2] > 0 and r["pt"][1] > r["pt"][2]
    r = at("truth_at_0")
    assert r["e_best"] == 0 and r["pf"][2] == max(r["pf"]) and r["noise"] < 0.01 * r["pf"][2]
    assert at("truth_at_plus16")["pt"][1] == at("truth_at_0")["pt"][1] == at("truth_at_minus16")["pt"][1]  # the same samples and phases
    r = at("truth_one_bin_up")
    assert r["pf"][1] == max(r["pf"])                                     # the signal is one step below this record's cell
    dt, hz, snr, ok = ft8.refined_estimate(msgs[0, :50], ref[0, :50])
    assert abs(hz[where["truth_one_bin_up"][1]] - 3.125 * 321) < 0.3
    for name in ("truth_at_plus16", "truth_at_minus16", "truth_at_0"):
        k = where[name][1]
        assert abs(dt[k] * 3200 - (256 * 9 + 256)) < 2.0 and abs(hz[k] - 3.125 * 321) < 0.1, name
    for name in ("far_before_the_frame", "far_behind_the_frame", "zeros_0", "zeros_1", "zeros_2"):
        r = at(name)                                                     # nothing but zeros under every window: every power is +0
        assert r["e_best"] == -16 and r["valid"] == 1 and r.tobytes()[4:] == bytes(44), name
    edge = [k for k in where if k.startswith("edge_")]
    assert len(edge) == 16 and all(at(k)["pt"][1] > 0 for k in edge)      # windows that leave the frame still see samples
    assert at("field_extremes")["valid"] == 1


# ---- (c) accuracy against known truth ---------------------------------------------------------------------------------------------------

def test_refined_values_beat_the_grid_on_known_truth(oracle, ft8):
    """Single-signal frames from ft8o_synth_cpfsk at a strong level and near BP's threshold, f0 and the start sample uniform
    off the grid, decoded by the oracle, refined by the restatement and the host helper.  On the strong set the median and the
    90th percentile of the refined errors must be strictly below the coarse ones.  The coarse errors are a uniform grid's:
    a median of about 0.78 Hz and, once dt_s is moved from the row's first sample to the symbol's start (+ 256 samples),
    about 64 samples.  tools/refine_accuracy.py runs the same on more frames and writes profiles/refine_accuracy.json."""
    iq, f0, start, text = rc.accuracy_frames(oracle, 32, rc.STRONG_DB, 20261019)
    strong = rc.summary(rc.accuracy(oracle, iq, f0, start, text))
    iq, f0, start, text = rc.accuracy_frames(oracle, 32, rc.WEAK_DB, 20261020)
    weak = rc.summary(rc.accuracy(oracle, iq, f0, start, text))
    print(json.dumps({"strong": strong, "weak": weak}))
    assert strong["decoded"] == 32 and weak["decoded"] >= 8
    for q in ("median", "p90"):
        assert strong["refined_hz"][q] < strong["coarse_hz"][q]
        assert strong["refined_samples"][q] < strong["coarse_samples"][q] < strong["coarse_raw_samples"][q]
    assert 0.5 < strong["coarse_hz"]["median"] < 1.1 and 30 < strong["coarse_samples"]["median"] < 100   # the grid's own error (+-3 sd of a median of 32)
