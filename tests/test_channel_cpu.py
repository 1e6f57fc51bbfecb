"""The fading channel without a GPU (include/ft8gpu.h "Fading channel"): the committed quantiles against the standard library, the
library's taps and its plain-C rule against the numpy restatement (tests/ft8_spec_channel.py) byte for byte, the struct and the
presets as the C compiler sees them, the entries' refusals (which need no context), the statistics of the rule's float64 model,
the example's compile check, the measurement tool's CPU mode, and the host code under AddressSanitizer / UBSan as a program of its
own."""
import json
import os
import re
import subprocess
import sys
from statistics import NormalDist

import numpy as np
import pytest

import ft8_spec_channel as sc
import ft8_spec_gfsk as sg
import gfsk_craft as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ("ft8gpu_channel_taps", "ft8gpu_channel_check", "ft8gpu_channel_clip", "ft8gpu_synth_gfsk_frames_faded",
               "ft8gpu_synth_gfsk_audio_faded")


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as ft8
    ft8.load_library()
    return ft8


def header_text():
    return open(os.path.join(ROOT, "include", "ft8gpu.h")).read()


# ---- constants and layout ------------------------------------------------------------------------------------------------------------

def test_quantiles_are_the_standard_librarys_to_the_digits_committed(ft8):
    m = re.search(r"#define FT8GPU_CHANNEL_QUANTILES \{(.*?)\}", header_text(), re.S)
    lits = [x.strip() for x in m.group(1).replace("\\", " ").split(",")]
    assert len(lits) == 16
    for k, lit in enumerate(lits):
        want = NormalDist().inv_cdf((k + 0.5) / 16)
        assert lit == f"{want:.15f}", (k, lit, want)
        assert float(lit) == sc.QUANTILES[k] == -sc.QUANTILES[15 - k]
    for name in NEW_SYMBOLS:
        assert name in ft8.ABI_SYMBOLS and name + "(" in header_text()
    assert (ft8.CHANNEL_TAPS, ft8.CHANNEL_GRID, ft8.CHANNEL_NONE, ft8.CHANNEL_FADED) == (sc.TAPS, sc.GRID, sc.NONE, sc.FADED)
    assert sc.GRID == 79 * 512 // sc.STEP[sg.IQ] + 1 == 79 * 1920 // sc.STEP[sg.AUDIO] + 1
    assert 3200 // sc.STEP[sg.IQ] == 12000 // sc.STEP[sg.AUDIO] == 100


def test_struct_layout_and_presets_as_the_c_compiler_sees_them(ft8, tmp_path):
    d = ft8.CHANNEL_DTYPE
    assert d == sc.CHANNEL_DTYPE and d.itemsize == 16
    assert [d.fields[k][1] for k in ("spread_hz", "delay_ms", "path2_gain", "mode")] == [0, 4, 8, 12]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "ft8gpu.h"
int main(void) {
    const ft8gpu_channel p[4] = { FT8GPU_CHANNEL_QUIET, FT8GPU_CHANNEL_MODERATE, FT8GPU_CHANNEL_DISTURBED, FT8GPU_CHANNEL_FLUTTER };
    printf("%zu %zu %zu %zu %zu\n", sizeof(ft8gpu_channel), offsetof(ft8gpu_channel, spread_hz), offsetof(ft8gpu_channel, delay_ms),
           offsetof(ft8gpu_channel, path2_gain), offsetof(ft8gpu_channel, mode));
    for (int k = 0; k < 4; k++) printf("%.9g %.9g %.9g %u\n", p[k].spread_hz, p[k].delay_ms, p[k].path2_gain, p[k].mode);
    return 0;
}'''
    src, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-std=gnu17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    lines = subprocess.check_output([exe]).decode().splitlines()
    assert lines[0].split() == ["16", "0", "4", "8", "12"]
    for line, name in zip(lines[1:], ("quiet", "moderate", "disturbed", "flutter")):
        got = tuple(float(F(x)) for x in line.split())                     # %.9g gives a float back exactly
        want = tuple(float(F(x)) for x in sc.PRESETS[name])
        assert got == want == tuple(float(F(x)) for x in ft8.CHANNEL_PRESETS[name]), name
        rec = ft8.channel_preset(name, (2,))
        assert rec.dtype == d and tuple(float(x) for x in rec[1].tolist()) == want


# ---- taps ------------------------------------------------------------------------------------------------------------------------------

def test_taps_agree_with_the_restatement_on_a_sweep(ft8):
    keys = [(0, 0, 0, 0), (1, 2, 3, 1), (2 ** 64 - 1, 2 ** 40 + 7, 63, 1), (0xDEADBEEF, 4095, 17, 0), (9, 2 ** 52, 0, 1)]
    seen = set()
    for seed, clip, signal, path in keys:
        for spread in (0.0, 0.1, 0.5, 1.0, 3.3333, 10.0, 20.0):
            gstep, theta = ft8.channel_taps(seed, clip, signal, path, spread)
            wg, wt = sc.taps(seed, clip, signal, path, spread)
            assert gstep.tobytes() == wg.tobytes() and theta.tobytes() == wt.tobytes(), (seed, clip, signal, path, spread)
            if spread == 0.0:
                assert not gstep.any()
            else:
                assert (gstep[:8] > 2 ** 31).all() and (gstep[8:] < 2 ** 31).all()        # negative frequencies wrap
                assert ((gstep[:8].astype(np.int64) + gstep[:7:-1].astype(np.int64)) % 2 ** 32 == 0).all()
            seen.add(theta.tobytes())
    assert len(seen) == len(keys)                                           # the phases depend on the key, not on the spread
    g20 = sc.taps(0, 0, 0, 0, 20.0)[0]
    assert int(g20[15]) == round(10.0 * sc.QUANTILES[15] / 100.0 * 2 ** 32)   # 18.6 Hz: 0.186 turn per grid step
    lib = ft8.load_library()
    buf = np.full(16, 0xA5A5A5A5, np.uint32)
    for spread, path in ((-0.1, 0), (20.5, 0), (np.nan, 0), (np.inf, 1), (1.0, 2)):
        assert lib.ft8gpu_channel_taps(1, 1, 1, path, spread, buf.ctypes.data, buf.ctypes.data) == -1
    assert (buf == 0xA5A5A5A5).all()
    assert lib.ft8gpu_channel_taps(1, 1, 1, 0, 1.0, None, None) == 0        # NULL outputs are left out
    only = np.zeros(16, np.uint32)
    assert lib.ft8gpu_channel_taps(1, 2, 3, 1, 1.0, None, only.ctypes.data) == 0 and only.tobytes() == sc.taps(1, 2, 3, 1, 1.0)[1].tobytes()


def test_path_amplitudes_and_delays():
    for g2 in (0.0, 0.5, 1.0, 4.0):
        w0, w1 = sc.path_amplitudes(g2)
        assert w0.dtype == F and abs(float(w0) ** 2 + float(w1) ** 2 - 1.0) < 3e-7
    assert sc.path_amplitudes(0.0) == (F(1.0), F(0.0))
    assert [sc.delay_of(d, sg.IQ) for d in (0.0, 0.5, 1.0, 2.0, 10.0)] == [0, 2, 3, 6, 32]      # 1.6 -> 2, 3.2 -> 3, 6.4 -> 6
    assert [sc.delay_of(d, sg.AUDIO) for d in (0.0, 0.5, 1.0, 2.0, 10.0)] == [0, 6, 12, 24, 120]


# ---- the plain-C rule against the restatement ------------------------------------------------------------------------------------------

def small_clip():
    """four signals: unfaded, one path block-faded, two paths with a delay past the clip's end, and fast fading before sample 0"""
    sigs = [(gc.random_tones(1), 700.0, 0.5, 1.0), (gc.random_tones(2), 1212.5, 1.0, 0.5), (gc.random_tones(3), 2000.3, 2.36, 0.7),
            (gc.random_tones(4), 433.1, -0.5, 2.0)]
    chs = [(0.0, 0.0, 0.0, sc.NONE), (0.0, 3.0, 0.0, sc.FADED), (1.0, 10.0, 1.0, sc.FADED), (20.0, 0.5, 4.0, sc.FADED)]
    return sigs, chs


@pytest.mark.parametrize("mode,nsamples", [(sg.IQ, None), (sg.AUDIO, 180000), (sg.AUDIO, 20011)])
def test_host_mirror_is_the_restatement_byte_for_byte(ft8, mode, nsamples):
    sigs, chs = small_clip()
    recs, crec = gc.records([sigs])[0], sc.channel_records([chs])[0]
    for seed, clip in ((0, 0), (77, 123456789)):
        want = sc.clip(sigs, chs, mode, nsamples, seed, clip)
        got = ft8.channel_clip(mode, recs, crec, nsamples or 1, seed, clip)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (mode, nsamples, seed, clip)
    assert want.any() and not np.isnan(want).any()
    unfaded = sg.clip(sigs, mode, nsamples)
    assert ft8.channel_clip(mode, recs, None, nsamples or 1).tobytes() == unfaded.tobytes()
    none = sc.channel_records([[(5.0, 5.0, 1.0, sc.NONE)] * 4])[0]
    assert ft8.channel_clip(mode, recs, none, nsamples or 1, 9, 9).tobytes() == unfaded.tobytes()
    assert sc.clip(sigs, [(np.nan, -1.0, 99.0, sc.NONE)] * 4, mode, nsamples).tobytes() == unfaded.tobytes()
    assert want.tobytes() != unfaded.tobytes() and want.tobytes() != sc.clip(sigs, chs, mode, nsamples, 77, 123456790).tobytes()


def test_block_fading_is_one_constant_gain_and_the_interpolation_meets_the_grid():
    gstep, theta = sc.taps(3, 4, 5, 0, 0.0)
    G = sc.grid(gstep, theta, F(1.0))
    assert (G == G[0]).all() and G[0].any()
    gstep, theta = sc.taps(3, 4, 5, 0, 20.0)
    G = sc.grid(gstep, theta, F(0.5))
    for mode in (sg.IQ, sg.AUDIO):
        g = sc.gain(G, mode)
        S = sc.STEP[mode]
        assert np.array_equal(g[:, ::S].T, G[:-1])                          # t = 0 at a grid point: G[j] + d * 0
        mid = g[:, S // 2::S].T.astype(np.float64)
        assert np.abs(mid - 0.5 * (G[:-1].astype(np.float64) + G[1:])).max() < 1e-6
    g64 = sc.gain64(3, 4, 5, 0, 20.0, np.arange(sc.GRID) / 100.0) * 0.5
    err = np.abs((G[:, 0] + 1j * G[:, 1]) - g64).max()
    print(f"grid values against the float64 model at 20 Hz: worst error {err:.2e}")
    assert err < 2e-6                                                       # 16 terms of 2^-24 turn phase truncation and float rounding


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------

REFUSALS = [
    (dict(spread_hz=np.nan), "spread_hz nan out of range [0, 20] or not finite"),
    (dict(spread_hz=-0.5), "spread_hz -0.5 out of range [0, 20]"),
    (dict(spread_hz=20.5), "spread_hz 20.5 out of range [0, 20]"),
    (dict(delay_ms=np.inf), "delay_ms inf out of range [0, 10] or not finite"),
    (dict(delay_ms=-1.0), "delay_ms -1 out of range [0, 10]"),
    (dict(delay_ms=10.5), "delay_ms 10.5 out of range [0, 10]"),
    (dict(path2_gain=np.nan), "path2_gain nan out of range [0, 4] or not finite"),
    (dict(path2_gain=4.5), "path2_gain 4.5 out of range [0, 4]"),
    (dict(path2_gain=-1.0), "path2_gain -1 out of range [0, 4]"),
    (dict(mode=2), "unknown mode 2"),
    (dict(mode=2, spread_hz=np.nan), "unknown mode 2"),
]


@pytest.mark.parametrize("which", ["frames", "audio"])
@pytest.mark.parametrize("kw,says", REFUSALS, ids=[s[:22] for _, s in REFUSALS])
def test_entries_refuse_a_bad_channel_before_the_context_is_looked_at(ft8, which, kw, says):
    lib = ft8.load_library()
    sig = np.zeros((1, 2), gc.SIGNAL_DTYPE)
    sig["f0_hz"], sig["t0_s"], sig["amplitude"] = 1000.0, 0.5, 1.0
    ch = ft8.channel_preset("moderate", (1, 2))
    for k, v in kw.items():
        ch[k][0, 1] = v
    out = np.full(2 * 48000, 0x5A5A5A5A, np.uint32)
    if which == "frames":
        rc = lib.ft8gpu_synth_gfsk_frames_faded(None, sig.ctypes.data, ch.ctypes.data, 1, 2, 0.0, 1, 0, 0.0, out.ctypes.data, 0)
    else:
        rc = lib.ft8gpu_synth_gfsk_audio_faded(None, sig.ctypes.data, ch.ctypes.data, 1, 2, 64, 0.0, 1, 0, 0.0, 1, out.ctypes.data, 0)
    err = lib.ft8gpu_last_error().decode()
    print(err)
    assert rc == -1 and says in err and "signal 1 of clip 0" in err and (out == 0x5A5A5A5A).all()
    assert lib.ft8gpu_channel_check(ch[0, 1:].ctypes.data) in (1, 2, 3, 4) and lib.ft8gpu_channel_check(ch[0, :1].ctypes.data) == 0


def test_entries_take_good_channels_up_to_the_context_and_keep_the_unfaded_refusals(ft8):
    lib = ft8.load_library()
    sig = np.zeros((1, 1), gc.SIGNAL_DTYPE)
    sig["f0_hz"], sig["t0_s"], sig["amplitude"] = 1000.0, 0.5, 1.0
    out = np.full(2 * 48000, 0x5A5A5A5A, np.uint32)
    edge = sc.channel_records([[(20.0, 10.0, 4.0, sc.FADED)]])
    ignored = sc.channel_records([[(np.nan, -1.0, 99.0, sc.NONE)]])         # mode 0: the other fields are not looked at
    for ch in (edge, ignored, None):
        cp = None if ch is None else ch.ctypes.data
        assert lib.ft8gpu_synth_gfsk_frames_faded(None, sig.ctypes.data, cp, 1, 1, 0.0, 1, 0, 0.0, out.ctypes.data, 0) == -1
        assert b"ctx is NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_channel_check(None) == 4
    bad = sig.copy()
    bad["f0_hz"] = 12000.0
    assert lib.ft8gpu_synth_gfsk_audio_faded(None, bad.ctypes.data, edge.ctypes.data, 1, 1, 64, 0.0, 1, 0, 0.0, 1, out.ctypes.data, 0) == -1
    assert b"out of range [0, 12000)" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_synth_gfsk_audio_faded(None, sig.ctypes.data, edge.ctypes.data, 1, 65, 64, 0.0, 1, 0, 0.0, 1, out.ctypes.data, 0) == -1
    assert b"nsig 65" in lib.ft8gpu_last_error()
    assert (out == 0x5A5A5A5A).all()
    with pytest.raises(ft8.Ft8GpuError):
        ft8.channel_clip(sg.IQ, sig[0], sc.channel_records([[(21.0, 0.0, 0.0, sc.FADED)]])[0])


# ---- statistics of the model ---------------------------------------------------------------------------------------------------------------

def test_model_has_unit_mean_power_and_the_gaussian_spectrums_autocorrelation():
    """The float64 restatement gain64 at spread 1 Hz over the seeds 0 .. 3999, one (clip, signal, path) each.
    Mean power: |G|^2 at one time is close to exponentially distributed, so the mean over 4000 seeds has a standard deviation
    near 1 / sqrt(4000) = 0.016; measured here 0.9941 at t = 0 and 0.9904 at t = 6.32 s; the margin is 0.08 (5 sigma).
    Autocorrelation: E[G(t) conj G(t + tau)] = (1 / 16) sum_m exp(-2 pi i f_m tau) exactly, since the phases are independent and
    uniform; against exp(-2 (pi (spread / 2) tau)^2) at tau = 0.1, 0.2, 0.4, 0.6 s that sum differs by 0.0035, 0.0097, 0.0021 and
    0.0275 (the sixteen quantiles stand for the Gaussian up to about one period of the outermost tap, 1 / 0.93 Hz), and the estimate
    over the 4000 seeds by 0.0099, 0.0146, 0.0083 and 0.0465 (its own standard deviation is below 0.016).  Margins: 0.04 for the
    exact sum, 0.04 + 5 * 0.016 = 0.12 for the estimate."""
    spread, nseeds = 1.0, 4000
    taus = np.array([0.1, 0.2, 0.4, 0.6])
    t = np.concatenate([[0.0, 6.32], 3.0 + taus, [3.0]])
    g = np.stack([sc.gain64(seed, 5, 7, seed & 1, spread, t) for seed in range(nseeds)])
    power = (np.abs(g[:, :2]) ** 2).mean(axis=0)
    print(f"mean power over {nseeds} seeds: {power[0]:.4f} at t = 0, {power[1]:.4f} at t = 6.32 s")
    assert np.abs(power - 1.0).max() <= 0.08
    gstep = sc.taps(0, 0, 0, 0, spread)[0]
    f = ((gstep.astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)) * (100.0 / 4294967296.0)
    for k, tau in enumerate(taus):
        want = np.exp(-2.0 * (np.pi * (spread / 2.0) * tau) ** 2)
        exact = np.exp(-2j * np.pi * f * tau).mean()
        est = (g[:, -1] * np.conj(g[:, 2 + k])).mean()
        print(f"tau {tau}: Gaussian {want:.4f}, the taps' exact value {exact.real:.4f}{exact.imag:+.4f}j, over the seeds {est.real:.4f}{est.imag:+.4f}j")
        assert abs(exact - want) <= 0.04 and abs(est - want) <= 0.12


def test_two_paths_keep_the_mean_power_of_the_unfaded_signal():
    """the float32 rule itself: one signal, two equal paths 2 ms apart at 1 Hz, over 256 clip indices; the mean of the clips' power
    over the power of the unfaded clip.  A clip is the audio mode's first 8000 samples, 0.67 s: shorter than a fade at 1 Hz, and
    2 ms is short against a symbol, so the two paths add up to nearly one complex Gaussian gain of unit power and a clip's power is
    close to one exponential draw.  The mean over 256 clips then has a standard deviation near 1 / sqrt(256) = 0.0625; the margin is
    5 sigma, 0.32.  Paths that were not scaled by 1 / sqrt(1 + g2^2) would give 2."""
    sig = [(gc.random_tones(11), 1000.0, 0.0, 1.0)]
    n, nclips = 8000, 256
    base = float((sg.clip(sig, sg.AUDIO, n).astype(np.float64) ** 2).sum())
    p = [float((sc.clip(sig, [(1.0, 2.0, 1.0, sc.FADED)], sg.AUDIO, n, 5, c).astype(np.float64) ** 2).sum()) / base for c in range(nclips)]
    print(f"faded over unfaded power, mean of {nclips} clips: {np.mean(p):.4f} (single clips {min(p):.3f} .. {max(p):.3f})")
    assert abs(np.mean(p) - 1.0) <= 0.32


# ---- the example, the tool and the sanitizers ------------------------------------------------------------------------------------------

def test_gen_example_with_channel_options_compiles_against_the_public_header(tmp_path):
    obj = str(tmp_path / "ft8_gen.o")
    subprocess.check_call(["gcc", "-O2", "-std=gnu17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "ft8_gen.c"), "-o", obj])
    src = open(os.path.join(ROOT, "examples", "ft8_gen.c")).read()
    assert "--spread" in src and "--delay" in src and "--path2" in src and "ft8gpu_synth_gfsk_audio_faded" in src


def test_fading_curve_tool_runs_on_the_cpu(tmp_path):
    out = str(tmp_path / "curve.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fading_curve.py"), "--cpu", "--frames", "2", "--snr", "-10", "-9",
                        "--channels", "awgn", "disturbed", "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    doc = json.load(open(out))
    assert doc["mode"] == "cpu" and set(doc["curves"]) == {"awgn", "disturbed"} and doc["snr_db"] == [-10, -9]
    for ch in doc["curves"].values():
        for stage, hits in ch.items():
            assert len(hits) == 2 and all(0 <= h <= 2 for h in hits), (stage, hits)
    assert doc["curves"]["awgn"]["bp"] == [2, 2]                            # two frames at -10 and -9 dB in white noise decode


def test_host_code_under_asan_ubsan(tmp_path):
    """a program of its own (tests/host_asan/channel_asan_main.c) linked with csrc/ft8_gfsk.c; nothing is loaded into python"""
    exe = str(tmp_path / "channel_asan")
    csrc = os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_asan", "channel_asan_main.c"), os.path.join(csrc, "ft8_gfsk.c"),
                           "-lm", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "channel_asan ok" in out.stdout, (out.stdout + out.stderr)[-3000:]
