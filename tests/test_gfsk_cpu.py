"""The GFSK synthesiser without a GPU (include/ft8gpu.h "GFSK synthesis"): the library's tables against the numpy restatement
(tests/ft8_spec_gfsk.py), the restatement against the float64 definition and against a spectrum bound, its signals through the
audio front end's restatement and the CPU oracle, clipping, summing, peak and the int16 rails, the entries' refusals (which need
no context), the .wav writer against the reader, the example's compile check, and the host code under AddressSanitizer / UBSan as
a program of its own."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import audio_craft as ac
import ft8_spec_audio as sa
import ft8_spec_gfsk as sg
import gfsk_craft as gc
import synth_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ("ft8gpu_gfsk_pulse", "ft8gpu_gfsk_ramp", "ft8gpu_gfsk_twiddles", "ft8gpu_synth_gfsk_frames", "ft8gpu_synth_gfsk_audio",
               "ft8gpu_write_wav")


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as ft8
    ft8.load_library()
    return ft8


# ---- the tables -------------------------------------------------------------------------------------------------------------------

def test_twiddles_and_ramps_equal_the_formulas_bit_for_bit(ft8):
    gcoarse, gfine = ft8.gfsk_twiddles()
    rc, rf = sg.twiddles()
    assert gcoarse.dtype == F and gcoarse.shape == (4096, 2) and gfine.shape == (4096, 2)
    assert gcoarse.tobytes() == rc.tobytes() and gfine.tobytes() == rf.tobytes()
    for sps in (512, 1920):
        r = ft8.gfsk_ramp(sps)
        assert r.shape == (sps // 8,) and r.tobytes() == sg.ramp(sps).tobytes()
        assert r[0] == 0 and (np.diff(r) > 0).all() and r[-1] < 1
    lib = ft8.load_library()
    lib.ft8gpu_gfsk_twiddles(None, None)                                   # NULL tables are left out
    only = np.zeros((4096, 2), F)
    lib.ft8gpu_gfsk_twiddles(None, only.ctypes.data)
    assert only.tobytes() == rf.tobytes()
    for name in NEW_SYMBOLS:
        assert name in ft8.ABI_SYMBOLS
    assert (ft8.GFSK_IQ, ft8.GFSK_AUDIO, ft8.GFSK_SPS_IQ, ft8.GFSK_SPS_AUDIO) == (sg.IQ, sg.AUDIO, 512, 1920)
    assert ft8.GFSK_TILE >= 256 and ft8.GFSK_TILE % 256 == 0


@pytest.mark.parametrize("sps", [512, 1920])
def test_pulse_table_is_the_restatement_within_one_unit(ft8, sps):
    """two libms may round erf differently; the sums of at most 5760 terms of at most 1 carry less than 0.01 unit of error"""
    q, want = ft8.gfsk_pulse(sps), sg.pulse(sps)
    assert q.dtype == np.uint32 and q.shape == (3 * sps + 1,)
    d = (q.astype(np.int64) - want.astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)     # the difference mod 2^32
    print(f"sps {sps}: largest difference {np.abs(d).max()} units")
    assert np.abs(d).max() <= 1
    assert q[0] == 0 and q[3 * sps] == 0
    raw = sg.pulse(sps, unreduced=True)
    assert raw[3 * sps] == 1 << 32 and all(b >= a for a, b in zip(raw, raw[1:]))
    wrap = int(np.argmax(np.diff(q.astype(np.int64)) < 0)) + 1 if (np.diff(q.astype(np.int64)) < 0).any() else 3 * sps + 1
    assert (np.diff(q[:wrap].astype(np.int64)) >= 0).all() and not q[wrap:].any()            # nondecreasing, then 2^32 = 0
    p = sg.pulse_p(sps)
    assert p[3 * sps // 2] == p.max() and np.allclose(p[1:], p[:0:-1], rtol=0, atol=1e-15)    # peaks at 1.5 sps, symmetric about it


def test_table_builders_refuse_another_sps(ft8):
    lib = ft8.load_library()
    buf = np.full(16, 0xA5A5A5A5, np.uint32)
    for sps in (0, 1, 511, 1024, -512):
        assert lib.ft8gpu_gfsk_pulse(sps, buf.ctypes.data) == -1 and lib.ft8gpu_gfsk_ramp(sps, buf.ctypes.data) == -1
    assert lib.ft8gpu_gfsk_pulse(512, None) == -1 and lib.ft8gpu_gfsk_ramp(1920, None) == -1
    assert (buf == 0xA5A5A5A5).all()
    with pytest.raises(ft8.Ft8GpuError):
        ft8.gfsk_pulse(500)


# ---- the restatement against the definition ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,f0", [(sg.IQ, 700.3), (sg.AUDIO, 1500.0), (sg.IQ, -431.7)])
def test_restatement_lies_within_1e_6_of_the_definition(mode, f0):
    """the float64 model with the frequency as quantised; one constant phase removed.  Bound: the phase is truncated to 2^-24 turn
    (3.75e-7 rad), table rounding and the five float operations add under 3e-7."""
    tones = gc.random_tones(3)
    x = sg.contribution(tones, f0, 1.0, mode).astype(np.float64)
    z = x[0] + 1j * x[1]
    d = sg.definition(tones, f0, mode) * sg.envelope(mode).astype(np.float64)
    rot = np.vdot(d, z)
    rot /= abs(rot)
    err = np.abs(z - rot * d).max()
    print(f"mode {mode}, f0 {f0}: worst complex error {err:.3e} of the amplitude (bound 1e-6)")
    assert err <= 1e-6
    assert abs(np.abs(z[sg.SPS[mode]:-sg.SPS[mode]]).max() - 1) < 1e-6


# ---- spectrum ---------------------------------------------------------------------------------------------------------------------

def test_power_stays_within_the_tones_and_cpfsk_leaks_more():
    tones = gc.random_tones(4)
    f0 = 700.0
    x = sg.contribution(tones, f0, 1.0, sg.IQ).astype(np.float64)
    ci, cq = S.cpfsk(tones, f0, 0, 1.0, n=79 * 512)
    f = np.fft.fftfreq(79 * 512, 1 / 3200.0)
    band = (f >= f0 - 6.25) & (f <= f0 + 7 * 6.25 + 6.25)
    outside = []
    for z in (x[0] + 1j * x[1], ci + 1j * cq):
        p = np.abs(np.fft.fft(z)) ** 2
        outside.append(float(p[~band].sum() / p.sum()))
    print(f"power outside the 8 tones +- 6.25 Hz: GFSK {outside[0]:.3e}, CPFSK {outside[1]:.3e}")
    assert outside[0] <= 0.01
    assert outside[1] > outside[0]


# ---- decodes on the CPU -----------------------------------------------------------------------------------------------------------

def test_five_gfsk_signals_decode_through_the_audio_front_end(oracle):
    pcm = gc.five_signal_clip_gfsk(oracle)
    frames = sa.frames(pcm[None], sa.S16, ac.BANDS)[0]
    for b, base in enumerate(ac.BANDS):
        dec, n = oracle.subsystem(frames[b, 0], frames[b, 1])
        got = {f"CQ {dec[k]['call'].decode()} {dec[k]['loc'].decode()}": int(dec[k]["freq"]) for k in range(n)}
        print(f"band {base}: {got}")
        assert sorted(got) == sorted(ac.IN_BAND[base])
        for text, freq in got.items():
            assert freq + int(base * 6.25) == int(ac.planted_hz(text))


def test_eight_iq_frames_at_minus_16_db_decode_in_the_oracle(oracle):
    frames = gc.eight_frames(oracle)
    hit = [gc.EIGHT_TEXT in gc.decoded_texts(oracle, frames[s]) for s in range(8)]
    print(f"decoded {sum(hit)} of 8: {hit}")
    assert all(hit)


# ---- clipping and summing ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [sg.IQ, sg.AUDIO])
def test_signals_are_cut_not_shifted(mode):
    rate, n = sg.RATE[mode], (sg.NSAMPLES_IQ if mode == sg.IQ else 180000)
    tones = gc.random_tones(5)
    whole = sg.contribution(tones, 1000.0, 0.5, mode)
    if mode == sg.AUDIO:
        whole = whole[:1]
    early = np.atleast_2d(sg.clip([(tones, 1000.0, -0.5, 0.5)], mode, n))
    late = np.atleast_2d(sg.clip([(tones, 1000.0, 14.0, 0.5)], mode, n))
    h = rate // 2
    assert sg.start_of(-0.5, mode) == -h and sg.start_of(14.0, mode) == 14 * rate
    assert np.array_equal(early[:, :whole.shape[1] - h], whole[:, h:]) and not early[:, whole.shape[1] - h:].any()
    assert np.array_equal(late[:, 14 * rate:], whole[:, :n - 14 * rate]) and not late[:, :14 * rate].any()
    short = np.atleast_2d(sg.clip([(tones, 1000.0, 0.0, 0.5)], mode, n))[:, :7]
    if mode == sg.AUDIO:
        assert np.array_equal(sg.clip([(tones, 1000.0, 0.0, 0.5)], mode, 7), short[0])


def test_overlapping_signals_sum_in_signal_order():
    a = (gc.random_tones(6), 700.0, 0.5, 0.3)
    b = (gc.random_tones(7), 912.5, 1.0, 1e-4)
    c = (gc.random_tones(8), 1103.1, 0.2, 0.77)
    abc, cba = sg.clip([a, b, c], sg.IQ), sg.clip([c, b, a], sg.IQ)
    assert np.abs(abc.astype(np.float64) - cba).max() < 1e-6 and (abc.view(np.uint32) != cba.view(np.uint32)).any()
    ab, ba = sg.clip([a, b], sg.IQ), sg.clip([b, a], sg.IQ)
    assert ab.tobytes() == ba.tobytes()                     # one addition is commutative: the order shows from the third term on


def test_peak_is_reached_exactly_and_the_rails_clamp():
    sigs = [(gc.random_tones(9), 700.0, 0.5, 0.3), (gc.random_tones(10), 1500.0, 1.0, 0.9)]
    for mode, n in ((sg.IQ, None), (sg.AUDIO, 180000)):
        for peak in (0.5, 1.0, 0.123):
            x = sg.synth(sigs, mode, n, peak=peak)
            got = np.abs(x).max()
            assert abs(float(got) - peak) <= peak * 2.0 ** -23, (mode, peak, got)
    assert np.abs(sg.synth([], sg.IQ, peak=0.5)).max() == 0                # silence stays silence: m = 1e-24
    x = np.array([1.0, -1.0, 0.99999, 2.0, -2.0, np.nan, np.inf, -np.inf, 0.5 / 32768, 1.5 / 32768, -0.5 / 32768, 2.0 ** -130], F)
    assert sg.to_s16(x).tolist() == [32767, -32768, 32767, 32767, -32768, 0, 32767, -32768, 0, 2, 0, 0]
    loud = sg.synth([(gc.random_tones(9), 700.0, 0.0, 1.5)], sg.AUDIO, 4000, fmt=sg.S16)
    assert loud.max() == 32767 and loud.min() == -32768


# ---- host entries -----------------------------------------------------------------------------------------------------------------

def _signals(n=1, **kw):
    s = np.zeros(n, gc.SIGNAL_DTYPE)
    s["f0_hz"], s["t0_s"], s["amplitude"] = 1000.0, 0.5, 1.0
    for k, v in kw.items():
        s[k][-1] = v
    return s


REFUSALS = [
    ("audio", dict(sig=_signals(f0_hz=np.nan)), "f0_hz, t0_s or amplitude is not finite"),
    ("audio", dict(sig=_signals(t0_s=np.inf)), "f0_hz, t0_s or amplitude is not finite"),
    ("frames", dict(sig=_signals(2, amplitude=-np.inf), nsig=2), "signal 1 of clip 0: f0_hz, t0_s or amplitude is not finite"),
    ("audio", dict(sig=_signals(f0_hz=12000.0)), "f0_hz 12000 out of range [0, 12000)"),
    ("audio", dict(sig=_signals(f0_hz=-1.0)), "f0_hz -1 out of range [0, 12000)"),
    ("frames", dict(sig=_signals(f0_hz=3200.0)), "f0_hz 3200 out of range (-3200, 3200)"),
    ("frames", dict(sig=_signals(f0_hz=-3200.0)), "f0_hz -3200 out of range (-3200, 3200)"),
    ("audio", dict(sig=_signals(t0_s=60.5)), "t0_s 60.5 out of range [-60, 60]"),
    ("frames", dict(sig=_signals(t0_s=-61.0)), "t0_s -61 out of range [-60, 60]"),
    ("audio", dict(sig=_signals(tones=np.r_[np.zeros(78, np.uint8), 8])), "tone 78 is 8, above 7"),
    ("frames", dict(sig=_signals(65), nsig=65), "nsig 65 out of range [0, 64]"),
    ("audio", dict(nsig=-1), "nsig -1 out of range [0, 64]"),
    ("audio", dict(nsamples=0), "nsamples 0 out of range [1, 180000]"),
    ("audio", dict(nsamples=180001), "nsamples 180001 out of range [1, 180000]"),
    ("audio", dict(fmt=2), "unknown audio format 2"),
    ("audio", dict(fmt=-1), "unknown audio format -1"),
    ("frames", dict(peak=-0.5), "peak -0.5 is negative or not finite"),
    ("audio", dict(peak=np.nan), "peak nan is negative or not finite"),
    ("frames", dict(sigma=-1.0), "noise_sigma -1 is negative or not finite"),
    ("audio", dict(sigma=np.inf), "noise_sigma inf is negative or not finite"),
    ("audio", dict(sig=None), "NULL array argument"),
]


def call_entry(lib, ctx, which, out, sig=_signals(), nclips=1, nsig=1, nsamples=64, sigma=0.0, peak=0.0, fmt=1, flags=0):
    sp = None if sig is None else sig.ctypes.data
    op = None if out is None else out.ctypes.data
    if which == "frames":
        return lib.ft8gpu_synth_gfsk_frames(ctx, sp, nclips, nsig, sigma, 1, 0, peak, op, flags)
    return lib.ft8gpu_synth_gfsk_audio(ctx, sp, nclips, nsig, nsamples, sigma, 1, 0, peak, fmt, op, flags)


@pytest.mark.parametrize("which,kw,says", REFUSALS, ids=[f"{w}-{s[:24]}" for w, _, s in REFUSALS])
def test_entries_refuse_with_a_message_before_the_context_is_looked_at(ft8, which, kw, says):
    lib = ft8.load_library()
    out = np.full(2 * 48000, 0x5A5A5A5A, np.uint32)
    assert call_entry(lib, None, which, out, **kw) == -1
    err = lib.ft8gpu_last_error().decode()
    print(err)
    assert says in err and (out == 0x5A5A5A5A).all()


def test_entries_refuse_a_null_context(ft8):
    lib = ft8.load_library()
    out = np.full(2 * 48000, 0x5A5A5A5A, np.uint32)
    for which in ("frames", "audio"):
        assert call_entry(lib, None, which, out) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()
        assert call_entry(lib, None, which, out, nclips=0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()
    assert (out == 0x5A5A5A5A).all()


def test_wav_writer_round_trip(ft8, tmp_path):
    for n in (0, 1, 5000, 180000):
        pcm = ac.to_s16(np.random.default_rng(8 + n).normal(0, 0.3, n))
        if n:
            pcm[0], pcm[-1] = -32768, 32767
        path = str(tmp_path / f"w{n}.wav")
        ft8.write_wav(path, pcm)
        assert os.path.getsize(path) == 44 + 2 * n
        assert np.array_equal(ft8.read_wav(path), pcm)
        with wave.open(path, "rb") as w:                                   # another reader agrees
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 12000, n)
            assert w.readframes(n) == pcm.astype("<i2").tobytes()


def test_wav_writer_refuses(ft8, tmp_path, capfd):
    lib = ft8.load_library()
    pcm = np.zeros(8, np.int16)
    bad = str(tmp_path / "no-such-directory" / "x.wav")
    capfd.readouterr()
    assert lib.ft8gpu_write_wav(bad.encode(), pcm.ctypes.data, 8) == -1
    assert bad in capfd.readouterr().err
    assert lib.ft8gpu_write_wav(None, pcm.ctypes.data, 8) == -1
    assert lib.ft8gpu_write_wav(str(tmp_path / "y.wav").encode(), None, 8) == -1
    assert lib.ft8gpu_write_wav(str(tmp_path / "y.wav").encode(), pcm.ctypes.data, -1) == -1
    assert not (tmp_path / "y.wav").exists()
    with pytest.raises(ft8.Ft8GpuError):
        ft8.write_wav(bad, pcm)


def test_gen_example_compiles_against_the_public_header(tmp_path):
    obj = str(tmp_path / "ft8_gen.o")
    subprocess.check_call(["gcc", "-O2", "-std=gnu17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "ft8_gen.c"), "-o", obj])


def test_host_code_under_asan_ubsan(tmp_path):
    """a program of its own (tests/host_asan/gfsk_asan_main.c) linked with csrc/ft8_gfsk.c, csrc/ft8_compat.c and csrc/ft8_pack.c;
    nothing is loaded into python"""
    exe = str(tmp_path / "gfsk_asan")
    csrc = os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_asan", "gfsk_asan_main.c"),
                           os.path.join(csrc, "ft8_gfsk.c"), os.path.join(csrc, "ft8_compat.c"), os.path.join(csrc, "ft8_pack.c"),
                           "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe, str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "gfsk_asan ok" in out.stdout, (out.stdout + out.stderr)[-3000:]
