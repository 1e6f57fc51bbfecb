"""The PCM front end without a GPU (include/ft8gpu.h "PCM front end"): the tables of the rule against their formulas and against
the filter bounds, the numpy restatement (tests/ft8_spec_pcm.py) against a float64 definition within a derived bound, on pure
tones and through the CPU oracle, the merge rule on hand-made records, the .wav reader on every accepted layout and every
refusal, the exported entries, the example, and the host C file under AddressSanitizer / UBSan as a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import ft8_spec_pcm as sp
import pcm_craft as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAMES = ("ft8gpu_pcm_decimation", "ft8gpu_pcm_mixer1", "ft8gpu_pcm_mixer2", "ft8gpu_pcm_taps_a", "ft8gpu_pcm_taps_b",
         "ft8gpu_pcm_frames", "ft8gpu_decode_pcm", "ft8gpu_read_wav_pcm")


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as ft8
    ft8.load_library()
    return ft8


# ---- the tables -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", sp.DS)
def test_tables_equal_the_formulas_bit_for_bit(ft8, D):
    M = D // 3
    w1, h = ft8.pcm_mixer1(D), ft8.pcm_taps_a(D)
    assert w1.dtype == F32 and w1.shape == (16 * D, 2) and h.dtype == F32 and h.shape == (8 * M + 1,)
    assert w1.tobytes() == sp.mixer1(D).tobytes() and h.tobytes() == sp.taps_a(D).tobytes()
    assert np.array_equal(h, h[::-1]) and abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6 and h[4 * M] == h.max()
    i = np.arange(16 * D)
    assert np.abs(w1[:, 0] - np.cos(2 * np.pi * i / (16 * D))).max() <= 2.0 ** -24
    assert np.abs(w1[:, 1] + np.sin(2 * np.pi * i / (16 * D))).max() <= 2.0 ** -24
    assert tuple(w1[0]) == (1.0, 0.0) and w1[4 * D, 1] == -1.0 and w1[8 * D, 0] == -1.0
    assert ft8.load_library().ft8gpu_pcm_decimation(3200 * D) == D


def test_second_stage_tables_and_refused_table_calls(ft8):
    w2, h = ft8.pcm_mixer2(), ft8.pcm_taps_b()
    assert w2.dtype == F32 and w2.shape == (1536, 2) and h.dtype == F32 and h.shape == (48,)
    assert w2.tobytes() == sp.mixer2().tobytes() and h.tobytes() == sp.taps_b().tobytes()
    assert h[47] == 0 and np.array_equal(h[:47], h[46::-1]) and abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6
    lib = ft8.load_library()
    lib.ft8gpu_pcm_mixer1(15, None)                                       # a NULL table is ignored
    lib.ft8gpu_pcm_mixer2(None)
    lib.ft8gpu_pcm_taps_b(None)
    assert lib.ft8gpu_pcm_taps_a(15, None) == -1
    keep = np.full(4, 7.0, F32)
    lib.ft8gpu_pcm_mixer1(45, keep.ctypes.data)                           # an unknown D writes nothing
    assert lib.ft8gpu_pcm_taps_a(45, keep.ctypes.data) == -1 and (keep == 7.0).all()
    for rate in (0, 12000, 44100, 47999, 1536000, -48000):
        assert lib.ft8gpu_pcm_decimation(rate) == 0
    with pytest.raises(ft8.Ft8GpuError):
        ft8.pcm_taps_a(45)


def chain_response_db(D, q):
    """float taps of both stages, every 3.125 Hz of the input band: f (offset from the band's centre), gain in dB.  A tone at
    offset f lies at f + 6.25 q behind the first mixer, is folded to 9600 sps and moved by -6.25 q by the second."""
    rate = 3200 * D
    n1, n2 = rate * 8 // 25, 3072                                         # 3.125 Hz per point at both rates
    ha = np.abs(np.fft.fft(sp.taps_a(D).astype(np.float64), n1))
    hb = np.abs(np.fft.fft(sp.taps_b().astype(np.float64)[:47], n2))
    i = np.arange(-n1 // 2, n1 // 2)                                      # offset in steps of 3.125 Hz
    a = i + 2 * q
    gain = ha[a % n1] * hb[(a % n2 - 2 * q) % n2]
    return 3.125 * i, 20 * np.log10(np.maximum(gain, 1e-300))


@pytest.mark.parametrize("D", sp.DS)
def test_chain_meets_the_filter_bounds(D):
    """at most -80 dB at or beyond 2400 Hz from the band's centre, within +-0.06 dB up to 800 Hz, for q = -16, 0, 15"""
    for q in (-16, 0, 15):
        f, db = chain_response_db(D, q)
        stop, lo, hi = db[np.abs(f) >= 2400].max(), db[np.abs(f) <= 800].min(), db[np.abs(f) <= 800].max()
        print(f"D {D} q {q}: stopband {stop:.2f} dB, passband {lo:+.5f} .. {hi:+.5f} dB")
        assert stop <= -80.0 and lo >= -0.06 and hi <= 0.06


def test_entries_are_exported_and_refuse_a_null_context(ft8):
    lib = ft8.load_library()
    for name in NAMES:
        assert name in ft8.ABI_SYMBOLS and hasattr(lib, name)
    assert lib.ft8gpu_pcm_frames(None, None, 0, 48000, 1, 8, None, 1, None, 0, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_decode_pcm(None, None, 0, 48000, 1, 8, None, 1, None, None, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()


def test_channel_arithmetic_covers_the_range():
    for D in sp.DS:
        for fmt in pc.FORMATS:
            lo, hi = sp.bin_range(D, fmt)
            for fb in (lo, lo + 1, hi - 1, hi) + pc.sixteen(D, fmt):
                c, q = sp.channel(fb)
                assert -16 <= q <= 15 and 32 * c + q == fb + 128 and abs(200 * c) <= 1600 * D    # the mixer stays inside the band


# ---- the restatement against a float64 definition ---------------------------------------------------------------------------------

def frame_float64(xr, xi, D, freq_bin):
    """the rule in double with exact-frequency mixers and the same (float) taps -> complex128 [48000]"""
    M = D // 3
    c, q = sp.channel(freq_bin)
    n = xr.shape[0]
    x = xr.astype(np.float64) + 1j * (0.0 if xi is None else xi.astype(np.float64))
    u = x * np.exp(-2j * np.pi * ((np.arange(n) * c) % (16 * D)) / (16 * D))
    ml = sp.last_m(D, n)
    up = np.zeros(M * ml + 8 * M + 1, np.complex128)
    k = min(n, up.shape[0] - 4 * M)
    up[4 * M:4 * M + k] = u[:k]
    h = sp.taps_a(D).astype(np.float64)
    at = M * np.arange(ml + 1) + 8 * M
    v = np.zeros(ml + 1, np.complex128)
    for k in range(8 * M + 1):
        v += h[k] * up[at - k]
    m = np.arange(ml + 1)
    z = np.zeros(3 * sp.NSAMPLES + 64, np.complex128)
    z[23:23 + ml + 1] = v * np.exp(-2j * np.pi * ((m * q) % 1536) / 1536)
    hb = sp.taps_b().astype(np.float64)
    at = 3 * np.arange(sp.NSAMPLES) + 46
    y = np.zeros(sp.NSAMPLES, np.complex128)
    for k in range(47):
        y += hb[k] * z[at - k]
    return y * 1j ** (np.arange(sp.NSAMPLES) % 4)


def float32_bound(D, peak):
    """A bound on the error of a component of the float32 chain against the float64 one, for components of x up to `peak`, from
    the standard model: every operation has relative error u = 2^-24, a table entry too, and a sequential sum of n products has
    error at most gamma_n * sum |h_k| |u_k|, gamma_n = n u / (1 - n u).
      a mixed component: at most 2 peak; its error: two products, an add and the entries' rounding, 4 u on each term -> 8 u peak.
      stage A: E_A = S_A (gamma_(8M+1) * 2 peak + 8 u peak), |v| <= V = 2 S_A peak.
      second mixer: |z| <= 2 V, error 2 E_A + 8 u V.
      stage B: E = S_B (gamma_47 * 2 V + 2 E_A + 8 u V); the rotation is exact."""
    u = 2.0 ** -24
    M = D // 3

    def gamma(n):
        return n * u / (1 - n * u)

    s_a = float(np.abs(sp.taps_a(D).astype(np.float64)).sum())
    s_b = float(np.abs(sp.taps_b().astype(np.float64)).sum())
    e_a = s_a * (gamma(8 * M + 1) * 2 * peak + 8 * u * peak)
    v = 2 * s_a * peak
    return s_b * (gamma(47) * 2 * v + 2 * e_a + 8 * u * v)


@pytest.mark.parametrize("D", sp.DS)
def test_restatement_is_the_float64_definition_within_the_summation_bound(D):
    for fmt, fb in ((sp.F32FMT | sp.COMPLEX, -177), (sp.S16, 47)):
        pcm = pc.random_capture(fmt, 40 * D + 7, 70 + D)
        xr, xi = sp.samples(pcm, fmt)
        peak = float(max(np.abs(xr).max(), 0.0 if xi is None else np.abs(xi).max()))
        got = sp.frame(pcm, fmt, D, fb)
        want = frame_float64(xr, xi, D, fb)
        err = max(float(np.abs(got[0] - want.real).max()), float(np.abs(got[1] - want.imag).max()))
        bound = float32_bound(D, peak)
        print(f"D {D} {pc.FORMAT_NAMES[fmt]}: error {err:.3e}, bound {bound:.3e}, output peak {np.abs(want).max():.3f}")
        assert np.abs(want).max() > 1e-3 and err <= bound


# ---- tones ------------------------------------------------------------------------------------------------------------------------

def tone_db(x, amplitude):
    """(bin, dB against `amplitude`) of the largest line of outputs 512 .. 1023 (6.25 Hz per bin)"""
    spec = np.fft.fft((x[0].astype(np.float64) + 1j * x[1])[512:1024])
    k = int(np.argmax(np.abs(spec)))
    return k, 20 * np.log10(np.abs(spec[k]) / 512 / amplitude)


def test_a_complex_tone_arrives_at_its_bin_with_its_amplitude():
    D, freq_bin = 60, -12011
    rate = 3200 * D
    assert sp.channel(freq_bin) == (-371, -11)
    t = np.arange(rate // 2) / rate
    z = 0.9 * np.exp(2j * np.pi * (6.25 * freq_bin + 1000.0) * t)
    pcm = np.empty(2 * t.size, F32)
    pcm[0::2], pcm[1::2] = z.real, z.imag
    for fmt, data in ((sp.F32FMT | sp.COMPLEX, pcm), (sp.S16 | sp.COMPLEX, pc.to_s16(pcm))):
        k, db = tone_db(sp.frame(data, fmt, D, freq_bin), 0.9)
        print(f"{pc.FORMAT_NAMES[fmt]}: peak at bin {k}, {db:+.4f} dB")
        assert k == 160 and abs(db) <= 0.06


def test_a_real_tone_arrives_at_its_bin_with_half_its_amplitude():
    """a real cosine of amplitude A is two complex lines of A / 2; the channel holds the upper one"""
    D, freq_bin = 15, 1203
    t = np.arange(24000) / 48000.0
    pcm = (0.8 * np.cos(2 * np.pi * (6.25 * freq_bin + 1000.0) * t)).astype(F32)
    for fmt, data in ((sp.F32FMT, pcm), (sp.S16, pc.to_s16(pcm))):
        k, db = tone_db(sp.frame(data, fmt, D, freq_bin), 0.4)
        print(f"{pc.FORMAT_NAMES[fmt]}: peak at bin {k}, {db:+.4f} dB")
        assert k == 160 and abs(db) <= 0.06


@pytest.mark.parametrize("D", (15, 240))
def test_a_tone_beyond_2400_hz_is_suppressed_by_the_bound(D):
    """tones 2400 Hz below and 2450 Hz above the band's centre, and one that the first decimation folds onto the centre: every
    output of the steady state stays 80 dB below the tone"""
    rate = 3200 * D
    freq_bin = 1000
    centre = 6.25 * (freq_bin + 128)
    t = np.arange(rate // 4) / rate
    for off in (-2400.0, 2450.0, 9600.0):
        z = np.exp(2j * np.pi * (centre + off) * t)
        pcm = np.empty(2 * t.size, F32)
        pcm[0::2], pcm[1::2] = z.real, z.imag
        x = sp.frame(pcm, sp.F32FMT | sp.COMPLEX, D, freq_bin)
        steady = np.abs(x[0, 100:700].astype(np.float64) + 1j * x[1, 100:700]).max()
        print(f"D {D}, {off:+.0f} Hz: {20 * np.log10(max(steady, 1e-300)):.2f} dB")
        assert steady <= 1e-4


# ---- through the CPU oracle -------------------------------------------------------------------------------------------------------

def test_restated_frames_of_48_ksps_audio_decode_in_the_oracle(oracle):
    """15 s of real audio at 48 ksps built in numpy, two CPFSK signals, one per channel, over noise, as int16"""
    n = sp.max_samples(15)
    planted = (("CQ K1ABC FN42", 0, 500.0, 0.5), ("CQ DL1XYZ JO62", 1500, 1000.0, 0.8))
    x = np.random.default_rng(11).normal(0, 0.05, n)
    for text, fb, f0, t0 in planted:
        rc, payload = oracle.pack77(text)
        assert rc == 0
        x += pc.cpfsk(oracle.encode(payload[:10]), 6.25 * fb + f0, t0, n, 0.03, 48000).real
    frames = sp.frames(pc.to_s16(x)[None], sp.S16, 15, [fb for _, fb, _, _ in planted], normalise=True)[0]
    for b, (text, fb, f0, _) in enumerate(planted):
        dec, cnt = oracle.subsystem(frames[b, 0], frames[b, 1])
        got = {f"CQ {dec[k]['call'].decode()} {dec[k]['loc'].decode()}": int(dec[k]["freq"]) for k in range(cnt)}
        print(f"channel {fb}: {got}")
        assert got == {text: int(f0)}


# ---- the merge rule ---------------------------------------------------------------------------------------------------------------

def test_merge_rule_on_hand_made_records(ft8):
    rng = np.random.default_rng(3)
    bins = (1000, 1240, 1256, -3000)
    bm = np.zeros((1, 4, 50), ft8.MESSAGE_DTYPE)
    bm.view(np.uint8)[...] = rng.integers(0, 256, bm.view(np.uint8).shape, dtype=np.uint8)    # every field, the padding too
    bm["cand"]["freq_offset"] = rng.integers(0, 249, bm.shape)
    bm["cand"]["freq_sub"] = rng.integers(0, 2, bm.shape)
    bn = np.array([[2, 3, 2, 70]], np.int32)                              # counts are clamped to [0, 50]
    bm[0, 1, 1]["a91"] = bm[0, 0, 0]["a91"]                               # 240 bins apart: dropped, the first wins
    bm[0, 2, 0]["a91"] = bm[0, 0, 1]["a91"]                               # 256 bins apart: kept twice
    bm[0, 2, 1]["a91"] = bm[0, 1, 2]["a91"]                               # 16 bins apart: dropped
    bm[0, 3, 5]["a91"] = bm[0, 0, 0]["a91"]                               # far away: kept
    bm[0, 3, 7]["a91"] = bm[0, 3, 6]["a91"]                               # within a channel: dropped
    msgs = np.zeros((1, 200), ft8.MESSAGE_DTYPE)
    msgs.view(np.uint8)[...] = 0xA5
    n = np.full(1, -1, np.int32)
    sp.merge(bm, bn, bins, msgs, n)
    order = [(0, 0), (0, 1), (1, 0), (1, 2), (2, 0)] + [(3, k) for k in range(50) if k != 7]
    assert n.tolist() == [len(order)]
    for k, (b, r) in enumerate(order):
        want = bm[0, b, r].copy()
        want["freq_hz"] = (F32(int(want["cand"]["freq_offset"]) + bins[b]) + F32(want["cand"]["freq_sub"]) / F32(2)) * F32(6.25)
        want["pad"][0] = b
        assert msgs[0, k].tobytes() == want.tobytes()
    assert (msgs[0, len(order):].view(np.uint8) == 0xA5).all()
    neg = msgs[0, 5]
    assert neg["pad"][0] == 3 and neg["freq_hz"] < 0
    assert float(neg["freq_hz"]) == (int(neg["cand"]["freq_offset"]) - 3000 + int(neg["cand"]["freq_sub"]) / 2) * 6.25        # exact
    bn[:] = 1000                                                           # the cap: never more than 50 * nchannels
    sp.merge(bm, bn, bins, msgs, n)
    assert n[0] <= 200


# ---- the .wav reader --------------------------------------------------------------------------------------------------------------

LAYOUTS = [(1, 1, 16, False), (1, 2, 16, False), (3, 1, 32, False), (3, 2, 32, False), (1, 2, 16, True), (3, 1, 32, True)]


@pytest.mark.parametrize("tag,channels,bits,extensible", LAYOUTS)
def test_wav_round_trip(ft8, tmp_path, tag, channels, bits, extensible):
    rng = np.random.default_rng(bits + channels)
    for rate in ft8.PCM_RATES:
        nsamples = 1001
        data = (rng.integers(-32768, 32768, channels * nsamples).astype(np.int16) if bits == 16 else
                rng.normal(0, 0.3, channels * nsamples).astype(F32))
        path = tmp_path / f"t{rate}.wav"
        path.write_bytes(pc.wav_bytes(data.tobytes(), rate, channels, tag, bits, extensible, extra_chunks=((b"LIST", b"12345"),)))
        got, fmt, got_rate = ft8.read_wav_pcm(str(path))
        assert fmt == (sp.F32FMT if bits == 32 else sp.S16) | (sp.COMPLEX if channels == 2 else 0) and got_rate == rate
        assert got.dtype == data.dtype and got.tobytes() == data.tobytes()
        cut, _, _ = ft8.read_wav_pcm(str(path), cap_bytes=100 * channels * bits // 8 + 1)      # truncated at cap_bytes, whole samples
        assert cut.tobytes() == data[:100 * channels].tobytes()


def test_wav_longer_than_15_s_is_truncated(ft8, tmp_path):
    data = np.zeros(720000 + 500, np.int16)
    data[-600:] = 5
    path = tmp_path / "long.wav"
    path.write_bytes(pc.wav_bytes(data.tobytes(), 48000, 1, 1, 16))
    got, fmt, rate = ft8.read_wav_pcm(str(path))
    assert got.shape == (720000,) and fmt == sp.S16 and rate == 48000 and got.tobytes() == data[:720000].tobytes()


def test_wav_refusals_name_what_was_found(ft8, tmp_path, capfd):
    lib = ft8.load_library()
    import ctypes as C
    data = bytes(64)
    ok = pc.wav_bytes(data, 48000, 1, 1, 16)
    cases = [("8bit", pc.wav_bytes(data, 48000, 1, 1, 8), "48000 Hz, 8 bit"), ("24bit", pc.wav_bytes(data + bytes(2), 48000, 1, 1, 24), "24 bit"),
             ("3ch", pc.wav_bytes(data + bytes(2), 48000, 3, 1, 16), "3 channel(s)"), ("44100", pc.wav_bytes(data, 44100, 1, 1, 16), "44100 Hz"),
             ("12000", pc.wav_bytes(data, 12000, 1, 1, 16), "12000 Hz"), ("float16", pc.wav_bytes(data, 48000, 1, 3, 16), "format tag 3"),
             ("adpcm", pc.wav_bytes(data, 48000, 1, 2, 16), "format tag 2"), ("ext24", pc.wav_bytes(data + bytes(2), 48000, 1, 1, 24, True), "24 bit"),
             ("header", ok[:10], "truncated header"), ("fmtcut", ok[:30], "truncated header"), ("stray", ok[:12] + b"abc", "truncated header"),
             ("nodata", ok[:36], "no data chunk"), ("short", pc.wav_bytes(data, 48000, 1, 1, 16, declared=100), "data chunk declares 100 bytes"),
             ("notwav", b"RIFX" + ok[4:], "not a RIFF/WAVE file"), ("empty", b"", "empty file"),
             ("datafirst", ok[:12] + b"data" + bytes(4) + ok[12:], "data chunk in front of the fmt chunk"),
             ("oddcut", pc.wav_bytes(data, 48000, 1, 1, 16, extra_chunks=((b"LIST", b"123"),))[:40], "truncated header")]
    out = np.full(64, 0x5A, np.uint8)
    for name, image, text in cases:
        path = tmp_path / f"{name}.wav"
        path.write_bytes(image)
        fmt, rate, n = C.c_int(9), C.c_int(9), C.c_int32(9)
        capfd.readouterr()
        rc = lib.ft8gpu_read_wav_pcm(os.fsencode(str(path)), out.ctypes.data, 64, C.byref(fmt), C.byref(rate), C.byref(n))
        err = capfd.readouterr().err
        assert rc == -1 and (fmt.value, rate.value, n.value) == (-1, 0, 0) and text in err and str(path) in err, (name, err)
        assert (out == 0x5A).all()
        with pytest.raises(ft8.Ft8GpuError):
            ft8.read_wav_pcm(str(path))
    # an odd-sized chunk is padded: the reader finds the data behind the pad byte
    path = tmp_path / "odd.wav"
    path.write_bytes(pc.wav_bytes(np.arange(32, dtype=np.int16).tobytes(), 96000, 2, 1, 16, extra_chunks=((b"LIST", b"123"), (b"junk", b""))))
    got, fmt, rate = ft8.read_wav_pcm(str(path))
    assert got.tolist() == list(range(32)) and fmt == sp.S16 | sp.COMPLEX and rate == 96000
    with pytest.raises(ft8.Ft8GpuError):
        ft8.read_wav_pcm(str(tmp_path / "missing.wav"))


# ---- the host C file and the example ----------------------------------------------------------------------------------------------

def test_host_file_under_asan_ubsan(tmp_path):
    """a program of its own (tests/host_asan/pcm_asan_main.c) linked with csrc/ft8_pcm.c; nothing is loaded into python"""
    exe = str(tmp_path / "pcm_asan")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_asan", "pcm_asan_main.c"),
                           os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc", "ft8_pcm.c"), "-lm", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe, str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pcm_asan ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


def test_pcm_example_compiles_against_the_public_header(tmp_path):
    obj = str(tmp_path / "ft8_pcm.o")
    subprocess.check_call(["gcc", "-O2", "-std=gnu17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "ft8_pcm.c"), "-o", obj])
