"""The audio front end without a GPU (include/ft8gpu.h "12 kHz audio"): the tables of the rule against their formulas and against
the filter bounds, the numpy restatement (tests/ft8_spec_audio.py) on a pure tone and through the CPU oracle, against the stage's
definition in double and against single taps, the inputs of the GPU tests (table entries read, clip ends, the twelve-signal
clip), the merge rule on hand-made records, and the .wav reader -- also under AddressSanitizer / UBSan as a program of its own."""
import ctypes as C
import os
import struct
import subprocess
import wave

import numpy as np
import pytest

import audio_craft as ac
import ft8_spec_audio as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as ft8
    ft8.load_library()
    return ft8


# ---- the tables -------------------------------------------------------------------------------------------------------------------

def test_tables_equal_the_formulas_bit_for_bit(ft8):
    h, wm = ft8.audio_taps(), ft8.audio_mixer()
    assert h.dtype == F32 and h.shape == (160,) and wm.dtype == F32 and wm.shape == (1920, 2)
    assert h.tobytes() == sa.taps().tobytes() and wm.tobytes() == sa.mixer().tobytes()
    assert h[159] == 0 and np.array_equal(h[:159], h[158::-1])            # symmetric about index 79
    i = np.arange(1920)
    assert np.abs(wm[:, 0] - np.cos(2 * np.pi * i / 1920)).max() < 1e-7 and np.abs(wm[:, 1] + np.sin(2 * np.pi * i / 1920)).max() < 1e-7
    lib = ft8.load_library()
    lib.ft8gpu_audio_taps(None)                                           # a NULL table is ignored
    lib.ft8gpu_audio_mixer(None)
    for name in ("ft8gpu_audio_taps", "ft8gpu_audio_mixer", "ft8gpu_audio_frames", "ft8gpu_decode_audio", "ft8gpu_read_wav"):
        assert name in ft8.ABI_SYMBOLS


def test_taps_meet_the_filter_bounds(ft8):
    """2^18-point response of the float taps at the 48 kHz rate, against the gain of 8 (4 for the zero stuffing times 2): at most
    -80 dB from 2400 Hz on (the offsets that alias into the bins the decoder reads), within +-0.002 dB up to 800 Hz"""
    h = ft8.audio_taps().astype(np.float64)
    H = np.abs(np.fft.rfft(h, 1 << 18)) / 8.0
    f = np.arange(H.size) * 48000.0 / (1 << 18)
    db = 20 * np.log10(np.maximum(H, 1e-300))
    stop, lo, hi = db[f >= 2400].max(), db[f <= 800].min(), db[f <= 800].max()
    print(f"stopband {stop:.2f} dB, passband {lo:+.5f} .. {hi:+.5f} dB")
    assert stop <= -80.0 and lo >= -0.002 and hi <= 0.002


def test_entries_refuse_a_null_context(ft8):
    lib = ft8.load_library()
    assert lib.ft8gpu_audio_frames(None, None, 0, 1, 1, None, 1, None, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_decode_audio(None, None, 0, 1, 1, None, 1, None, None, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()


# ---- the restatement --------------------------------------------------------------------------------------------------------------

def test_a_pure_tone_arrives_at_its_bin_with_its_amplitude():
    t = np.arange(sa.NSAMPLES_AUDIO) / 12000.0
    a = (0.5 * np.cos(2 * np.pi * 1000.0 * t)).astype(F32)
    x = sa.frame(a, 0)
    spec = np.fft.fft((x[0] + 1j * x[1])[1000:4200])
    k = int(np.argmax(np.abs(spec)))
    amp = np.abs(spec[k]) / 3200
    print(f"peak at bin {k}, amplitude {amp:.5f}")
    assert k == 1000 and abs(amp - 0.5) <= 1e-3


@pytest.fixture(scope="module")
def five(oracle):
    pcm = ac.five_signal_clip(oracle)
    return pcm, sa.frames(pcm[None], sa.S16, ac.BANDS)[0]


def test_restated_frames_decode_in_the_oracle(oracle, five):
    """0 dB in 2500 Hz; every band gives exactly the planted signals within its reach, at their frequencies"""
    _, frames = five
    for b, base in enumerate(ac.BANDS):
        dec, n = oracle.subsystem(frames[b, 0], frames[b, 1])
        got = {f"CQ {dec[k]['call'].decode()} {dec[k]['loc'].decode()}": int(dec[k]["freq"]) for k in range(n)}
        print(f"band {base}: {got}")
        assert sorted(got) == sorted(ac.IN_BAND[base])
        for text, freq in got.items():
            assert freq + int(base * 6.25) == int(ac.planted_hz(text))


# ---- the restatement against the definition, against single taps, and where the GPU tests aim -----------------------------------

@pytest.mark.parametrize("nsamples", ac.REF64_LENGTHS)
@pytest.mark.parametrize("fmt", [sa.S16, sa.F32])
def test_restatement_lies_within_the_rounding_bound_of_the_definition(fmt, nsamples):
    """ac.ref64 is the stage in double from its definition (zero-stuff, FIR at 48 kHz, every 15th sample), with none of the phase
    arithmetic of the rule; the bound is 44 roundings of float32 on the window's magnitudes, derived there"""
    a = sa.samples(ac.noise_clip(fmt, nsamples), fmt)
    for base in ac.REF64_BASES:
        worst = ac.worst_ratio(sa.frame(a, base), a, base)
        print(f"format {fmt}, {nsamples} samples, base {base}: worst error {worst:.2f} u S (bound 44)")
        assert 0 < worst <= 44


@pytest.mark.parametrize("base", [3, 704])
@pytest.mark.parametrize("fmt", [sa.S16, sa.F32])
def test_impulse_clip_meets_every_tap_alone(fmt, base):
    """impulses 41 samples apart: no window holds two, so an output is one product of the tables or +0, and the closed form needs
    no sum.  The tap of an output has k mod 4 = r = (3 - m) mod 4, so a class of m mod 4 can meet only the taps of its own phase:
    it meets every one of them, 0 .. 158 over the four classes (41 is coprime to 4 and to 15)."""
    pcm = ac.impulse_clip(fmt)
    assert pcm[0] != 0 and np.flatnonzero(pcm)[-1] == (ac.N - 1) // 41 * 41 and np.count_nonzero(pcm) == (ac.N - 1) // 41 + 1
    want = ac.impulse_frame(pcm, fmt, base)
    _, k, hit = ac.impulse_taps()
    live = hit & ((want[0] != 0) | (want[1] != 0))
    m = np.arange(sa.NSAMPLES)
    used = set()
    for q in range(4):
        taps_q = set(k[live & (m % 4 == q)].tolist())
        assert taps_q == set(range((3 - q) % 4, 159, 4)), q
        used |= taps_q
    assert used == set(range(159))
    assert not want[:, ~hit].any()                                          # zeros elsewhere
    got = sa.frame(sa.samples(pcm, fmt), base)
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()


def test_new_band_lists_read_the_whole_mixer_table():
    """a band steps through the table by f = base + 128 and visits 1920 / gcd(f, 1920) entries: the band lists of the first GPU
    tests read 225 entries at most, the ones added since read all 1920"""
    old = set().union(*(ac.entries_read(b) for b in ac.OLD_BAND_LISTS))
    assert len(old) <= 225
    for base, visits in ((0, 15), (240, 120), (480, 60), (704, 30), (3, 1920)):
        assert len(ac.entries_read((base,))) == visits == 1920 // np.gcd(base + 128, 1920)
    lists = ac.OLD_BAND_LISTS + ac.WIDE_BAND_LISTS + (ac.SEAM_BANDS, ac.DOZEN_BANDS)
    assert set().union(*(ac.entries_read(b) for b in lists)) == set(range(1920))
    assert any(b % 2 for bl in ac.WIDE_BAND_LISTS for b in bl) and any(b % 4 == 0 and b % 16 for bl in ac.WIDE_BAND_LISTS for b in bl)


@pytest.mark.parametrize("fmt", [sa.S16, sa.F32])
@pytest.mark.parametrize("group", sorted(ac.SEAM_LENGTHS))
def test_clip_ends_fall_where_the_seam_lengths_say(fmt, group):
    """per length: the outputs all of whose taps lie past the clip are +0 under the rotation, bit for bit, and the output before
    them is not zero (from 179978 samples on no output is past the clip, and the last output stands for it)"""
    for nsamples in ac.SEAM_LENGTHS[group]:
        pcm = ac.seam_clips(fmt, nsamples)
        assert pcm.shape == (2, nsamples) and pcm[:, -1].all()
        m0 = ac.first_silent_output(nsamples)
        assert 1 <= m0 <= sa.NSAMPLES and (m0 == sa.NSAMPLES) == (nsamples >= 179978)
        x = sa.frames(pcm, fmt, ac.SEAM_BANDS)
        assert x[..., m0:].view(np.uint32).tobytes() == np.broadcast_to(ac.SILENCE[:, m0:], x[..., m0:].shape).view(np.uint32).tobytes()
        assert (np.abs(x[:, :, :, m0 - 1]).max(axis=2) > 0).all(), nsamples


@pytest.fixture(scope="module")
def dozen(oracle):
    pcm = ac.dozen_signal_clip(oracle)
    distinct = sorted(set(ac.DOZEN_BANDS))
    return pcm, dict(zip(distinct, sa.frames(pcm[None], sa.S16, distinct)[0]))


def test_dozen_signal_clip_decodes_in_three_overlapping_bands(oracle, dozen):
    """the clip of the merge test on the GPU: the oracle finds at least ten of the twelve signals in each of the three distinct
    bands of DOZEN_BANDS, at their frequencies (the seed was chosen for that)"""
    _, frames = dozen
    texts = [t for t, _, _ in ac.DOZEN]
    assert len(set(texts)) == 12 and len({f for _, f, _ in ac.DOZEN}) == 12 and len({s for _, _, s in ac.DOZEN}) == 12
    assert all(700 <= f <= 1500 for _, f, _ in ac.DOZEN) and len(set(ac.DOZEN_BANDS)) == 3
    for base, x in frames.items():
        dec, n = oracle.subsystem(x[0], x[1])
        got = {f"CQ {dec[k]['call'].decode()} {dec[k]['loc'].decode()}": int(dec[k]["freq"]) for k in range(n)}
        planted = [t for t in got if t in texts]
        print(f"band {base}: {len(planted)} of 12, {got}")
        assert len(planted) >= 10
        for t in planted:
            assert got[t] + int(base * 6.25) == int(ac.dozen_hz(t))


# ---- the merge rule ---------------------------------------------------------------------------------------------------------------

def _records(ft8, rng, nclips, nbands):
    m = np.zeros((nclips, nbands, 50), ft8.MESSAGE_DTYPE)
    m.view(np.uint8)[...] = rng.integers(0, 256, m.view(np.uint8).shape, dtype=np.uint8)    # every field, the padding too
    m["cand"]["freq_offset"] = rng.integers(0, 249, m.shape)
    m["cand"]["freq_sub"] = rng.integers(0, 2, m.shape)
    return m


def test_merge_rule_on_hand_made_records(ft8):
    rng = np.random.default_rng(3)
    bases = (0, 240, 704)
    bm = _records(ft8, rng, 2, 3)
    bn = np.array([[3, 4, 2], [50, 70, -5]], np.int32)                    # counts are clamped to [0, 50]
    bm[0, 1, 1]["a91"] = bm[0, 0, 2]["a91"]                               # a duplicate across bands
    bm[0, 2, 0]["a91"] = bm[0, 1, 0]["a91"]
    bm[0, 1, 3]["a91"] = bm[0, 1, 2]["a91"]                               # and within a band
    bm[1, 1, 7]["a91"] = bm[1, 0, 49]["a91"]
    msgs = np.zeros((2, 150), ft8.MESSAGE_DTYPE)
    msgs.view(np.uint8)[...] = 0xA5
    n = np.full(2, -1, np.int32)
    sa.merge(bm, bn, bases, msgs, n)
    assert n.tolist() == [6, 99]
    order = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 1)]              # (band, record) of clip 0's kept records, in order
    for k, (b, r) in enumerate(order):
        want = bm[0, b, r].copy()
        want["freq_hz"] = (F32(int(want["cand"]["freq_offset"]) + bases[b]) + F32(want["cand"]["freq_sub"]) / F32(2)) * F32(6.25)
        want["pad"][0] = b
        assert msgs[0, k].tobytes() == want.tobytes()
    assert (msgs[0, 6:].view(np.uint8) == 0xA5).all() and (msgs[1, 99:].view(np.uint8) == 0xA5).all()
    assert msgs[1, 49]["pad"][0] == 0 and msgs[1, 50]["pad"][0] == 1 and msgs[1, 98].tobytes()[48:60] == bm[1, 1, 49]["a91"].tobytes()
    # the cap: the walk never keeps more than 50 * nbands, whatever the counts say
    bn[:] = 1000
    sa.merge(bm, bn, bases, msgs, n)
    assert (n <= 150).all() and n[1] == 149


# ---- the .wav reader --------------------------------------------------------------------------------------------------------------

def _wav_bytes(samples, rate=12000, channels=1, bits=16, tag=1, extra=b"", data_size=None):
    body = np.asarray(samples, np.int16).tobytes()
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    data = b"data" + struct.pack("<I", len(body) if data_size is None else data_size) + body
    riff = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + extra + data
    return b"RIFF" + struct.pack("<I", len(riff)) + riff


def test_wav_reader_reads_what_the_wave_module_wrote(ft8, tmp_path):
    pcm = ac.to_s16(np.random.default_rng(8).normal(0, 0.2, 5000))
    path = str(tmp_path / "clip.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(12000)
        w.writeframes(pcm.tobytes())
    assert np.array_equal(ft8.read_wav(path), pcm)
    assert np.array_equal(ft8.read_wav(path, cap=1234), pcm[:1234])         # a cap smaller than the file
    # a LIST chunk and an odd-sized chunk (with its pad byte) in front of data
    extra = b"LIST" + struct.pack("<I", 10) + b"INFOabcdef" + b"odd " + struct.pack("<I", 3) + b"xyz\0"
    (tmp_path / "chunks.wav").write_bytes(_wav_bytes(pcm, extra=extra))
    assert np.array_equal(ft8.read_wav(str(tmp_path / "chunks.wav")), pcm)
    full = np.zeros(200000, np.int16)
    (tmp_path / "long.wav").write_bytes(_wav_bytes(full))
    assert ft8.read_wav(str(tmp_path / "long.wav")).shape == (180000,)


@pytest.mark.parametrize("name,content,says", [
    ("8-bit", _wav_bytes(np.zeros(64, np.int16), bits=8), "8 bit"),
    ("stereo", _wav_bytes(np.zeros(64, np.int16), channels=2), "2 channel"),
    ("11025", _wav_bytes(np.zeros(64, np.int16), rate=11025), "11025 Hz"),
    ("truncated", _wav_bytes(np.zeros(64, np.int16))[:30], "truncated header"),
    ("short-data", _wav_bytes(np.zeros(64, np.int16), data_size=4096), "declares 4096 bytes"),
    ("no-data", _wav_bytes(np.zeros(64, np.int16))[:36], "no data chunk"),
    ("empty", b"", "empty file"),
    ("not-riff", b"OggS" + bytes(60), "not a RIFF/WAVE file"),
])
def test_wav_reader_refuses_with_a_message(ft8, tmp_path, capfd, name, content, says):
    path = str(tmp_path / (name + ".wav"))
    with open(path, "wb") as f:
        f.write(content)
    out = np.full(64, 0x5A5A, np.int16)
    n = np.array([77], np.int32)
    capfd.readouterr()
    assert ft8.load_library().ft8gpu_read_wav(path.encode(), out.ctypes.data, 64, n.ctypes.data_as(C.POINTER(C.c_int32))) == -1
    err = capfd.readouterr().err
    print(err.strip())
    assert says in err and path in err and n[0] == 0 and (out == 0x5A5A).all()
    with pytest.raises(ft8.Ft8GpuError):
        ft8.read_wav(path)


def test_wav_reader_under_asan_ubsan(tmp_path):
    """a program of its own (tests/host_asan/audio_asan_main.c) linked with csrc/ft8_compat.c and csrc/ft8_pack.c; nothing is
    loaded into python"""
    exe = str(tmp_path / "audio_asan")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_asan", "audio_asan_main.c"),
                           os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc", "ft8_compat.c"),
                           os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc", "ft8_pack.c"),
                           "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe, str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "audio_asan ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


def test_wav_example_compiles_against_the_public_header(tmp_path):
    obj = str(tmp_path / "ft8_wav.o")
    subprocess.check_call(["gcc", "-O2", "-std=gnu17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "ft8_wav.c"), "-o", obj])
