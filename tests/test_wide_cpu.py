"""The wideband RX front end without a GPU (include/ft8gpu.h "wideband RX"): the tables of the rule against their formulas and
against the filter bounds, the numpy restatement (tests/ft8_spec_wide.py) in its fast form against the 497-tap definition, at the
integer worst case, on a pure tone and through the CPU oracle, the merge rule on hand-made records, the exported entries, the
example, and the host C file under AddressSanitizer / UBSan as a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import ft8_spec_wide as sw
import wide_craft as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAMES = ("ft8gpu_wide_mixer1", "ft8gpu_wide_mixer2", "ft8gpu_wide_taps", "ft8gpu_wide_frames", "ft8gpu_decode_wide")


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as ft8
    ft8.load_library()
    return ft8


# ---- the tables -------------------------------------------------------------------------------------------------------------------

def test_tables_equal_the_formulas_bit_for_bit(ft8):
    w1, w2, h = ft8.wide_mixer1(), ft8.wide_mixer2(), ft8.wide_taps()
    assert w1.dtype == np.int16 and w1.shape == (6000, 2) and w2.dtype == F32 and w2.shape == (3072, 2) and h.dtype == F32 and h.shape == (96,)
    assert w1.tobytes() == sw.mixer1().tobytes() and w2.tobytes() == sw.mixer2().tobytes() and h.tobytes() == sw.taps().tobytes()
    assert h[95] == 0 and np.array_equal(h[:95], h[94::-1])               # symmetric about index 47
    assert abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6
    i = np.arange(6000)
    assert np.abs(w1[:, 0] - 32767 * np.cos(2 * np.pi * i / 6000)).max() <= 0.5 + 1e-6
    assert np.abs(w1[:, 1] + 32767 * np.sin(2 * np.pi * i / 6000)).max() <= 0.5 + 1e-6
    assert tuple(w1[0]) == (32767, 0) and tuple(w1[1500]) == (0, -32767) and np.abs(w1.astype(np.int32)).max() == 32767
    lib = ft8.load_library()
    for name in NAMES[:3]:
        getattr(lib, name)(None)                                          # a NULL table is ignored
    assert float(sw.C0) == float(F32(1.0 / (32767.0 * 125.0 ** 4 * 128.0)))


def test_cic_taps_are_symmetric_and_sum_to_125_to_the_fourth():
    g = sw.cic_taps()
    assert g.shape == (497,) and np.array_equal(g, g[::-1]) and int(g.sum()) == 125 ** 4 and g[0] == 1 and g[248] == g.max()


def test_chain_meets_the_filter_bounds(ft8):
    """float taps at 19 200 sps times the exact response of g at 2.4 Msps, every 1.5625 Hz over the whole capture, the channel's
    residual offset 6.25 q Hz between the two: at most -80 dB at or beyond 2400 Hz from the band's centre, within +-0.06 dB up
    to 800 Hz"""
    h = ft8.wide_taps().astype(np.float64)[:95]
    f = np.arange(-1200000.0, 1200000.0, 1.5625)
    k = np.arange(95) - 47
    hf = np.empty_like(f)
    for i in range(0, f.size, 1 << 17):
        hf[i:i + (1 << 17)] = np.abs(np.exp(-2j * np.pi * np.outer(f[i:i + (1 << 17)], k) / 19200.0) @ h)

    def g_resp(ff):
        x = np.pi * ff / 2.4e6
        s = np.sin(x)
        with np.errstate(all="ignore"):
            r = np.where(np.abs(s) < 1e-12, 1.0, np.sin(125 * x) / (125 * s))
        return r ** 4

    for q in (-32, 0, 31):
        db = 20 * np.log10(np.maximum(np.abs(g_resp(f + 6.25 * q)) * hf, 1e-300))
        stop, lo, hi = db[np.abs(f) >= 2400].max(), db[np.abs(f) <= 800].min(), db[np.abs(f) <= 800].max()
        print(f"q {q}: stopband {stop:.2f} dB, passband {lo:+.5f} .. {hi:+.5f} dB")
        assert stop <= -80.0 and lo >= -0.06 and hi <= 0.06


def test_entries_are_exported_and_refuse_a_null_context(ft8):
    lib = ft8.load_library()
    for name in NAMES:
        assert name in ft8.ABI_SYMBOLS and hasattr(lib, name)
    assert lib.ft8gpu_wide_frames(None, None, 1, 8, None, 1, None, 0, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_decode_wide(None, None, 1, 8, None, 1, None, None, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()


# ---- stage A ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [-2748, -7, 0, 5, 2752])
def test_fast_form_is_the_497_tap_definition(c):
    raw = wc.random_capture(2000, 1)
    v = sw.stage_a(raw, c)
    assert v.shape == (2, sw.last_m(2000) + 2) and np.array_equal(v, sw.stage_a_direct(raw, c, np.arange(-1, v.shape[1] - 1)))
    assert v[:, 0].any() and v[:, -1].any()                                # m = -1 and the last m hold samples
    assert not sw.stage_a_direct(raw, c, [-2, sw.last_m(2000) + 1]).any()  # and their neighbours none


def test_worst_case_stays_exact():
    """all bytes 0x00 with c = 0: x = -128 - 128 i, w1[0] = 32767, so a full window gives -128 * 32767 * 125^4, near 2^50, in
    both components, and the cumulative sums wrap on the way"""
    raw = np.zeros(2 * 48000, np.uint8)
    v = sw.stage_a(raw, 0)
    full = -128 * 32767 * 125 ** 4
    assert 2 ** 49 < -full < 2 ** 52 and (v[:, 3:-4] == full).all()
    assert np.array_equal(v[:, :6], sw.stage_a_direct(raw, 0, np.arange(-1, 5)))
    x = sw.stage_b(v, 0)
    assert np.all(np.abs(np.abs(x[:, 10:55]) - 1.0) < 1e-5)                # 128/128 after c0 and the taps' unit sum


def test_a_full_scale_tone_arrives_at_its_bin_with_its_amplitude():
    freq_bin, npairs = 12345, 1200000
    assert sw.channel(freq_bin) == (195, -7)
    t = np.arange(npairs) / 2.4e6
    raw = wc.to_bytes(127.0 * np.exp(2j * np.pi * (6.25 * freq_bin + 1000.0) * t))
    x = sw.frame(raw, freq_bin)
    spec = np.fft.fft((x[0] + 1j * x[1])[512:1024])
    k = int(np.argmax(np.abs(spec)))
    db = 20 * np.log10(np.abs(spec[k]) / 512 / (127.0 / 128.0))
    print(f"peak at bin {k}, {db:+.4f} dB from 127/128")
    assert k == 160 and abs(db) <= 0.06


@pytest.fixture(scope="module")
def two_signal_frames(oracle):
    """one 15 s capture, two signals at amplitude 20 in two channels over noise of sigma 30, quantised to bytes"""
    rng = np.random.default_rng(11)
    planted = (("CQ K1ABC FN42", 48000, 500.0, 0.5), ("CQ DL1XYZ JO62", -66000, 1000.0, 0.8))
    x = rng.normal(0, 30.0, 2 * sw.MAX_PAIRS).astype(np.float32).view(np.complex64).astype(np.complex128)
    for text, fb, f0, t0 in planted:
        rc, payload = oracle.pack77(text)
        assert rc == 0
        x += wc.cpfsk(oracle.encode(payload[:10]), 6.25 * fb + f0, t0, sw.MAX_PAIRS, 20.0)
    raw = wc.to_bytes(x)
    return planted, sw.frames(raw[None], [fb for _, fb, _, _ in planted], normalise=True)[0]


def test_restated_frames_decode_in_the_oracle(oracle, two_signal_frames):
    planted, frames = two_signal_frames
    for b, (text, fb, f0, _) in enumerate(planted):
        dec, n = oracle.subsystem(frames[b, 0], frames[b, 1])
        got = {f"CQ {dec[k]['call'].decode()} {dec[k]['loc'].decode()}": int(dec[k]["freq"]) for k in range(n)}
        print(f"channel {fb}: {got}")
        assert got == {text: int(f0)}


# ---- the merge rule ---------------------------------------------------------------------------------------------------------------

def test_merge_rule_on_hand_made_records(ft8):
    rng = np.random.default_rng(3)
    bins = (48000, 48240, 48256, -66000)
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
    sw.merge(bm, bn, bins, msgs, n)
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
    assert float(neg["freq_hz"]) == (int(neg["cand"]["freq_offset"]) - 66000 + int(neg["cand"]["freq_sub"]) / 2) * 6.25      # exact
    bn[:] = 1000                                                           # the cap: never more than 50 * nchannels
    sw.merge(bm, bn, bins, msgs, n)
    assert n[0] <= 200


# ---- the host C file and the example ----------------------------------------------------------------------------------------------

def test_host_file_under_asan_ubsan(tmp_path):
    """a program of its own (tests/host_asan/wide_asan_main.c) linked with csrc/ft8_wide.c; nothing is loaded into python"""
    exe = str(tmp_path / "wide_asan")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_asan", "wide_asan_main.c"),
                           os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc", "ft8_wide.c"), "-lm", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "wide_asan ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


def test_wide_example_compiles_against_the_public_header(tmp_path):
    obj = str(tmp_path / "ft8_wide.o")
    subprocess.check_call(["gcc", "-O2", "-std=gnu17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "ft8_wide.c"), "-o", obj])
