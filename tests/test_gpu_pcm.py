"""GPU tests of the PCM front end (ft8gpu_pcm_frames, ft8gpu_decode_pcm) against the numpy restatement tests/ft8_spec_pcm.py,
byte for byte: the stage at every rate and in every format on random samples, at the lengths that sit on the edges of the
kernel's tiles, on the channels that reach every branch of the channel arithmetic, with 1, 2, 3 and 16 channels, host and device
pointers (the device form from a capture that starts at an odd element), guard bands around the device form's outputs; runs
that straddle captures; contexts of 8, 4 and 1 frames; the special captures; two full-length captures; the whole path on a 48
ksps capture built in numpy; the refusals; and the existing entries before and after PCM calls on one context."""
import numpy as np
import pytest

import ft8_spec_pcm as sp
import pcm_craft as pc

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xA5


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def guarded(a):
    """a device copy of a's bytes between two guard bands of FILL"""
    import torch
    a = np.ascontiguousarray(a)
    b = torch.full((GUARD + a.nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    b[GUARD:GUARD + a.nbytes] = up(a)
    return b


def unguard(b, nbytes):
    h = b.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + nbytes:] == FILL).all(), "a guard band was written"
    return h[GUARD:GUARD + nbytes].copy()


def filled_msgs(ft8, ncap, nch):
    return np.full((ncap, 50 * nch * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(ncap, 50 * nch)


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as ft8
    ft8.check_build_id()
    return ft8


@pytest.fixture(scope="module")
def dec4(ft8):
    with ft8.Decoder(device=0, max_frames=4) as dec:
        yield dec


def frames_dev(dec, pcm, fmt, D, bins, normalise=False):
    """the device form between guard bands; the captures start one element into their allocation, so at an address that is
    aligned to the sample type and to nothing more -> iq [ncap][nch][2][48000]"""
    import torch
    ncap = pcm.shape[0]
    nsamples = pcm.shape[1] // (2 if fmt & sp.COMPLEX else 1)
    out = np.zeros((ncap, len(bins), 2, sp.NSAMPLES), np.float32)
    item = pcm.dtype.itemsize
    p_d = up(np.concatenate([np.zeros(1, pcm.dtype), pcm.reshape(-1)]))
    o_b = guarded(out)
    assert o_b[GUARD:].data_ptr() % 16 == 0
    torch.cuda.synchronize()
    dec.pcm_frames_dev(p_d.data_ptr() + item, fmt, sp.rate_of(D), ncap, nsamples, bins, o_b[GUARD:].data_ptr(), normalise)
    dec.synchronize()
    return unguard(o_b, out.nbytes).view(np.float32).reshape(out.shape)


def frames_host(dec, pcm, fmt, D, bins, normalise=False):
    return dec.pcm_frames(pcm, sp.rate_of(D), bins, complex_iq=bool(fmt & sp.COMPLEX), normalise=normalise)


def both_forms(dec, pcm, fmt, D, bins, normalise=False):
    yield "host", frames_host(dec, pcm, fmt, D, bins, normalise)
    yield "device", frames_dev(dec, pcm, fmt, D, bins, normalise)


def same_bytes(got, ref, what):
    d = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(ref).view(np.uint32))
    assert len(d) == 0, f"{what}: {len(d)} values differ, the first at {d[0].tolist()}: {got[tuple(d[0])]!r} != {ref[tuple(d[0])]!r}"


def same_but_nans(got, ref, what):
    """NaN positions equal, every other value the same bytes"""
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaNs at other places"
    same_bytes(np.where(gn, np.float32(0), got), np.where(rn, np.float32(0), ref), what)


def restated(pcm, fmt, D, bins, normalise=False):
    """[ncap][nch][2][48000], every (capture, freq_bin) computed once"""
    memo = {}
    out = np.zeros((pcm.shape[0], len(bins), 2, sp.NSAMPLES), np.float32)
    for k in range(pcm.shape[0]):
        for b, fb in enumerate(bins):
            if (k, fb) not in memo:
                memo[k, fb] = sp.frame(pcm[k], fmt, D, fb, normalise)
            out[k, b] = memo[k, fb]
    return out


# ---- stage parity -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", pc.FORMATS, ids=[pc.FORMAT_NAMES[f] for f in pc.FORMATS])
@pytest.mark.parametrize("D", sp.DS)
def test_stage_is_the_restatement_byte_for_byte(dec4, D, fmt):
    """two captures of random samples per length: 1, M, 4 M + 1, one sample either side of a tile of the planes kernel, 19997; 1,
    2, 3 and 16 channels that give q = 0, -16 and 15, a negative c (complex), freq_bin 0 (real) and the ends of the range; both
    pointer forms"""
    for nsamples in pc.lengths(D):
        pcm = np.stack([pc.random_capture(fmt, nsamples, 10 + k) for k in range(2)])
        sixteen = pc.sixteen(D, fmt)
        ref16 = restated(pcm, fmt, D, sixteen)
        assert ref16.any()
        for bins in pc.channel_lists(D, fmt):
            ref = ref16[:, [sixteen.index(b) for b in bins]]
            for form, got in both_forms(dec4, pcm, fmt, D, bins):
                assert got.shape == ref.shape
                same_bytes(got, ref, f"{form} form, D {D}, {pc.FORMAT_NAMES[fmt]}, {nsamples} samples, channels {bins}")


def test_runs_straddle_captures(ft8, dec4):
    """three captures of three channels in a context of four frames: the pieces are frames 0-3, 4-7 and 8"""
    fmt, D = sp.S16 | sp.COMPLEX, 30
    pcm = np.stack([pc.random_capture(fmt, 6001, 20 + k) for k in range(3)])
    bins = (-48, -177, 3000)
    ref = restated(pcm, fmt, D, bins)
    for form, got in both_forms(dec4, pcm, fmt, D, bins):
        same_bytes(got, ref, f"{form} form")
    out = {}
    for mf in (8, 4, 1):
        with ft8.Decoder(device=0, max_frames=mf) as dec:
            out[mf] = [got.tobytes() for _, got in both_forms(dec, pcm, fmt, D, bins)]
    assert out[8][0] == out[8][1] == ref.tobytes() and out[4] == out[8] and out[1] == out[8]


# ---- special captures -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", pc.FORMATS, ids=[pc.FORMAT_NAMES[f] for f in pc.FORMATS])
def test_capture_with_its_first_and_last_sample_alone(dec4, fmt):
    for D, nsamples in ((15, 2001), (240, 30001)):
        pcm = pc.ends_capture(fmt, nsamples)[None]
        bins = pc.edge_bins(D, fmt)[:3]
        ref = restated(pcm, fmt, D, bins)
        assert ref[0, :, :, 0].any() and np.count_nonzero(ref) < 3 * 2 * 64
        for form, got in both_forms(dec4, pcm, fmt, D, bins):
            same_bytes(got, ref, f"{form} form, D {D}")


@pytest.mark.parametrize("normalise", [False, True])
def test_silent_capture_gives_plus_zero_everywhere(dec4, normalise):
    for fmt in pc.FORMATS:
        pcm = np.zeros((1, pc.nelements(fmt, 5000)), np.float32 if fmt & sp.F32FMT else np.int16)
        for form, got in both_forms(dec4, pcm, fmt, 60, pc.edge_bins(60, fmt), normalise):
            assert not got.view(np.uint32).any(), (form, fmt)              # +0: no sign bit either


@pytest.mark.parametrize("normalise", [False, True])
def test_full_scale_negative_s16(dec4, normalise):
    """every sample -32768: x = -1 (- i), the filters' unit sums give a plateau of magnitude 1 at c = 0"""
    for fmt in (sp.S16, sp.S16 | sp.COMPLEX):
        pcm = np.full((1, pc.nelements(fmt, 19997)), -32768, np.int16)
        bins = (-128, -97) if fmt & sp.COMPLEX else (0, 47)
        D = 15
        ref = restated(pcm, fmt, D, bins, normalise)
        if fmt & sp.COMPLEX and not normalise:
            assert abs(float(np.abs(ref[0, 0, :, 100:1000]).max()) - 1.0) < 1e-4
        for form, got in both_forms(dec4, pcm, fmt, D, bins, normalise):
            same_bytes(got, ref, f"{form} form, {pc.FORMAT_NAMES[fmt]}")


def test_f32_nan_infinity_and_subnormals_are_kept(dec4):
    """NaN, +-infinity and subnormals at known places of a float capture: the NaN positions are those of the rule, every other
    value is the same bytes"""
    for fmt in (sp.F32FMT, sp.F32FMT | sp.COMPLEX):
        D = 30
        pcm = pc.random_capture(fmt, 19997, 60)[None].copy()
        pcm[0, 3000], pcm[0, 9000], pcm[0, 9001], pcm[0, 15000] = np.nan, np.inf, -np.inf, np.float32(1e-40)
        pcm[0, 17000:17400] = np.float32(3e-42) * np.arange(400, dtype=np.float32)
        bins = pc.edge_bins(D, fmt)[:3]
        ref = restated(pcm, fmt, D, bins)
        assert np.isnan(ref).any() and not np.isnan(ref).all()
        for form, got in both_forms(dec4, pcm, fmt, D, bins):
            same_but_nans(got, ref, f"{form} form, {pc.FORMAT_NAMES[fmt]}")
    # subnormals alone: outputs that are subnormal themselves, not flushed
    pcm = (np.float32(1e-39) * np.random.default_rng(61).normal(0, 1, (1, 4001))).astype(np.float32)
    ref = restated(pcm, sp.F32FMT, 15, (0, 47))
    tiny = np.abs(ref[ref != 0])
    assert tiny.size and tiny.max() < np.finfo(np.float32).tiny
    for form, got in both_forms(dec4, pcm, sp.F32FMT, 15, (0, 47)):
        same_bytes(got, ref, f"{form} form, subnormals")


def test_normalise_is_the_peak_rule(dec4):
    fmt, D = sp.S16 | sp.COMPLEX, 60
    pcm = pc.random_capture(fmt, 19997, 31)[None]
    bins = (3000, -9000)
    ref = restated(pcm, fmt, D, bins, True)
    for form, got in both_forms(dec4, pcm, fmt, D, bins, True):
        same_bytes(got, ref, f"{form} form")
        assert np.allclose(np.abs(got).max(axis=(2, 3)), 0.5, rtol=0, atol=1e-6)


# ---- full length ------------------------------------------------------------------------------------------------------------------

def test_full_length_capture_at_48_ksps(dec4):
    """720 000 complex int16 samples, two channels, all 48000 outputs of both, byte for byte"""
    fmt, D = sp.S16 | sp.COMPLEX, 15
    pcm = pc.random_capture(fmt, sp.max_samples(D), 40)[None]
    bins = (1000, -3000)
    ref = restated(pcm, fmt, D, bins)
    assert ref[0, :, :, -1].all()
    same_bytes(frames_dev(dec4, pcm, fmt, D, bins), ref, "device form")
    same_bytes(frames_host(dec4, pcm, fmt, D, bins), ref, "host form")


def test_full_length_capture_at_768_ksps(dec4):
    """11 520 000 complex float samples, one channel, all 48000 outputs, byte for byte"""
    fmt, D = sp.F32FMT | sp.COMPLEX, 240
    pcm = pc.random_capture(fmt, sp.max_samples(D), 41)[None]
    bins = (-40001,)
    ref = restated(pcm, fmt, D, bins)
    assert ref[0, :, :, -1].all()
    same_bytes(frames_dev(dec4, pcm, fmt, D, bins), ref, "device form")
    same_bytes(frames_host(dec4, pcm, fmt, D, bins), ref, "host form")


# ---- the whole path ---------------------------------------------------------------------------------------------------------------

CHANNELS = (0, 240, 1500)
# text, Hz on the audio axis, start (s), the channel that reports it
PLANTED = (("CQ K1ABC FN42", 500.0, 0.5, 0), ("CQ JA1AAA PM95", 2000.0, 0.3, 1), ("CQ DL1XYZ JO62", 9800.0, 0.8, 2))


def real_capture(oracle):
    """15 s of real audio at 48 ksps: three CPFSK signals over noise, as int16"""
    n = sp.max_samples(15)
    x = np.random.default_rng(5).normal(0, 0.05, n)
    for text, f0, t0, _ in PLANTED:
        rc, payload = oracle.pack77(text)
        assert rc == 0
        x += pc.cpfsk(oracle.encode(payload[:10]), f0, t0, n, 0.03, 48000).real
    return pc.to_s16(x)


def decode_dev(ft8, dec, pcm, fmt, D, bins):
    """the whole path's device form between guard bands -> (msgs, n_msgs)"""
    import torch
    ncap = pcm.shape[0]
    nsamples = pcm.shape[1] // (2 if fmt & sp.COMPLEX else 1)
    fill = filled_msgs(ft8, ncap, len(bins))
    p_d = up(pcm)
    m_b, n_b = guarded(fill), guarded(np.zeros(ncap, np.int32))
    torch.cuda.synchronize()
    dec.decode_pcm_dev(p_d, fmt, sp.rate_of(D), ncap, nsamples, bins, m_b[GUARD:].data_ptr(), n_b[GUARD:].data_ptr())
    dec.synchronize()
    return unguard(m_b, fill.nbytes).view(ft8.MESSAGE_DTYPE).reshape(fill.shape), unguard(n_b, 4 * ncap).view(np.int32)


def test_whole_path_is_decode_messages_and_the_merge(ft8, dec4, oracle):
    import torch
    cap = real_capture(oracle)
    pcm = np.stack([cap, np.zeros_like(cap)])                              # the capture and a silent one
    nch = len(CHANNELS)
    iq = torch.zeros((2 * nch, 2, sp.NSAMPLES), dtype=torch.float32, device="cuda")
    dec4.pcm_frames_dev(up(pcm), sp.S16, 48000, 2, cap.shape[0], CHANNELS, iq, True)
    cm = torch.zeros(2 * nch * 50 * 64, dtype=torch.uint8, device="cuda")
    cn = torch.zeros(2 * nch, dtype=torch.int32, device="cuda")
    dec4.decode_messages_dev(iq, 2 * nch, cm, cn)
    dec4.synchronize()
    bm = cm.cpu().numpy().view(ft8.MESSAGE_DTYPE).reshape(2, nch, 50)
    bn = cn.cpu().numpy().reshape(2, nch)
    want_m, want_n = sp.merge(bm, bn, CHANNELS, filled_msgs(ft8, 2, nch), np.zeros(2, np.int32))
    got_m, got_n = decode_dev(ft8, dec4, pcm, sp.S16, 15, CHANNELS)
    assert got_n.tolist() == want_n.tolist() and got_m.tobytes() == want_m.tobytes()
    host_m, host_n = dec4.decode_pcm(pcm, 48000, CHANNELS, msgs=filled_msgs(ft8, 2, nch))
    assert host_n.tolist() == want_n.tolist() and host_m.tobytes() == want_m.tobytes()
    recs = got_m[0, :int(got_n[0])]
    texts = [pc.text_of(r) for r in recs]
    print(texts, [float(r["freq_hz"]) for r in recs], [int(r["pad"][0]) for r in recs], bn.tolist())
    # each planted signal exactly once, on the audio axis
    assert sorted(texts) == sorted(t for t, _, _, _ in PLANTED)
    for text, f0, _, chan in PLANTED:
        mine = [r for r, t in zip(recs, texts) if t == text]
        assert len(mine) == 1, text
        assert abs(float(mine[0]["freq_hz"]) - f0) <= 3.125
    assert got_n[1] == 0


def test_one_signal_in_two_overlapping_channels_is_kept_once(ft8, dec4, oracle):
    """channels 0 and 80 (0 and 500 Hz) both hold the signal at 1000 Hz: both decode it, the merge keeps the first"""
    n = sp.max_samples(15)
    rc, payload = oracle.pack77("CQ K1ABC FN42")
    assert rc == 0
    x = np.random.default_rng(6).normal(0, 0.05, n) + pc.cpfsk(oracle.encode(payload[:10]), 1000.0, 0.5, n, 0.03, 48000).real
    pcm = pc.to_s16(x)[None]
    bins = (0, 80)
    iq = dec4.pcm_frames(pcm, 48000, bins, normalise=True)
    bm, bn = dec4.decode_messages(iq.reshape(2, 2, sp.NSAMPLES))
    bm, bn = bm.reshape(1, 2, 50), bn.reshape(1, 2)
    assert bn.tolist() == [[1, 1]] and pc.text_of(bm[0, 0, 0]) == pc.text_of(bm[0, 1, 0]) == "CQ K1ABC FN42"
    want_m, want_n = sp.merge(bm, bn, bins, filled_msgs(ft8, 1, 2), np.zeros(1, np.int32))
    got_m, got_n = decode_dev(ft8, dec4, pcm, sp.S16, 15, bins)
    assert got_n.tolist() == want_n.tolist() == [1] and got_m.tobytes() == want_m.tobytes()
    assert got_m[0, 0]["pad"][0] == 0 and abs(float(got_m[0, 0]["freq_hz"]) - 1000.0) <= 3.125


def test_a_context_of_one_frame_decodes_sixteen_channels(ft8, oracle):
    n = 200000                                                             # 4.2 s: no message, but every channel goes through
    pcm = pc.random_capture(sp.S16, n, 7)[None]
    bins = pc.sixteen(15, sp.S16)
    with ft8.Decoder(device=0, max_frames=1) as dec:
        msgs, cnt = dec.decode_pcm(pcm, 48000, bins, msgs=filled_msgs(ft8, 1, 16))
    assert cnt.tolist() == [0] and (msgs.view(np.uint8) == FILL).all()


def test_example_decodes_a_written_wav(tmp_path, oracle):
    """examples/ft8_pcm.c built against the library and run on a 48 kHz one-channel .wav: the default channels 0 and 1500 Hz"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.join(root, "rtlsdr_ft8d_amd")
    exe, wav = str(tmp_path / "ft8_pcm"), tmp_path / "capture.wav"
    subprocess.check_call(["gcc", "-O2", "-std=gnu17", "-Wall", "-Wextra", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "ft8_pcm.c"), "-L", lib_dir, "-lft8gpu", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    wav.write_bytes(pc.wav_bytes(real_capture(oracle).tobytes(), 48000, 1, 1, 16))
    out = subprocess.run([exe, str(wav)], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "720000 real samples at 48000 Hz" in out.stdout and "2 messages" in out.stdout
    assert "CQ K1ABC FN42" in out.stdout and "CQ JA1AAA PM95" in out.stdout
    bad = tmp_path / "bad.wav"
    bad.write_bytes(pc.wav_bytes(bytes(64), 44100, 1, 1, 16))
    out = subprocess.run([exe, str(bad)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "44100 Hz" in out.stderr


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_arguments_are_refused_with_their_text_and_outputs_stay(ft8, dec4):
    import torch
    lib = ft8.load_library()
    cplx, real = sp.S16 | sp.COMPLEX, sp.S16
    pcm = pc.random_capture(cplx, 752, 3)[None]
    iq = np.full((1, 16, 2, sp.NSAMPLES), np.float32(-7.5), np.float32)
    msgs, n = filled_msgs(ft8, 1, 16), np.full(1, -9, np.int32)
    keep_m = msgs.tobytes()

    def bins(*b):
        return np.array(b, np.int32)

    one = bins(0)
    cases = [  # (pcm, format, rate, nsamples, freq_bin, nchannels, iq / msgs present, text)
        (pcm, cplx, 48000, 752, one, 0, True, "nchannels 0 out of range [1, 16]"),
        (pcm, cplx, 48000, 752, bins(*range(17)), 17, True, "nchannels 17 out of range [1, 16]"),
        (pcm, 4, 48000, 752, one, 1, True, "unknown PCM format 4"), (pcm, -1, 48000, 752, one, 1, True, "unknown PCM format -1"),
        (pcm, cplx, 44100, 752, one, 1, True, "rate 44100 is not one of 48000, 96000, 192000, 384000, 768000"),
        (pcm, cplx, 12000, 752, one, 1, True, "rate 12000 is not one of"), (pcm, cplx, 0, 752, one, 1, True, "rate 0 is not one of"),
        (pcm, cplx, 48000, 752, bins(0, 3585), 2, True, "freq_bin[1] = 3585 out of range [-3840, 3584]"),
        (pcm, cplx, 48000, 752, bins(-3841), 1, True, "freq_bin[0] = -3841 out of range [-3840, 3584]"),
        (pcm, real, 48000, 752, bins(-1), 1, True, "freq_bin[0] = -1 out of range [0, 3584]"),
        (pcm, cplx, 768000, 752, bins(61185), 1, True, "freq_bin[0] = 61185 out of range [-61440, 61184]"),
        (pcm, cplx, 48000, 0, one, 1, True, "nsamples 0 out of range [1, 720000]"),
        (pcm, cplx, 48000, 720001, one, 1, True, "nsamples 720001 out of range [1, 720000]"),
        (pcm, cplx, 768000, 11520001, one, 1, True, "nsamples 11520001 out of range [1, 11520000]"),
        (pcm, cplx, 48000, 752, None, 1, True, "NULL array argument"), (None, cplx, 48000, 752, one, 1, True, "NULL array argument"),
        (pcm, cplx, 48000, 752, one, 1, False, "NULL array argument")]
    for r, fmt, rate, ns, b, nb, outs, text in cases:
        rp = None if r is None else r.ctypes.data
        bp = None if b is None else b.ctypes.data
        rc = lib.ft8gpu_pcm_frames(dec4.h, rp, fmt, rate, 1, ns, bp, nb, iq.ctypes.data if outs else None, 0, ft8.HOST_PTRS)
        assert rc == -1 and text in lib.ft8gpu_last_error().decode(), (text, lib.ft8gpu_last_error())
        rc = lib.ft8gpu_decode_pcm(dec4.h, rp, fmt, rate, 1, ns, bp, nb, msgs.ctypes.data if outs else None, n.ctypes.data, ft8.HOST_PTRS)
        assert rc == -1 and text in lib.ft8gpu_last_error().decode(), (text, lib.ft8gpu_last_error())
        assert (iq == np.float32(-7.5)).all() and msgs.tobytes() == keep_m and (n == -9).all()
    # a pointer that is not aligned to its sample type, in the device form
    r_d, o_b = up(np.concatenate([np.zeros(2, np.int16), pcm[0]])), guarded(iq[:, :1])
    m_b, n_b = guarded(msgs[:, :50]), guarded(n)
    torch.cuda.synchronize()
    rc = lib.ft8gpu_pcm_frames(dec4.h, r_d.data_ptr() + 1, cplx, 48000, 1, 752, one.ctypes.data, 1, o_b[GUARD:].data_ptr(), 0, ft8.DEVICE_PTRS)
    assert rc == -1 and "pcm must be aligned to its sample type" in lib.ft8gpu_last_error().decode()
    rc = lib.ft8gpu_decode_pcm(dec4.h, r_d.data_ptr() + 1, cplx, 48000, 1, 752, one.ctypes.data, 1, m_b[GUARD:].data_ptr(),
                               n_b[GUARD:].data_ptr(), ft8.DEVICE_PTRS)
    assert rc == -1 and "pcm must be aligned to its sample type" in lib.ft8gpu_last_error().decode()
    rc = lib.ft8gpu_pcm_frames(dec4.h, r_d.data_ptr(), cplx, 48000, 1, 752, one.ctypes.data, 1, o_b[GUARD:].data_ptr() + 4, 0, ft8.DEVICE_PTRS)
    assert rc == -1 and "iq must be 16-byte aligned" in lib.ft8gpu_last_error().decode()
    dec4.synchronize()
    assert (unguard(o_b, iq[:, :1].nbytes).view(np.float32) == np.float32(-7.5)).all()
    assert unguard(m_b, msgs[:, :50].nbytes).tobytes() == msgs[:, :50].tobytes() and (unguard(n_b, 4).view(np.int32) == -9).all()
    # a valid call follows
    same_bytes(dec4.pcm_frames(pcm, 48000, (0, 3584), complex_iq=True), restated(pcm, cplx, 15, (0, 3584)), "after the refusals")
    _, cnt = dec4.decode_pcm(pcm, 48000, (0,), complex_iq=True)
    assert cnt.tolist() == [0]


# ---- the existing entries ---------------------------------------------------------------------------------------------------------

def test_existing_entries_are_unchanged_by_pcm_calls(ft8, oracle):
    """decode_messages, audio_frames and wide_frames on fixed inputs before and after PCM calls on the same, fresh context: the
    buffers of the PCM path are allocated by the calls in between and stay with the context"""
    i, q = oracle.selftest_signal()
    iq = np.stack([np.stack([i, q]), np.random.default_rng(2).normal(0, 0.1, (2, sp.NSAMPLES)).astype(np.float32)])
    audio = np.random.default_rng(3).integers(-2000, 2000, (2, 30000)).astype(np.int16)
    wide = np.random.default_rng(4).integers(0, 256, (2, 2 * 48000), dtype=np.uint8)
    pcm = np.stack([pc.random_capture(sp.S16 | sp.COMPLEX, 19997, 50 + k) for k in range(2)])
    with ft8.Decoder(device=0, max_frames=4) as dec:
        def existing():
            m, n = dec.decode_messages(iq, msgs=filled_msgs(ft8, 2, 1))
            return m.tobytes(), n.tobytes(), dec.audio_frames(audio, (0, 240)).tobytes(), dec.wide_frames(wide, (0, 48000)).tobytes()
        e0 = existing()
        _, cnt = dec.decode_pcm(pcm, 48000, (0, 240, -3000), complex_iq=True)
        assert cnt.tolist() == [0, 0]
        e1 = existing()
        dec.pcm_frames(pcm, 768000, pc.sixteen(240, sp.S16 | sp.COMPLEX), complex_iq=True)
        e2 = existing()
    assert np.frombuffer(e0[1], np.int32)[0] >= 1 and e0 == e1 == e2
