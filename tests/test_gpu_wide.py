"""GPU tests of the wideband RX front end (ft8gpu_wide_frames, ft8gpu_decode_wide) against the numpy restatement
tests/ft8_spec_wide.py, byte for byte: the stage on random bytes at four lengths, on the channels that reach every branch of the
channel arithmetic, with 1, 2, 3 and 16 channels, host and device pointers, guard bands around the device form's outputs; runs
that straddle captures; contexts of 8, 4 and 1 frames; the special captures; one full-length capture; the whole path on a
capture built on the device; the refusals; and the existing entries before and after wide calls on one context."""
import numpy as np
import pytest

import ft8_spec_wide as sw
import wide_craft as wc

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


def frames_dev(dec, raw, bins, normalise=False):
    """the device form between guard bands: raw uint8 [ncap][2 npairs] on the host or a device tensor -> iq [ncap][nch][2][48000]"""
    import torch
    ncap, nbytes = raw.shape
    out = np.zeros((ncap, len(bins), 2, sw.NSAMPLES), np.float32)
    r_d = raw if isinstance(raw, torch.Tensor) else up(raw)
    o_b = guarded(out)
    assert r_d.data_ptr() % 16 == 0 and o_b[GUARD:].data_ptr() % 16 == 0
    torch.cuda.synchronize()
    dec.wide_frames_dev(r_d, ncap, nbytes // 2, bins, o_b[GUARD:].data_ptr(), normalise)
    dec.synchronize()
    return unguard(o_b, out.nbytes).view(np.float32).reshape(out.shape)


def decode_dev(ft8, dec, raw, bins):
    """the whole path's device form between guard bands -> (msgs, n_msgs)"""
    import torch
    ncap, nbytes = raw.shape
    fill = filled_msgs(ft8, ncap, len(bins))
    r_d = raw if isinstance(raw, torch.Tensor) else up(raw)
    m_b, n_b = guarded(fill), guarded(np.zeros(ncap, np.int32))
    torch.cuda.synchronize()
    dec.decode_wide_dev(r_d, ncap, nbytes // 2, bins, m_b[GUARD:].data_ptr(), n_b[GUARD:].data_ptr())
    dec.synchronize()
    return unguard(m_b, fill.nbytes).view(ft8.MESSAGE_DTYPE).reshape(fill.shape), unguard(n_b, 4 * ncap).view(np.int32)


def same_bytes(got, ref, what):
    d = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(ref).view(np.uint32))
    assert len(d) == 0, f"{what}: {len(d)} values differ, the first at {d[0].tolist()}: {got[tuple(d[0])]!r} != {ref[tuple(d[0])]!r}"


_restated = {}


def restated(raw, key, fb, normalise=False):
    """sw.frame of one capture and channel, computed once per (key, freq_bin, normalise)"""
    k = (key, int(fb), bool(normalise))
    if k not in _restated:
        _restated[k] = sw.frame(raw, int(fb), normalise)
        _restated[k].setflags(write=False)
    return _restated[k]


def both_forms(dec, raw, bins, normalise=False):
    yield "host", dec.wide_frames(raw, bins, normalise)
    yield "device", frames_dev(dec, raw, bins, normalise)


# ---- stage parity -----------------------------------------------------------------------------------------------------------------

CHANNEL_LISTS = ((-128,), (6240, -3297), (176000, -176000, -128), wc.SIXTEEN)


@pytest.mark.parametrize("npairs", wc.LENGTHS)
def test_stage_is_the_restatement_byte_for_byte(dec4, npairs):
    """two captures of random bytes (0 and 255 among them) per length; 1, 2, 3 and 16 channels that give c = 0 with q = 0,
    q = -32, q = 31, a negative c and both ends of the range; both pointer forms"""
    raw = np.stack([wc.random_capture(npairs, 10 + k) for k in range(2)])
    assert raw.min() == 0 and raw.max() == 255
    for bins in CHANNEL_LISTS:
        ref = np.stack([np.stack([restated(raw[k], (npairs, k), fb) for fb in bins]) for k in range(2)])
        assert ref.any()
        for form, got in both_forms(dec4, raw, bins):
            assert got.shape == ref.shape
            same_bytes(got, ref, f"{form} form, {npairs} pairs, channels {bins}")


def test_runs_straddle_captures(ft8, dec4):
    """three captures of three channels in a context of four frames: the pieces are frames 0-3, 4-7 and 8"""
    raw = np.stack([wc.random_capture(48000, 20 + k) for k in range(3)])
    bins = (6240, -3297, 48000)
    ref = sw.frames(raw, bins)
    for form, got in both_forms(dec4, raw, bins):
        same_bytes(got, ref, f"{form} form")
    out = {}
    for mf in (8, 4, 1):
        with ft8.Decoder(device=0, max_frames=mf) as dec:
            out[mf] = [got.tobytes() for _, got in both_forms(dec, raw, bins)]
    assert out[8][0] == out[8][1] == ref.tobytes() and out[4] == out[8] and out[1] == out[8]


# ---- special captures -------------------------------------------------------------------------------------------------------------

def test_capture_with_its_first_and_last_pair_alone(dec4):
    for npairs in (752, 192008):
        raw = wc.ends_capture(npairs)[None]
        bins = (-128, 6240, -3297)
        ref = sw.frames(raw, bins)
        assert ref[0, :, :, 0].any() and np.count_nonzero(ref) < 3 * 2 * 64
        for form, got in both_forms(dec4, raw, bins):
            same_bytes(got, ref, f"{form} form, {npairs} pairs")


@pytest.mark.parametrize("normalise", [False, True])
def test_silent_capture_gives_plus_zero_everywhere(dec4, normalise):
    raw = np.full((1, 2 * 48000), 0x80, np.uint8)
    for form, got in both_forms(dec4, raw, wc.EDGE_BINS, normalise):
        assert not got.view(np.uint32).any(), form                         # +0: no sign bit either


@pytest.mark.parametrize("normalise", [False, True])
def test_worst_case_needs_the_full_accumulators(dec4, normalise):
    """all bytes 0x00 with c = 0: |v| near 2^50 (tests/test_wide_cpu.py), which fails with any accumulator narrower than the
    rule's; a second channel with q = 31 beside it"""
    raw = np.zeros((1, 2 * 48000), np.uint8)
    bins = (-128, -97)
    assert sw.channel(-97) == (0, 31)
    ref = np.stack([restated(raw[0], "zeros", fb, normalise) for fb in bins])[None]
    mid, peak = float(np.abs(ref[0, 0, :, 20]).max()), float(np.abs(ref[0, 0]).max())
    if normalise:                                                          # the peak is the overshoot at the capture's ends
        assert abs(peak - 0.5) < 1e-6 and 0.4 < mid < 0.5
    else:
        assert abs(mid - 1.0) < 1e-5 and peak < 1.2
    for form, got in both_forms(dec4, raw, bins, normalise):
        same_bytes(got, ref, f"{form} form")


def test_normalise_is_the_peak_rule(dec4):
    raw = wc.random_capture(192008, 31)[None]
    bins = (48000, -66000)
    for form, got in both_forms(dec4, raw, bins, True):
        ref = np.stack([restated(raw[0], "norm", fb, True) for fb in bins])[None]
        same_bytes(got, ref, f"{form} form")
        assert np.allclose(np.abs(got).max(axis=(2, 3)), 0.5, rtol=0, atol=1e-6)


# ---- full length ------------------------------------------------------------------------------------------------------------------

def test_full_length_capture(dec4):
    """36 000 000 pairs, two channels, all 48000 outputs of both, byte for byte"""
    raw = wc.random_capture(sw.MAX_PAIRS, 40)[None]
    bins = (48000, -65760)
    ref = sw.frames(raw, bins)
    assert ref[0, :, :, -1].all()
    same_bytes(frames_dev(dec4, raw, bins), ref, "device form")
    same_bytes(dec4.wide_frames(raw, bins), ref, "host form")


# ---- the whole path ---------------------------------------------------------------------------------------------------------------

CHANNELS = (48000, 48240, -66000, -65760)
# text, dial (freq_bin), Hz above the dial, start (s), the channel that reports it
PLANTED = (("CQ K1ABC FN42", 48000, 500.0, 0.5, 0), ("CQ DL1XYZ JO62", 48000, 2400.0, 0.8, 1),
           ("CQ JA1AAA PM95", -66000, 1531.25, 0.3, 2), ("CQ VK2BBB QF56", -66000, 700.0, 1.0, 2),
           ("CQ K1ABC FN42", -66000, 1100.0, 0.6, 2))                      # channel 0's text again, 114 000 bins from it


def device_capture(oracle):
    """one full-length capture built on the device in float64 from the tone sequences: five CPFSK signals at amplitude 20 over
    noise of sigma 30, rounded to bytes -> uint8 tensor [2 * 36 000 000]"""
    import torch
    n = sw.MAX_PAIRS
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(n, 2, generator=gen, device="cuda", dtype=torch.float32).double() * 30.0
    for text, dial, f0, t0, _ in PLANTED:
        rc, payload = oracle.pack77(text)
        assert rc == 0
        tones = torch.from_numpy(np.asarray(oracle.encode(payload[:10]), np.float64)).cuda()
        f = (6.25 * dial + f0 + 6.25 * tones).repeat_interleave(wc.SYMBOL)
        s = int(round(t0 * sw.RATE))
        k = min(f.numel(), n - s)
        phase = torch.cumsum(2.0 * np.pi * f[:k] / sw.RATE, 0)
        x[s:s + k, 0] += 20.0 * torch.cos(phase)
        x[s:s + k, 1] += 20.0 * torch.sin(phase)
        del f, phase
    return (torch.round(x) + 128.0).clamp_(0, 255).to(torch.uint8).reshape(-1)


def test_whole_path_is_decode_messages_and_the_merge(ft8, dec4, oracle):
    import torch
    cap = device_capture(oracle)
    raw = torch.stack([cap, torch.full_like(cap, 0x80)])                   # the capture and a silent one: [2][72 000 000]
    del cap
    nch = len(CHANNELS)
    iq = torch.zeros((2 * nch, 2, sw.NSAMPLES), dtype=torch.float32, device="cuda")
    dec4.wide_frames_dev(raw, 2, sw.MAX_PAIRS, CHANNELS, iq, True)
    cm = torch.zeros(2 * nch * 50 * 64, dtype=torch.uint8, device="cuda")
    cn = torch.zeros(2 * nch, dtype=torch.int32, device="cuda")
    dec4.decode_messages_dev(iq, 2 * nch, cm, cn)
    dec4.synchronize()
    bm = cm.cpu().numpy().view(ft8.MESSAGE_DTYPE).reshape(2, nch, 50)
    bn = cn.cpu().numpy().reshape(2, nch)
    want_m, want_n = sw.merge(bm, bn, CHANNELS, filled_msgs(ft8, 2, nch), np.zeros(2, np.int32))
    got_m, got_n = decode_dev(ft8, dec4, raw, CHANNELS)
    assert got_n.tolist() == want_n.tolist() and got_m.tobytes() == want_m.tobytes()
    recs = got_m[0, :int(got_n[0])]
    texts = [wc.text_of(r) for r in recs]
    print(texts, [float(r["freq_hz"]) for r in recs], [int(r["pad"][0]) for r in recs], bn.tolist())
    # each planted signal exactly once: JA1AAA lies in channels 2 and 3 and is dropped from 3; K1ABC was sent in channels 0 and 2,
    # which are more than 256 bins apart, and is kept from both, each record with its own frequency and channel
    assert sorted(texts) == sorted(t for t, _, _, _, _ in PLANTED)
    for text, dial, f0, _, chan in PLANTED:
        mine = [r for r, t in zip(recs, texts) if t == text and r["pad"][0] == chan]
        assert len(mine) == 1, (text, chan)
        assert abs(float(mine[0]["freq_hz"]) - (6.25 * dial + f0)) <= 3.125
    assert bn[0, 3] >= 1 and any(wc.text_of(r) == "CQ JA1AAA PM95" for r in bm[0, 3, :bn[0, 3]])   # heard there too, and dropped
    assert got_n[1] == 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_arguments_are_refused_with_their_text_and_outputs_stay(ft8, dec4):
    import torch
    lib = ft8.load_library()
    raw = wc.random_capture(752, 3)[None]
    iq = np.full((1, 16, 2, sw.NSAMPLES), np.float32(-7.5), np.float32)
    msgs, n = filled_msgs(ft8, 1, 16), np.full(1, -9, np.int32)
    keep_m = msgs.tobytes()

    def bins(*b):
        return np.array(b, np.int32)

    one = bins(0)
    cases = [  # (raw, npairs, freq_bin, nchannels, iq / msgs present, text)
        (raw, 752, one, 0, True, "nchannels 0 out of range [1, 16]"), (raw, 752, bins(*range(17)), 17, True, "nchannels 17 out of range [1, 16]"),
        (raw, 752, bins(0, 176001), 2, True, "freq_bin[1] = 176001 out of range [-176000, 176000]"),
        (raw, 752, bins(-176001), 1, True, "freq_bin[0] = -176001 out of range [-176000, 176000]"),
        (raw, 0, one, 1, True, "npairs 0 is not a positive multiple of 8 up to 36000000"),
        (raw, 750, one, 1, True, "npairs 750 is not a positive multiple of 8 up to 36000000"),
        (raw, 36000008, one, 1, True, "npairs 36000008 is not a positive multiple of 8 up to 36000000"),
        (raw, 752, None, 1, True, "NULL array argument"), (None, 752, one, 1, True, "NULL array argument"),
        (raw, 752, one, 1, False, "NULL array argument")]
    for r, npairs, b, nb, outs, text in cases:
        rp = None if r is None else r.ctypes.data
        bp = None if b is None else b.ctypes.data
        rc = lib.ft8gpu_wide_frames(dec4.h, rp, 1, npairs, bp, nb, iq.ctypes.data if outs else None, 0, ft8.HOST_PTRS)
        assert rc == -1 and text in lib.ft8gpu_last_error().decode(), (text, lib.ft8gpu_last_error())
        rc = lib.ft8gpu_decode_wide(dec4.h, rp, 1, npairs, bp, nb, msgs.ctypes.data if outs else None, n.ctypes.data, ft8.HOST_PTRS)
        assert rc == -1 and text in lib.ft8gpu_last_error().decode(), (text, lib.ft8gpu_last_error())
        assert (iq == np.float32(-7.5)).all() and msgs.tobytes() == keep_m and (n == -9).all()
    # a misaligned raw in the device form
    r_d, o_b = up(np.concatenate([np.zeros(8, np.uint8), raw[0]])), guarded(iq[:, :1])
    m_b, n_b = guarded(msgs[:, :50]), guarded(n)
    torch.cuda.synchronize()
    rc = lib.ft8gpu_wide_frames(dec4.h, r_d.data_ptr() + 8, 1, 752, one.ctypes.data, 1, o_b[GUARD:].data_ptr(), 0, ft8.DEVICE_PTRS)
    assert rc == -1 and "raw must be 16-byte aligned" in lib.ft8gpu_last_error().decode()
    rc = lib.ft8gpu_decode_wide(dec4.h, r_d.data_ptr() + 8, 1, 752, one.ctypes.data, 1, m_b[GUARD:].data_ptr(), n_b[GUARD:].data_ptr(), ft8.DEVICE_PTRS)
    assert rc == -1 and "raw must be 16-byte aligned" in lib.ft8gpu_last_error().decode()
    dec4.synchronize()
    assert (unguard(o_b, iq[:, :1].nbytes).view(np.float32) == np.float32(-7.5)).all()
    assert unguard(m_b, msgs[:, :50].nbytes).tobytes() == msgs[:, :50].tobytes() and (unguard(n_b, 4).view(np.int32) == -9).all()
    # a valid call follows
    same_bytes(dec4.wide_frames(raw, (0, 176000)), sw.frames(raw, (0, 176000)), "after the refusals")
    _, cnt = dec4.decode_wide(raw, (0,))
    assert cnt.tolist() == [0]


# ---- the existing entries ---------------------------------------------------------------------------------------------------------

def test_existing_entries_are_unchanged_by_wide_calls(ft8, oracle):
    """decode_messages and decode_batch on fixed frames before and after wide calls on the same, fresh context: the buffers of
    the wide path are allocated by the calls in between and stay with the context"""
    i, q = oracle.selftest_signal()
    iq = np.stack([np.stack([i, q]), np.random.default_rng(2).normal(0, 0.1, (2, sw.NSAMPLES)).astype(np.float32)])
    raw = np.stack([wc.random_capture(48000, 50 + k) for k in range(2)])
    with ft8.Decoder(device=0, max_frames=4) as dec:
        m0, n0 = dec.decode_messages(iq, msgs=filled_msgs(ft8, 2, 1))
        d0, r0 = dec.decode_batch(iq)
        _, cnt = dec.decode_wide(raw, (48000, 48240, -66000))
        assert cnt.tolist() == [0, 0]
        m1, n1 = dec.decode_messages(iq, msgs=filled_msgs(ft8, 2, 1))
        d1, r1 = dec.decode_batch(iq)
        dec.wide_frames(raw, wc.SIXTEEN)
        m2, n2 = dec.decode_messages(iq, msgs=filled_msgs(ft8, 2, 1))
        d2, r2 = dec.decode_batch(iq)
    assert n0[0] >= 1 and n0.tobytes() == n1.tobytes() == n2.tobytes() and m0.tobytes() == m1.tobytes() == m2.tobytes()
    assert d0.tobytes() == d1.tobytes() == d2.tobytes() and r0.tobytes() == r1.tobytes() == r2.tobytes()
