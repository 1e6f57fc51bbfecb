"""GPU tests of the audio front end (ft8gpu_audio_frames, ft8gpu_decode_audio) against the numpy restatement
tests/ft8_spec_audio.py, byte for byte (a NaN of the rule for a NaN): the stage on both formats, whole and ragged and tiny clips,
one to four bands, host and device pointers; chunking under contexts of 1, 4 and 8 frames; guard bands around the device form's
outputs; the whole path on the five-signal clip of tests/test_audio_cpu.py beside a clip of noise and a clip of zeros; the
refusals; and the existing messages path before and after an audio call on the same context."""
import numpy as np
import pytest

import audio_craft as ac
import ft8_spec_audio as sa

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xA5
BAND_LISTS = ((0,), (0, 240), (704,), (0, 240, 480, 704))


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


def filled_msgs(ft8, nclips, nbands):
    return np.full((nclips, 50 * nbands * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(nclips, 50 * nbands)


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as ft8
    ft8.check_build_id()
    return ft8


@pytest.fixture(scope="module")
def dec4(ft8):
    with ft8.Decoder(device=0, max_frames=4) as dec:
        yield dec


def frames_dev(ft8, dec, pcm, fmt, bases):
    """the device form between guard bands -> iq [nclips][nbands][2][48000]"""
    import torch
    nclips, nsamples = pcm.shape
    out = np.zeros((nclips, len(bases), 2, sa.NSAMPLES), np.float32)
    p_d, o_b = up(pcm), guarded(out)
    torch.cuda.synchronize()
    dec.audio_frames_dev(p_d.data_ptr(), fmt, nclips, nsamples, bases, o_b[GUARD:].data_ptr())
    dec.synchronize()
    return unguard(o_b, out.nbytes).view(np.float32).reshape(out.shape)


def decode_dev(ft8, dec, pcm, fmt, bases):
    """the whole path's device form between guard bands -> (msgs, n_msgs)"""
    import torch
    nclips, nsamples = pcm.shape
    fill = filled_msgs(ft8, nclips, len(bases))
    p_d, m_b, n_b = up(pcm), guarded(fill), guarded(np.zeros(nclips, np.int32))
    torch.cuda.synchronize()
    dec.decode_audio_dev(p_d.data_ptr(), fmt, nclips, nsamples, bases, m_b[GUARD:].data_ptr(), n_b[GUARD:].data_ptr())
    dec.synchronize()
    return unguard(m_b, fill.nbytes).view(ft8.MESSAGE_DTYPE).reshape(fill.shape), unguard(n_b, 4 * nclips).view(np.int32)


# ---- stage parity -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nsamples", [180000, 179999, 7, 1])
@pytest.mark.parametrize("fmt", [sa.S16, sa.F32])
def test_stage_is_the_restatement_byte_for_byte(ft8, dec4, fmt, nsamples):
    pcm = ac.s16_clips(nsamples) if fmt == sa.S16 else ac.f32_clips(nsamples)
    want = {base: sa.frames(pcm, fmt, (base,))[:, 0] for base in (0, 240, 480, 704)}       # every band once: [3][2][48000]
    nan_clip = fmt == sa.F32
    for bases in BAND_LISTS:
        ref = np.stack([want[b] for b in bases], axis=1)
        for form in ("host", "device"):
            got = dec4.audio_frames(pcm, bases) if form == "host" else frames_dev(ft8, dec4, pcm, fmt, bases)
            for c in range(3):
                if nan_clip and c == 1:
                    nans, diff = sa.same(got[c], ref[c])
                    assert diff is None, f"{form} form, bands {bases}, clip {c}: {diff}"
                    assert nans > 0 and np.array_equal(np.isnan(got[c]), np.isnan(ref[c]))
                else:
                    assert not np.isnan(ref[c]).any()
                    d = np.argwhere(got[c].view(np.uint32) != ref[c].view(np.uint32))
                    assert len(d) == 0, f"{form} form, bands {bases}, clip {c}: {len(d)} samples differ, the first at {d[0].tolist()}"
    assert want[0][0].any() and want[704][0].any()                                          # the noise clip is not silent
    assert not want[240][2].any()                                                           # all zeros in, zeros out


# ---- chunking ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def five(oracle):
    """the five-signal clip, a clip of noise alone and a clip of zeros: int16 [3][180000]"""
    return np.stack([ac.five_signal_clip(oracle), ac.to_s16(ac.noise(6)), np.zeros(ac.N, np.int16)])


def test_chunking_gives_the_same_bytes(ft8, five):
    """3 clips x 2 bands on contexts of 8, 4 and 1 frames: one run, runs of 4 + 2, and a clip whose bands do not fit one run"""
    out = {}
    for mf in (8, 4, 1):
        with ft8.Decoder(device=0, max_frames=mf) as dec:
            iq = dec.audio_frames(five, ac.BANDS)
            iq_d = frames_dev(ft8, dec, five, sa.S16, ac.BANDS)
            m, n = dec.decode_audio(five, ac.BANDS, msgs=filled_msgs(ft8, 3, 2))
            m_d, n_d = decode_dev(ft8, dec, five, sa.S16, ac.BANDS)
            out[mf] = (iq.tobytes(), iq_d.tobytes(), m.tobytes(), n.tobytes(), m_d.tobytes(), n_d.tobytes())
    assert out[8][0] == out[8][1] and out[8][2] == out[8][4] and out[8][3] == out[8][5]
    assert out[4] == out[8] and out[1] == out[8]


# ---- the whole path ---------------------------------------------------------------------------------------------------------------

def test_whole_path_is_decode_messages_and_the_merge(ft8, dec4, five):
    frames = sa.frames(five, sa.S16, ac.BANDS)                              # [3][2][2][48000]
    bm, bn = dec4.decode_messages(frames.reshape(6, 2, sa.NSAMPLES))
    want_m, want_n = sa.merge(bm.reshape(3, 2, 50), bn.reshape(3, 2), ac.BANDS, filled_msgs(ft8, 3, 2), np.zeros(3, np.int32))
    for form in ("host", "device"):
        if form == "host":
            got_m, got_n = dec4.decode_audio(five, ac.BANDS, msgs=filled_msgs(ft8, 3, 2))
        else:
            got_m, got_n = decode_dev(ft8, dec4, five, sa.S16, ac.BANDS)
        assert got_n.tolist() == want_n.tolist(), form
        assert got_m.tobytes() == want_m.tobytes(), form
    n0 = int(want_n[0])
    recs = want_m[0, :n0]
    texts = [ac.text_of(r) for r in recs]
    print(texts, [float(r["freq_hz"]) for r in recs], want_n.tolist())
    assert sorted(texts) == sorted(t for t, _, _ in ac.PLANTED)              # each once: JA1AAA is heard in both bands
    for r, text in zip(recs, texts):
        assert abs(float(r["freq_hz"]) - ac.planted_hz(text)) <= 3.125
        if text == "CQ JA1AAA PM95":
            assert r["pad"][0] == 0
    assert want_n[2] == 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_arguments_are_refused_with_their_text_and_outputs_stay(ft8, dec4):
    lib = ft8.load_library()
    pcm = ac.s16_clips(7)
    iq = np.full((3, 4, 2, sa.NSAMPLES), np.float32(-7.5), np.float32)
    msgs, n = filled_msgs(ft8, 3, 4), np.full(3, -9, np.int32)
    keep_m = msgs.tobytes()

    def bases(*b):
        return np.array(b, np.int32)

    cases = [  # (format, nsamples, base_bin, nbands, text)
        (0, 7, bases(0), 0, "nbands 0 out of range [1, 4]"), (0, 7, bases(0, 1, 2, 3, 4), 5, "nbands 5 out of range [1, 4]"),
        (0, 7, bases(0, 705), 2, "base_bin[1] = 705 out of range [0, 704]"), (0, 7, bases(-1), 1, "base_bin[0] = -1 out of range [0, 704]"),
        (2, 7, bases(0), 1, "unknown audio format 2"), (-1, 7, bases(0), 1, "unknown audio format -1"),
        (0, 0, bases(0), 1, "nsamples 0 out of range [1, 180000]"), (0, 180001, bases(0), 1, "nsamples 180001 out of range [1, 180000]")]
    for fmt, ns, b, nb, text in cases:
        rc = lib.ft8gpu_audio_frames(dec4.h, pcm.ctypes.data, fmt, 3, ns, b.ctypes.data, nb, iq.ctypes.data, ft8.HOST_PTRS)
        assert rc == -1 and text in lib.ft8gpu_last_error().decode(), (text, lib.ft8gpu_last_error())
        rc = lib.ft8gpu_decode_audio(dec4.h, pcm.ctypes.data, fmt, 3, ns, b.ctypes.data, nb, msgs.ctypes.data, n.ctypes.data, ft8.HOST_PTRS)
        assert rc == -1 and text in lib.ft8gpu_last_error().decode(), (text, lib.ft8gpu_last_error())
        assert (iq == np.float32(-7.5)).all() and msgs.tobytes() == keep_m and (n == -9).all()
    # a valid call follows
    got = dec4.audio_frames(pcm, (0, 704))
    assert got.view(np.uint32).tobytes() == sa.frames(pcm, sa.S16, (0, 704)).view(np.uint32).tobytes()
    _, cnt = dec4.decode_audio(pcm, (0,))
    assert cnt.tolist() == [0, 0, 0]


# ---- the existing entries ---------------------------------------------------------------------------------------------------------

def test_messages_path_is_unchanged_by_an_audio_call(ft8, oracle, five):
    """decode_messages on a fixed frame before and after decode_audio on the same, fresh context: the frame buffer of the audio
    path is allocated by the call in between and stays with the context"""
    i, q = oracle.selftest_signal()
    iq = np.stack([np.stack([i, q]), np.random.default_rng(2).normal(0, 0.1, (2, sa.NSAMPLES)).astype(np.float32)])
    with ft8.Decoder(device=0, max_frames=4) as dec:
        m0, n0 = dec.decode_messages(iq, msgs=filled_msgs(ft8, 2, 1))
        d0, r0 = dec.decode_batch(iq)
        _, cnt = dec.decode_audio(five[:2], ac.BANDS)
        assert cnt[0] == 5
        m1, n1 = dec.decode_messages(iq, msgs=filled_msgs(ft8, 2, 1))
        d1, r1 = dec.decode_batch(iq)
        dec.audio_frames(five[2:, :1000], (0,))
        m2, n2 = dec.decode_messages(iq, msgs=filled_msgs(ft8, 2, 1))
    assert n0[0] >= 1 and n0.tobytes() == n1.tobytes() == n2.tobytes() and m0.tobytes() == m1.tobytes() == m2.tobytes()
    assert d0.tobytes() == d1.tobytes() and r0.tobytes() == r1.tobytes()
