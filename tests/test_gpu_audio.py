"""GPU tests of the audio front end (ft8gpu_audio_frames, ft8gpu_decode_audio) against the numpy restatement
tests/ft8_spec_audio.py, byte for byte (a NaN of the rule for a NaN): the stage on both formats, whole and ragged and tiny clips,
one to four bands, host and device pointers; chunking under contexts of 1, 4 and 8 frames; guard bands around the device form's
outputs; the whole path on the five-signal clip of tests/test_audio_cpu.py beside a clip of noise and a clip of zeros; the
refusals; and the existing messages path before and after an audio call on the same context.  A second round aims at the kernel's
own seams with the constructed inputs of tests/audio_craft.py: band lists that read every entry of the mixer table, the stage
in double from its definition with a derived rounding bound, impulse clips that meet one tap per output, clips that end at every
group, tile and workgroup boundary, an unaligned device pointer, runs that begin and end inside a clip, and the merge on
overlapping bands."""
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


def up_at(a, offset):
    """a device copy of a's bytes `offset` bytes behind a 16-byte aligned address -> (the buffer, the address of the copy)"""
    import torch
    a = np.ascontiguousarray(a)
    b = torch.full((offset + a.nbytes + 16,), FILL, dtype=torch.uint8, device="cuda")
    assert b.data_ptr() % 16 == 0
    b[offset:offset + a.nbytes] = up(a)
    return b, b.data_ptr() + offset


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


def frames_dev(ft8, dec, pcm, fmt, bases, offset=0):
    """the device form between guard bands, pcm `offset` bytes behind a 16-byte aligned address -> iq [nclips][nbands][2][48000]"""
    import torch
    nclips, nsamples = pcm.shape
    out = np.zeros((nclips, len(bases), 2, sa.NSAMPLES), np.float32)
    (p_b, p_d), o_b = up_at(pcm, offset), guarded(out)
    assert p_d % 16 == offset % 16
    torch.cuda.synchronize()
    dec.audio_frames_dev(p_d, fmt, nclips, nsamples, bases, o_b[GUARD:].data_ptr())
    dec.synchronize()
    return unguard(o_b, out.nbytes).view(np.float32).reshape(out.shape)


def decode_dev(ft8, dec, pcm, fmt, bases, offset=0):
    """the whole path's device form between guard bands, pcm as in frames_dev -> (msgs, n_msgs)"""
    import torch
    nclips, nsamples = pcm.shape
    fill = filled_msgs(ft8, nclips, len(bases))
    (p_b, p_d), m_b, n_b = up_at(pcm, offset), guarded(fill), guarded(np.zeros(nclips, np.int32))
    assert p_d % 16 == offset % 16
    torch.cuda.synchronize()
    dec.decode_audio_dev(p_d, fmt, nclips, nsamples, bases, m_b[GUARD:].data_ptr(), n_b[GUARD:].data_ptr())
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


def both_forms(ft8, dec, pcm, fmt, bases):
    yield "host", dec.audio_frames(pcm, bases)
    yield "device", frames_dev(ft8, dec, pcm, fmt, bases)


def same_bytes(got, ref, what):
    d = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert len(d) == 0, f"{what}: {len(d)} samples differ, the first at {d[0].tolist()}"


_restated = {}


def restated(pcm, fmt, nsamples, base):
    """sa.frames of the stage parity clips for one base, computed once per (format, nsamples, base): [3][2][48000]"""
    key = (fmt, nsamples, base)
    if key not in _restated:
        _restated[key] = sa.frames(pcm, fmt, (base,))[:, 0]
        _restated[key].setflags(write=False)
    return _restated[key]


@pytest.mark.parametrize("bases", ac.WIDE_BAND_LISTS, ids=lambda b: "-".join(map(str, b)))
@pytest.mark.parametrize("nsamples", [180000, 179999])
@pytest.mark.parametrize("fmt", [sa.S16, sa.F32])
def test_stage_on_bands_that_read_the_whole_mixer_table(ft8, dec4, fmt, nsamples, bases):
    """the clips and the comparison of test_stage_is_the_restatement_byte_for_byte on odd bases, a base that is a multiple of 4
    but not of 16, a descending list and a repeated base: together they read every entry of wm[] (tests/test_audio_cpu.py)"""
    pcm = ac.s16_clips(nsamples) if fmt == sa.S16 else ac.f32_clips(nsamples)
    ref = np.stack([restated(pcm, fmt, nsamples, b) for b in bases], axis=1)
    for form, got in both_forms(ft8, dec4, pcm, fmt, bases):
        for c in range(3):
            if fmt == sa.F32 and c == 1:
                nans, diff = sa.same(got[c], ref[c])
                assert diff is None, f"{form} form, bands {bases}, clip {c}: {diff}"
                assert nans > 0 and np.array_equal(np.isnan(got[c]), np.isnan(ref[c]))
            else:
                assert not np.isnan(ref[c]).any()
                same_bytes(got[c], ref[c], f"{form} form, bands {bases}, clip {c}")
        if bases == (240, 240):                                                            # a base twice: the same frame twice
            one = dec4.audio_frames(pcm, (240,))
            for b in range(2):
                assert sa.same(got[:, b], one[:, 0])[1] is None and sa.same(got[:, b], got[:, 0])[1] is None, form
    assert ref[0].any()


# ---- against the definition in double ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nsamples", ac.REF64_LENGTHS)
@pytest.mark.parametrize("fmt", [sa.S16, sa.F32])
def test_stage_lies_within_the_rounding_bound_of_the_definition(ft8, dec4, fmt, nsamples):
    """ac.ref64: zero-stuff by 4, the FIR at 48 kHz, every 15th sample, in double; the bound is 44 float32 roundings on the
    magnitudes under the window, derived there and not measured"""
    pcm = ac.noise_clip(fmt, nsamples)
    a = sa.samples(pcm, fmt)
    got = dec4.audio_frames(pcm[None], ac.REF64_BASES)[0]
    for b, base in enumerate(ac.REF64_BASES):
        worst = ac.worst_ratio(got[b], a, base)
        print(f"format {fmt}, {nsamples} samples, base {base}: worst error {worst:.2f} u S (bound 44)")
        assert 0 < worst <= 44


# ---- single taps ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("base", [3, 704])
@pytest.mark.parametrize("fmt", [sa.S16, sa.F32])
def test_impulse_clip_is_the_closed_form_byte_for_byte(ft8, dec4, fmt, base):
    """impulses 41 samples apart: every output is one product of the two tables or +0 (tests/test_audio_cpu.py proves that the
    expected frame meets every tap), so a wrong tap, table entry or rotation cannot hide in a sum"""
    pcm = ac.impulse_clip(fmt)
    want = ac.impulse_frame(pcm, fmt, base)
    assert want.any()
    for form, got in both_forms(ft8, dec4, pcm[None], fmt, (base,)):
        same_bytes(got[0, 0], want, f"{form} form")


# ---- clip ends --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", sorted(ac.SEAM_LENGTHS))
@pytest.mark.parametrize("fmt", [sa.S16, sa.F32])
def test_clip_ends_at_the_kernels_seams(ft8, dec4, fmt, group):
    """two dense clips that end inside a 16-byte group at every residue, at a tile's first staged sample, behind a tile's last
    one, at a workgroup's seam and at the start of the last tile; the second clip starts unaligned unless the length is a
    multiple of 8 (int16) or 4 (float32).  All outputs of every frame are compared, the silent tail too."""
    for nsamples in ac.SEAM_LENGTHS[group]:
        pcm = ac.seam_clips(fmt, nsamples)
        ref = sa.frames(pcm, fmt, ac.SEAM_BANDS)
        m0 = ac.first_silent_output(nsamples)
        for form, got in both_forms(ft8, dec4, pcm, fmt, ac.SEAM_BANDS):
            assert got.shape == (2, 2, 2, sa.NSAMPLES)
            same_bytes(got, ref, f"{form} form, {nsamples} samples")
            same_bytes(got[..., m0:], np.broadcast_to(ac.SILENCE[:, m0:], got[..., m0:].shape), f"{form} form, {nsamples} samples, the tail")
            assert (np.abs(got[:, :, :, m0 - 1]).max(axis=2) > 0).all()


# ---- an unaligned pcm pointer -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nsamples", [180000, 179999])
@pytest.mark.parametrize("fmt", [sa.S16, sa.F32])
def test_device_pcm_need_not_be_aligned(ft8, dec4, five, fmt, nsamples):
    """include/ft8gpu.h asks nothing of pcm in the device form: the five-signal clip and the noise clip, both dense, 2 .. 14 bytes
    behind a 16-byte aligned address give the bytes of the aligned call, frames and messages"""
    pcm = np.ascontiguousarray(five[:2, :nsamples])
    if fmt == sa.F32:
        pcm = pcm.astype(np.float32) * np.float32(2.0 ** -15)
    iq0 = frames_dev(ft8, dec4, pcm, fmt, ac.SEAM_BANDS)
    m0, n0 = decode_dev(ft8, dec4, pcm, fmt, ac.SEAM_BANDS)
    same_bytes(iq0, sa.frames(pcm, fmt, ac.SEAM_BANDS), "aligned")
    assert n0[0] >= 1                                                       # band 3 holds K1ABC at 700 Hz: the records are no blanks
    for offset in ((2, 8, 14) if fmt == sa.S16 else (4, 8, 12)):
        same_bytes(frames_dev(ft8, dec4, pcm, fmt, ac.SEAM_BANDS, offset), iq0, f"{offset} bytes off")
        m, n = decode_dev(ft8, dec4, pcm, fmt, ac.SEAM_BANDS, offset)
        assert n.tolist() == n0.tolist() and m.tobytes() == m0.tobytes(), offset


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


BANDS4 = (0, 240, 480, 704)


def test_runs_cut_inside_a_clip(ft8, five):
    """3 clips x 4 bands are frames 0 .. 11 of one chunk.  A context of 5 frames works them off as 0-4, 5-9, 10-11 and one of 3
    frames as 0-2, 3-5, 6-8, 9-11: runs that start at a band other than a clip's first, hold several frames and end inside
    another clip.  The bytes are those of the context that takes all twelve at once, and its frames are the restatement's."""
    out = {}
    for mf in (12, 5, 3):
        with ft8.Decoder(device=0, max_frames=mf) as dec:
            iq = dec.audio_frames(five, BANDS4)
            m, n = dec.decode_audio(five, BANDS4, msgs=filled_msgs(ft8, 3, 4))
            m_d, n_d = decode_dev(ft8, dec, five, sa.S16, BANDS4)
            out[mf] = (iq, m.tobytes(), n.tobytes(), m_d.tobytes(), n_d.tobytes())
    same_bytes(out[12][0], sa.frames(five, sa.S16, BANDS4), "12 frames")
    assert out[12][1] == out[12][3] and out[12][2] == out[12][4]
    assert np.frombuffer(out[12][2], np.int32).tolist()[0] == 5 and np.frombuffer(out[12][2], np.int32).tolist()[2] == 0
    for mf in (5, 3):
        same_bytes(out[mf][0], out[12][0], f"{mf} frames")
        assert out[mf][1:] == out[12][1:], mf


def test_runs_cut_inside_a_ragged_float_clip(ft8):
    """the stage part again on three float32 noise clips of 179999 samples, whose second and third clip start unaligned"""
    pcm = np.random.default_rng(31).normal(0, 0.2, (3, 179999)).astype(np.float32)
    out = {}
    for mf in (12, 5, 3):
        with ft8.Decoder(device=0, max_frames=mf) as dec:
            out[mf] = dec.audio_frames(pcm, BANDS4)
    same_bytes(out[12], sa.frames(pcm, sa.F32, BANDS4), "12 frames")
    for mf in (5, 3):
        same_bytes(out[mf], out[12], f"{mf} frames")


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


def test_merge_on_overlapping_bands(ft8, dec4, oracle):
    """twelve signals between 700 and 1500 Hz under the bands (96, 100, 0, 100): overlapping, not ascending, one base twice, so
    most records are duplicates, in up to four bands.  The expected result is the merge rule on decode_messages of the restated
    frames; what it keeps is checked against the planted signals and across the bands."""
    bases = ac.DOZEN_BANDS
    pcm = np.stack([ac.dozen_signal_clip(oracle), ac.to_s16(ac.noise(6)), np.zeros(ac.N, np.int16)])
    distinct = sorted(set(bases))
    by_base = sa.frames(pcm, sa.S16, distinct)                              # [3][3][2][48000]
    frames = np.stack([by_base[:, distinct.index(b)] for b in bases], axis=1)
    bm, bn = dec4.decode_messages(frames.reshape(12, 2, sa.NSAMPLES))
    bm, bn = bm.reshape(3, 4, 50), bn.reshape(3, 4)
    want_m, want_n = sa.merge(bm, bn, bases, filled_msgs(ft8, 3, 4), np.zeros(3, np.int32))
    for form in ("host", "device"):
        if form == "host":
            got_m, got_n = dec4.decode_audio(pcm, bases, msgs=filled_msgs(ft8, 3, 4))
        else:
            got_m, got_n = decode_dev(ft8, dec4, pcm, sa.S16, bases)
        assert got_n.tolist() == want_n.tolist(), form
        assert got_m.tobytes() == want_m.tobytes(), form
    kept = got_m[0, :int(got_n[0])]
    texts = [ac.text_of(r) for r in kept]
    planted = [t for t, _, _ in ac.DOZEN]
    print(texts, bn.tolist(), got_n.tolist())
    assert len(set(texts)) == len(texts) and sum(t in planted for t in texts) >= 10 and got_n[2] == 0
    assert bn[0].sum() >= 3 * len(kept)                                     # most records are duplicates
    assert bn[0, 3] == bn[0, 1] > 0 and not (kept["pad"][:, 0] == 3).any()   # the second band of base 100 adds nothing
    in_band = [[bm[0, b, k]["a91"].tobytes() for k in range(bn[0, b])] for b in range(4)]
    for r, text in zip(kept, texts):
        holds = [b for b in range(4) if r["a91"].tobytes() in in_band[b]]
        assert r["pad"][0] == holds[0]                                      # the first band in list order
        hz = {bases[b]: (float(c["freq_offset"]) + bases[b] + float(c["freq_sub"]) / 2) * 6.25
              for b in holds for c in [bm[0, b, in_band[b].index(r["a91"].tobytes())]["cand"]]}
        assert float(r["freq_hz"]) == hz[bases[holds[0]]]
        assert max(hz.values()) - min(hz.values()) <= 3.125, (text, hz)     # one signal, seen from every base at one frequency
        if text in planted:
            assert all(abs(f - ac.dozen_hz(text)) <= 3.125 for f in hz.values()), (text, hz)


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
