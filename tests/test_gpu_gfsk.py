"""GPU tests of the GFSK synthesiser (ft8gpu_synth_gfsk_frames, ft8gpu_synth_gfsk_audio) against the numpy restatement
tests/ft8_spec_gfsk.py, byte for byte at noise_sigma = 0: both modes, both audio formats, with and without peak normalisation,
host and device pointers between guard bands, 0 to 64 signals that start before the clip, at 0, across tile seams and end behind
it, clips that end one below, at and one above every tile boundary of the kernel as built; with noise on, the same bytes under
contexts of 1, 4 and 8 frames and under any partition of a job; the noise's moments; the device's clips straight into the
decoders on the same context; refusals with a live context; and the existing paths before and after GFSK calls."""
import hashlib

import numpy as np
import pytest

import audio_craft as ac
import ft8_spec_gfsk as sg
import gfsk_craft as gc

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xA5
F = np.float32


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def guarded(nbytes):
    import torch
    return torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")


def unguard(b, nbytes):
    h = b.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + nbytes:] == FILL).all(), "a guard band was written"
    return h[GUARD:GUARD + nbytes].copy()


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as ft8
    ft8.check_build_id()
    return ft8


@pytest.fixture(scope="module")
def dec4(ft8):
    with ft8.Decoder(device=0, max_frames=4) as dec:
        yield dec


def synth(dec, mode, recs, nsamples=sg.NSAMPLES_AUDIO, fmt=sg.F32, peak=0.0, form="host", sigma=0.0, seed=0, first=0):
    """one call of either entry in either pointer form (the device form between guard bands) -> [nclips][2][48000] or
    [nclips][nsamples]"""
    import torch
    nclips, nsig = recs.shape
    if form == "host":
        if mode == sg.IQ:
            return dec.synth_gfsk_frames(recs, nclips, nsig, sigma, seed, first, peak)
        return dec.synth_gfsk_audio(recs, nclips, nsig, nsamples, sigma, seed, first, peak, fmt)
    shape = (nclips, 2, sg.NSAMPLES_IQ) if mode == sg.IQ else (nclips, nsamples)
    dtype = np.int16 if (mode == sg.AUDIO and fmt == sg.S16) else F
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    b = guarded(nbytes)
    torch.cuda.synchronize()
    if mode == sg.IQ:
        dec.synth_gfsk_frames_dev(recs, nclips, nsig, sigma, seed, first, peak, b[GUARD:].data_ptr())
    else:
        dec.synth_gfsk_audio_dev(recs, nclips, nsig, nsamples, sigma, seed, first, peak, fmt, b[GUARD:].data_ptr())
    dec.synchronize()
    return unguard(b, nbytes).view(dtype).reshape(shape)


def same_bytes(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    assert not np.isnan(ref).any()
    u = np.uint16 if got.dtype == np.int16 else np.uint32
    d = np.argwhere(got.view(u) != ref.view(u))
    assert len(d) == 0, f"{what}: {len(d)} samples differ, the first at {d[0].tolist()}: {got[tuple(d[0])]!r} != {ref[tuple(d[0])]!r}"


# ---- byte identity ----------------------------------------------------------------------------------------------------------------
_cases = {}


def case(mode, nsig):
    """two clips: the case's signals, and the same in reverse order -> (records [2][nsig], the restated sums before normalisation)"""
    if (mode, nsig) not in _cases:
        sigs = gc.case_signals(mode, nsig)
        clips = [sigs, sigs[::-1]]
        _cases[mode, nsig] = (gc.records(clips), [sg.clip(c, mode, sg.NSAMPLES_AUDIO) for c in clips])
    return _cases[mode, nsig]


def expected(sums, mode, nsamples, fmt, peak):
    out = []
    for x in sums:
        x = sg.normalise(x if mode == sg.IQ else x[:nsamples], peak)
        out.append(sg.to_s16(x) if fmt == sg.S16 else x)
    return np.stack(out)


@pytest.mark.parametrize("nsig", [0, 1, 3, 8, 64])
def test_frames_are_the_restatement_byte_for_byte(ft8, dec4, nsig):
    recs, sums = case(sg.IQ, nsig)
    if nsig == 8:
        assert (recs["f0_hz"] < 0).any() and (recs["amplitude"] == F(2.0 ** 100)).any() and (recs["amplitude"] == F(2.0 ** -130)).any()
    if nsig == 3:
        sub = np.abs(sums[0][:, int(12.5 * 3200):int(13.5 * 3200)])
        assert sub.max() < 2.0 ** -126 and (sub > 0).any()                 # only the 2^-130 signal sounds there: subnormals
    for peak in (0.0, 0.5):
        want = expected(sums, sg.IQ, None, sg.F32, peak)
        assert nsig == 0 or want.any()
        for form in ("host", "device"):
            same_bytes(synth(dec4, sg.IQ, recs, peak=peak, form=form), want, f"{form} form, peak {peak}")


@pytest.mark.parametrize("nsig", [0, 1, 3, 8, 64])
@pytest.mark.parametrize("fmt", [sg.S16, sg.F32])
def test_audio_is_the_restatement_byte_for_byte(ft8, dec4, fmt, nsig):
    recs, sums = case(sg.AUDIO, nsig)
    for nsamples in (180000, 179999, 7, 1):
        for peak in (0.0, 0.5):
            want = expected(sums, sg.AUDIO, nsamples, fmt, peak)
            for form in ("host", "device"):
                same_bytes(synth(dec4, sg.AUDIO, recs, nsamples, fmt, peak, form), want, f"{form} form, {nsamples} samples, peak {peak}")
    if nsig == 8 and fmt == sg.S16:
        full = expected(sums, sg.AUDIO, 180000, fmt, 0.0)
        assert full.max() == 32767 and full.min() == -32768              # the 2^100 signal drives both rails


def tile_lengths(tile):
    out = []
    for k in range(1, sg.NSAMPLES_AUDIO // tile + 2):
        out += [n for n in (k * tile - 1, k * tile, k * tile + 1) if 1 <= n <= sg.NSAMPLES_AUDIO]
    return out


@pytest.mark.parametrize("fmt,peak", [(sg.F32, 0.0), (sg.S16, 0.5)])
def test_clips_that_end_at_every_tile_boundary(ft8, dec4, fmt, peak):
    """the kernel's tile is its workgroup's share, so these are all of its seams; the three signals cover every sample"""
    recs, sums = case(sg.AUDIO, 3)
    lengths = tile_lengths(ft8.GFSK_TILE)
    assert len(lengths) >= 3 * (sg.NSAMPLES_AUDIO // ft8.GFSK_TILE) and np.abs(sums[0]).min() >= 0 and (sums[0] != 0).mean() > 0.99
    for nsamples in lengths:
        same_bytes(synth(dec4, sg.AUDIO, recs, nsamples, fmt, peak, "device"), expected(sums, sg.AUDIO, nsamples, fmt, peak),
                   f"{nsamples} samples")


def test_a_signal_across_a_tile_seam_and_the_clip_ends(ft8, dec4):
    """one signal per clip: starting 100 samples before a seam, before the clip, at 0, and running past the end"""
    tile = ft8.GFSK_TILE
    tones = gc.random_tones(77)
    for mode in (sg.IQ, sg.AUDIO):
        rate = sg.RATE[mode]
        clips = [[(tones, 1000.0, t0, 0.5)] for t0 in ((3 * tile - 100) / rate, -0.5, 0.0, 14.0)]
        want = np.stack([sg.clip(c, mode, sg.NSAMPLES_AUDIO) for c in clips])
        start = sg.start_of(clips[0][0][2], mode)
        assert start == 3 * tile - 100 and not want[0][..., :start].any() and (want[0][..., start + 1:start + 200] != 0).mean() > 0.9
        for form in ("host", "device"):
            same_bytes(synth(dec4, mode, gc.records(clips), form=form), want, f"mode {mode}, {form} form")


# ---- chunking and partitioning, with noise ---------------------------------------------------------------------------------------

def noisy_job():
    clips = [[(gc.random_tones(200 + c), 600.0 + 111.0 * c, 0.1 * c, 0.3), (gc.random_tones(300 + c), 1500.0 - 50.0 * c, 1.0, 0.2)] for c in range(5)]
    return gc.records(clips)


JOBS = [(sg.IQ, sg.F32, sg.NSAMPLES_IQ), (sg.AUDIO, sg.S16, 50001), (sg.AUDIO, sg.F32, 4099)]


def test_chunking_gives_the_same_bytes_with_noise(ft8):
    recs = noisy_job()
    out = {}
    for mf in (8, 4, 1):
        with ft8.Decoder(device=0, max_frames=mf) as dec:
            out[mf] = [synth(dec, mode, recs, n, fmt, 0.5, form, sigma=0.1, seed=9).tobytes()
                       for mode, fmt, n in JOBS for form in ("host", "device")]
    assert out[8][0] == out[8][1] and out[8][2] == out[8][3] and out[8][4] == out[8][5]
    assert out[4] == out[8] and out[1] == out[8]
    assert len(set(out[8])) == len(JOBS)


def test_any_partition_of_a_job_gives_the_same_clips(ft8, dec4):
    recs = noisy_job()
    for mode, fmt, n in JOBS:
        whole = synth(dec4, mode, recs, n, fmt, 0.5, "device", sigma=0.1, seed=9, first=40)
        parts = np.concatenate([synth(dec4, mode, recs[:2], n, fmt, 0.5, "device", sigma=0.1, seed=9, first=40),
                                synth(dec4, mode, recs[2:], n, fmt, 0.5, "host", sigma=0.1, seed=9, first=42)])
        assert whole.tobytes() == parts.tobytes(), (mode, fmt)
        other = synth(dec4, mode, recs, n, fmt, 0.5, "device", sigma=0.1, seed=9, first=41)
        assert whole.tobytes() != other.tobytes()                          # the noise does depend on the global index
        clean = synth(dec4, mode, recs, n, fmt, 0.5, "device")
        assert whole.tobytes() != clean.tobytes()


# ---- noise alone ------------------------------------------------------------------------------------------------------------------

def test_noise_alone_has_the_moments_of_unit_gaussian_noise(ft8, dec4):
    none = np.zeros((1, 0), gc.SIGNAL_DTYPE)
    n = sg.NSAMPLES_AUDIO
    a = synth(dec4, sg.AUDIO, none, n, sg.F32, 0.0, "device", sigma=1.0, seed=1)[0].astype(np.float64)
    print(f"audio: mean {a.mean():+.5f} (bound {5 / np.sqrt(n):.5f}), variance {a.var():.5f}")
    assert abs(a.mean()) <= 5 / np.sqrt(n) and abs(a.var() - 1.0) <= 0.02  # 6 standard deviations of the sample variance at N = 180000
    assert np.abs(a).max() < 7
    x = synth(dec4, sg.IQ, none, peak=0.0, form="device", sigma=1.0, seed=1)[0].astype(np.float64)
    m = sg.NSAMPLES_IQ
    corr = float((x[0] * x[1]).mean() / np.sqrt(x[0].var() * x[1].var()))
    print(f"I/Q: means {x[0].mean():+.5f} {x[1].mean():+.5f}, variances {x[0].var():.5f} {x[1].var():.5f}, correlation {corr:+.5f}")
    for p in range(2):
        assert abs(x[p].mean()) <= 5 / np.sqrt(m) and abs(x[p].var() - 1.0) <= 6 * np.sqrt(2.0 / m)
    assert abs(corr) <= 5 / np.sqrt(m)
    again = synth(dec4, sg.AUDIO, none, n, sg.F32, 0.0, "host", sigma=1.0, seed=1)[0]
    other = synth(dec4, sg.AUDIO, none, n, sg.F32, 0.0, "host", sigma=1.0, seed=2)[0]
    assert again.astype(np.float64).tobytes() == a.tobytes() and (other != again).mean() > 0.99
    half = synth(dec4, sg.AUDIO, none, n, sg.F32, 0.0, "host", sigma=0.5, seed=1)[0]
    assert abs(half.astype(np.float64).var() - 0.25) <= 0.005
    silent = synth(dec4, sg.AUDIO, none, n, sg.F32, 0.5, "device")[0]
    assert not silent.view(np.uint32).any()                                # no signal, no noise: +0 everywhere, also under a peak


# ---- the whole path on the device -------------------------------------------------------------------------------------------------

def test_five_signal_clip_goes_straight_into_the_audio_decoder(ft8, dec4, oracle):
    import torch
    recs = gc.records([gc.five_signals(oracle)])
    pcm = torch.zeros(sg.NSAMPLES_AUDIO, dtype=torch.int16, device="cuda")
    msgs = torch.zeros(100 * ft8.MESSAGE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec4.synth_gfsk_audio_dev(recs, 1, 5, sg.NSAMPLES_AUDIO, gc.FIVE_SIGMA, 5, 0, 0.5, sg.S16, pcm.data_ptr())
    dec4.decode_audio_dev(pcm.data_ptr(), sg.S16, 1, sg.NSAMPLES_AUDIO, ac.BANDS, msgs.data_ptr(), n.data_ptr())
    dec4.synchronize()
    count = int(n.cpu()[0])
    rec = msgs.cpu().numpy().view(ft8.MESSAGE_DTYPE)[:count]
    got = sorted(ac.text_of(r) for r in rec)
    print(got, [float(r["freq_hz"]) for r in rec])
    assert got == sorted(t for t, _, _ in ac.PLANTED)
    for r in rec:
        assert abs(float(r["freq_hz"]) - ac.planted_hz(ac.text_of(r))) <= 3.125
    assert int(np.abs(pcm.cpu().numpy().astype(np.int32)).max()) == 16384   # peak 0.5 of full scale, reached exactly


def test_eight_frames_at_minus_16_db_go_straight_into_the_decoder(ft8, oracle):
    import torch
    recs = gc.records(gc.eight_signals(oracle))
    with ft8.Decoder(device=0, max_frames=8) as dec:
        iq = torch.zeros((8, 2, sg.NSAMPLES_IQ), dtype=torch.float32, device="cuda")
        msgs = torch.zeros(8 * 50 * ft8.MESSAGE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        n = torch.zeros(8, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.synth_gfsk_frames_dev(recs, 8, 1, 1.0, 100, 0, 0.5, iq.data_ptr())
        dec.decode_messages_dev(iq.data_ptr(), 8, msgs.data_ptr(), n.data_ptr())
        dec.synchronize()
    frames, counts = iq.cpu().numpy(), n.cpu().numpy()
    rec = msgs.cpu().numpy().view(ft8.MESSAGE_DTYPE).reshape(8, 50)
    gpu = [gc.EIGHT_TEXT in [ac.text_of(r) for r in rec[f, :counts[f]]] for f in range(8)]
    cpu = [gc.EIGHT_TEXT in gc.decoded_texts(oracle, frames[f]) for f in range(8)]
    print(f"GPU {sum(gpu)} of 8, oracle on the same frames {sum(cpu)} of 8")
    for f in range(8):
        assert gpu[f] or not cpu[f], f
    assert sum(gpu) == 8
    assert all(abs(float(np.abs(frames[f]).max()) - 0.5) <= 2.0 ** -24 for f in range(8))


# ---- refusals with a live context, and the existing paths ------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(ft8, dec4):
    import torch
    lib = ft8.load_library()
    good = gc.records([[(gc.random_tones(1), 1000.0, 0.5, 1.0)]])
    cases = []
    for field, value, says in (("f0_hz", np.nan, "not finite"), ("f0_hz", 12000.0, "out of range [0, 12000)"), ("t0_s", -60.5, "out of range [-60, 60]"),
                               ("amplitude", np.inf, "not finite")):
        bad = good.copy()
        bad[field][0, 0] = value
        cases.append((bad, 1, 64, 0.0, 0.0, sg.F32, says))
    bad = good.copy()
    bad["tones"][0, 0, 40] = 8
    cases += [(bad, 1, 64, 0.0, 0.0, sg.F32, "tone 40 is 8"), (good, 65, 64, 0.0, 0.0, sg.F32, "nsig 65"), (good, 1, 0, 0.0, 0.0, sg.F32, "nsamples 0"),
              (good, 1, 180001, 0.0, 0.0, sg.F32, "nsamples 180001"), (good, 1, 64, -1.0, 0.0, sg.F32, "noise_sigma"),
              (good, 1, 64, 0.0, -1.0, sg.F32, "peak"), (good, 1, 64, 0.0, 0.0, 7, "unknown audio format 7")]
    for recs, nsig, nsamples, sigma, peak, fmt, says in cases:
        b = guarded(1024)
        torch.cuda.synchronize()
        rc = lib.ft8gpu_synth_gfsk_audio(dec4.h, recs.ctypes.data, 1, nsig, nsamples, sigma, 1, 0, peak, fmt, b[GUARD:].data_ptr(), ft8.DEVICE_PTRS)
        err = lib.ft8gpu_last_error().decode()
        dec4.synchronize()
        assert rc == -1 and says in err, (says, err)
        assert (b.cpu().numpy() == FILL).all()
    host = np.full(64, 0x5A5A, np.int16)
    assert lib.ft8gpu_synth_gfsk_audio(dec4.h, good.ctypes.data, 1, 1, 64, 0.0, 1, 0, 0.0, sg.S16, None, ft8.HOST_PTRS) == -1
    assert b"NULL array argument" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_synth_gfsk_audio(dec4.h, good.ctypes.data, -1, 1, 64, 0.0, 1, 0, 0.0, sg.S16, host.ctypes.data, ft8.HOST_PTRS) == -1
    assert lib.ft8gpu_synth_gfsk_audio(dec4.h, good.ctypes.data, 0, 1, 64, 0.0, 1, 0, 0.0, sg.S16, host.ctypes.data, ft8.HOST_PTRS) == 0
    assert (host == 0x5A5A).all()
    same_bytes(synth(dec4, sg.AUDIO, good, 64, sg.F32), sg.clip([(good["tones"][0, 0], 1000.0, 0.5, 1.0)], sg.AUDIO, 64)[None], "after the refusals")


def test_existing_paths_are_unchanged_by_gfsk_calls(ft8, oracle):
    import torch
    import synth_util as S
    iq = np.stack([S.make_frame(500 + k, 6, S.oracle_encode_fn(oracle))[0] for k in range(3)])
    sigs = np.zeros((3, 2), ft8.SIGNAL_DTYPE)
    for k in range(3):
        for s in range(2):
            sigs[k, s]["tones"] = gc.random_tones(10 * k + s)
            sigs[k, s]["f0_hz"], sigs[k, s]["t0_s"], sigs[k, s]["amplitude"] = 500.0 + 300 * s, 0.5 + 0.1 * k, 2.0

    def digests(dec):
        d, n = dec.decode_batch(iq)
        m, nm = dec.decode_messages(iq)
        buf = torch.zeros((3, 2, 48000), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dec.synth_frames(sigs, 3, 2, 1.0, 7, buf.data_ptr())
        dec.synchronize()
        return [hashlib.sha256(x.tobytes()).hexdigest() for x in (d, n, m, nm, buf.cpu().numpy())]

    with ft8.Decoder(device=0, max_frames=4) as dec:
        before = digests(dec)
        recs = noisy_job()
        for mode, fmt, n in JOBS:
            for form in ("host", "device"):
                synth(dec, mode, recs, n, fmt, 0.5, form, sigma=0.1, seed=3)
        after = digests(dec)
    with ft8.Decoder(device=0, max_frames=4) as fresh:
        assert digests(fresh) == before
    assert after == before
