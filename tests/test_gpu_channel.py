"""GPU tests of the fading channel (ft8gpu_synth_gfsk_frames_faded, ft8gpu_synth_gfsk_audio_faded) against the numpy restatement
tests/ft8_spec_channel.py, byte for byte at noise_sigma = 0: I/Q frames with signals across a tile seam, before sample 0, with a
second path past the clip's end, on and off the gain grid, spreads 0, 0.1 and 20 Hz, path-2 gains 0, 1 and 4, faded and unfaded
signals mixed; audio in both formats at 20000 and 20011 samples with a signal across the last partial tile; 64 signals of two paths;
all-unfaded channels and no channels against the unfaded entries with noise on; any chunking and any partition of a job with noise
on; and faded frames through the decoder against the oracle."""
import numpy as np
import pytest

import ft8_spec_channel as sc
import ft8_spec_gfsk as sg
import ft8_spec_messages as sm
import gfsk_craft as gc

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xA5
F = np.float32


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as ft8
    ft8.check_build_id()
    return ft8


@pytest.fixture(scope="module")
def dec4(ft8):
    with ft8.Decoder(device=0, max_frames=4) as dec:
        yield dec


def synth(dec, mode, recs, chans, nsamples=sg.NSAMPLES_AUDIO, fmt=sg.F32, peak=0.0, form="host", sigma=0.0, seed=0, first=0):
    """one call of either faded entry in either pointer form (the device form between guard bands)"""
    import torch
    nclips, nsig = recs.shape
    if form == "host":
        if mode == sg.IQ:
            return dec.synth_gfsk_frames_faded(recs, chans, nclips, nsig, sigma, seed, first, peak)
        return dec.synth_gfsk_audio_faded(recs, chans, nclips, nsig, nsamples, sigma, seed, first, peak, fmt)
    shape = (nclips, 2, sg.NSAMPLES_IQ) if mode == sg.IQ else (nclips, nsamples)
    dtype = np.int16 if (mode == sg.AUDIO and fmt == sg.S16) else F
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    b = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if mode == sg.IQ:
        dec.synth_gfsk_frames_faded_dev(recs, chans, nclips, nsig, sigma, seed, first, peak, b[GUARD:].data_ptr())
    else:
        dec.synth_gfsk_audio_faded_dev(recs, chans, nclips, nsig, nsamples, sigma, seed, first, peak, fmt, b[GUARD:].data_ptr())
    dec.synchronize()
    h = b.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + nbytes:] == FILL).all(), "a guard band was written"
    return h[GUARD:GUARD + nbytes].copy().view(dtype).reshape(shape)


def unfaded(dec, mode, recs, nsamples=sg.NSAMPLES_AUDIO, fmt=sg.F32, peak=0.0, sigma=0.0, seed=0, first=0):
    nclips, nsig = recs.shape
    if mode == sg.IQ:
        return dec.synth_gfsk_frames(recs, nclips, nsig, sigma, seed, first, peak)
    return dec.synth_gfsk_audio(recs, nclips, nsig, nsamples, sigma, seed, first, peak, fmt)


def same_bytes(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    assert not np.isnan(ref).any()
    u = np.uint16 if got.dtype == np.int16 else np.uint32
    d = np.argwhere(got.view(u) != ref.view(u))
    assert len(d) == 0, f"{what}: {len(d)} samples differ, the first at {d[0].tolist()}: {got[tuple(d[0])]!r} != {ref[tuple(d[0])]!r}"


def expected(clips, chans, mode, nsamples, fmt, peak, seed, first):
    out = []
    for c, (sigs, chs) in enumerate(zip(clips, chans)):
        x = sg.normalise(sc.clip(sigs, chs, mode, nsamples, seed, first + c), peak)
        out.append(sg.to_s16(x) if fmt == sg.S16 else x)
    return np.stack(out)


# ---- I/Q frames -------------------------------------------------------------------------------------------------------------------------

def iq_case(ft8):
    tile = ft8.GFSK_TILE
    sigs = [(gc.random_tones(40), 700.0, (tile - 100) / 3200.0, 1.0),      # across the seam at sample 8192
            (gc.random_tones(41), -431.7, -0.5, 0.5),                       # from before sample 0
            (gc.random_tones(42), 1212.5, 2.36, 0.7),                       # ends at 48000: path 2, 32 samples later, runs past the end
            (gc.random_tones(43), 1800.0, 1.0, 0.3),                        # start 3200 = 100 grid steps: n' on grid points
            (gc.random_tones(44), 2200.3, 3217 / 3200.0, 0.9),              # off the grid
            (gc.random_tones(45), 950.0, 0.64, 0.25),                       # unfaded among the faded
            (gc.random_tones(46), 300.0, 5.0, 2.0)]                         # unfaded, its other fields are not looked at
    chs = [(0.1, 1.0, 1.0, sc.FADED), (20.0, 0.5, 4.0, sc.FADED), (0.0, 10.0, 1.0, sc.FADED), (0.1, 3.0, 0.0, sc.FADED),
           (20.0, 0.0, 0.0, sc.FADED), (0.0, 0.0, 0.0, sc.NONE), (np.nan, -3.0, 77.0, sc.NONE)]
    return [sigs, sigs[::-1]], [chs, chs[::-1]]


def test_frames_are_the_restatement_byte_for_byte(ft8, dec4):
    clips, chans = iq_case(ft8)
    starts = [sg.start_of(s[2], sg.IQ) for s in clips[0]]
    assert starts[0] == ft8.GFSK_TILE - 100 and starts[1] < 0 and starts[2] + 79 * 512 == 48000 and sc.delay_of(10.0, sg.IQ) == 32
    assert starts[3] % 32 == 0 and starts[4] % 32 != 0
    recs, crec = gc.records(clips), sc.channel_records(chans)
    for peak in (0.0, 0.5):
        want = expected(clips, chans, sg.IQ, None, sg.F32, peak, 11, 5)
        assert want.any() and want[0].tobytes() != want[1].tobytes()
        for form in ("host", "device"):
            same_bytes(synth(dec4, sg.IQ, recs, crec, peak=peak, form=form, seed=11, first=5), want, f"{form} form, peak {peak}")
    other = synth(dec4, sg.IQ, recs, crec, seed=12, first=5)
    assert other.tobytes() != want.tobytes()                               # the taps do depend on the seed
    assert np.abs(other.astype(np.float64) - sg.clip(clips[0], sg.IQ)).max() > 0.1


def test_sixty_four_signals_of_two_paths_in_one_clip(ft8, dec4):
    sigs = [(gc.random_tones(500 + s), 100.0 + 45.3 * s, -0.4 + 0.04 * s, 0.25 + 0.01 * s) for s in range(64)]
    chs = [((0.1, 1.0, 20.0)[s % 3], 0.15 * s, (1.0, 4.0, 0.5)[s % 3], sc.FADED) for s in range(64)]
    recs, crec = gc.records([sigs]), sc.channel_records([chs])
    want = expected([sigs], [chs], sg.IQ, None, sg.F32, 0.0, 3, 2 ** 33)
    same_bytes(synth(dec4, sg.IQ, recs, crec, form="device", seed=3, first=2 ** 33), want, "64 signals, two paths each")


# ---- audio ------------------------------------------------------------------------------------------------------------------------------

def audio_case(ft8):
    tile = ft8.GFSK_TILE
    sigs = [(gc.random_tones(60), 1500.0, (2 * tile - 304) / 12000.0, 1.0),   # across the seam at 16384 into the last, partial tile
            (gc.random_tones(61), 433.1, -12.0, 0.5),                          # only its last 0.64 s sound
            (gc.random_tones(62), 2718.28, 8401 / 12000.0, 0.7),               # off the grid of 120
            (gc.random_tones(63), 1000.0, 1.0, 0.4)]                           # unfaded
    chs = [(20.0, 10.0, 1.0, sc.FADED), (0.1, 0.5, 4.0, sc.FADED), (0.0, 2.0, 0.0, sc.FADED), (1.0, 1.0, 1.0, sc.NONE)]
    return [sigs, sigs[::-1]], [chs, chs[::-1]]


@pytest.mark.parametrize("fmt", [sg.S16, sg.F32])
def test_audio_is_the_restatement_byte_for_byte(ft8, dec4, fmt):
    clips, chans = audio_case(ft8)
    start = sg.start_of(clips[0][0][2], sg.AUDIO)
    assert start == 2 * ft8.GFSK_TILE - 304 and start % 120 == 0 and sg.start_of(clips[0][2][2], sg.AUDIO) == 8401 and sc.delay_of(10.0, sg.AUDIO) == 120
    recs, crec = gc.records(clips), sc.channel_records(chans)
    for nsamples in (20000, 20011):
        assert nsamples % ft8.GFSK_TILE and nsamples > 2 * ft8.GFSK_TILE and (nsamples == 20000 or (nsamples % 120 and nsamples % 2))
        for peak in (0.0, 0.5):
            want = expected(clips, chans, sg.AUDIO, nsamples, fmt, peak, 21, 0)
            assert want[:, 2 * ft8.GFSK_TILE:].any()
            for form in ("host", "device"):
                same_bytes(synth(dec4, sg.AUDIO, recs, crec, nsamples, fmt, peak, form, seed=21), want, f"{form} form, {nsamples} samples, peak {peak}")


# ---- no channels, unfaded channels, chunking and partitions: with noise ---------------------------------------------------------------

JOBS = [(sg.IQ, sg.F32, sg.NSAMPLES_IQ), (sg.AUDIO, sg.S16, 20011), (sg.AUDIO, sg.F32, 4099)]


def noisy_job():
    clips = [[(gc.random_tones(200 + c), 600.0 + 111.0 * c, 0.1 * c, 0.3), (gc.random_tones(300 + c), 1500.0 - 50.0 * c, 0.2, 0.2)] for c in range(5)]
    chans = [[(1.0, 2.0, 1.0, sc.FADED), ((0.0, 0.0, 0.0, sc.NONE) if c % 2 else (10.0, 0.5, 0.0, sc.FADED))] for c in range(5)]
    return gc.records(clips), sc.channel_records(chans)


def test_unfaded_channels_and_no_channels_are_the_unfaded_entries_with_noise(ft8, dec4):
    recs, _ = noisy_job()
    none = sc.channel_records([[(5.0, 5.0, 1.0, sc.NONE), (np.nan, np.inf, -1.0, sc.NONE)]] * 5)
    for mode, fmt, n in JOBS:
        want = unfaded(dec4, mode, recs, n, fmt, 0.5, sigma=0.1, seed=9, first=40)
        for chans in (none, None):
            for form in ("host", "device"):
                got = synth(dec4, mode, recs, chans, n, fmt, 0.5, form, sigma=0.1, seed=9, first=40)
                assert got.tobytes() == want.tobytes(), (mode, fmt, form, chans is None)
        assert want.tobytes() != unfaded(dec4, mode, recs, n, fmt, 0.5, seed=9, first=40).tobytes()      # the noise is on


def test_chunking_gives_the_same_bytes_with_noise(ft8):
    recs, crec = noisy_job()
    out = {}
    for mf in (8, 2, 1):
        with ft8.Decoder(device=0, max_frames=mf) as dec:
            out[mf] = [synth(dec, mode, recs, crec, n, fmt, 0.5, form, sigma=0.1, seed=9, first=7).tobytes()
                       for mode, fmt, n in JOBS for form in ("host", "device")]
    assert out[8][0] == out[8][1] and out[8][2] == out[8][3] and out[8][4] == out[8][5]
    assert out[2] == out[8] and out[1] == out[8]
    assert len(set(out[8])) == len(JOBS)


def test_any_partition_of_a_job_gives_the_same_clips(ft8, dec4):
    recs, crec = noisy_job()
    for mode, fmt, n in JOBS:
        whole = synth(dec4, mode, recs, crec, n, fmt, 0.5, "device", sigma=0.1, seed=9, first=40)
        parts = np.concatenate([synth(dec4, mode, recs[:2], crec[:2], n, fmt, 0.5, "device", sigma=0.1, seed=9, first=40),
                                synth(dec4, mode, recs[2:], crec[2:], n, fmt, 0.5, "host", sigma=0.1, seed=9, first=42)])
        assert whole.tobytes() == parts.tobytes(), (mode, fmt)
        clean = synth(dec4, mode, recs, crec, n, fmt, 0.5, "device", seed=9, first=40)
        assert whole.tobytes() != clean.tobytes()
        shifted = synth(dec4, mode, recs, crec, n, fmt, 0.5, "device", seed=9, first=41)
        assert clean.tobytes() != shifted.tobytes()                        # the taps do depend on the global clip index


# ---- faded frames through the decoder ----------------------------------------------------------------------------------------------------

def test_decoder_and_oracle_give_the_same_records_on_faded_frames(ft8, oracle):
    """eight frames of one station at +4 dB, one path, 1 Hz spread: the device's frames through ft8gpu_decode_messages and through
    the oracle's stages and the restated collection; how many decode is not asserted"""
    import synth_util as S
    tones = gc.tones_of(oracle, gc.EIGHT_TEXT)
    amp = S.amplitude_for_snr(4.0, 1.0)
    clips = [[(tones, 700.0 + 3.1 * s, (1600 + 37 * s) / 3200.0, amp)] for s in range(8)]
    recs, crec = gc.records(clips), sc.channel_records([[(1.0, 0.0, 0.0, sc.FADED)]] * 8)
    with ft8.Decoder(device=0, max_frames=8) as dec:
        frames = synth(dec, sg.IQ, recs, crec, peak=0.5, sigma=1.0, seed=100)
        got, n = dec.decode_messages(frames)
    mag, cands, counts, status = sm.oracle_stages(oracle, frames)
    want, wn = sm.collect(mag, cands, counts, status)
    print(f"messages per frame: device {n.tolist()}, oracle {wn.tolist()}")
    assert sm.check(got, n, want, wn) is None, sm.check(got, n, want, wn)
    assert all(abs(float(np.abs(frames[f]).max()) - 0.5) <= 2.0 ** -24 for f in range(8))
