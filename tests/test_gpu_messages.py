"""GPU tests of the messages path (ft8gpu_decode_messages / ft8gpu_collect_messages / ft8gpu_noise_baseline): the noise
baseline against np.partition, the message records against the numpy restatement (tests/ft8_spec_messages.py) on
oracle-made stage inputs, the whole path against its own stages and against ft8gpu_decode_batch, the host and device
forms, chunking, guard bands, and the estimate's accuracy on synthesised frames."""
import json
import os

import numpy as np
import pytest

import ft8_spec_messages as spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A


def _mixed_frames(texts, tones, nframes, nsig, snr, seed):
    import synth_util as S
    return np.stack([S.make_mixed_frame(seed + k, nsig, snr, texts, tones)[0] for k in range(nframes)])


def _cq_frames(oracle, nframes, nsig, seed):
    import synth_util as S
    enc = S.oracle_encode_fn(oracle)
    return np.stack([S.make_frame(seed + k, nsig, enc, snr_range=(-16.0, 4.0))[0] for k in range(nframes)])


def test_noise_baseline_equals_np_partition(oracle):
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    texts, tones = workload.mixed_message_pool(128, seed=2)
    iq = _mixed_frames(texts, tones, 5, 8, (-10.0, 10.0), 40)
    mag = oracle.waterfall_batch(iq, nthreads=8)
    rng = np.random.default_rng(9)
    hand = np.zeros((5, ft8.MAG_ARRAY), np.uint8)
    hand[0] = 0
    hand[1] = 255
    hand[2] = rng.integers(0, 3, ft8.MAG_ARRAY)                        # ties everywhere
    hand[3] = rng.choice(np.array([0, 255], np.uint8), ft8.MAG_ARRAY)   # only the extremes
    col = hand[4].reshape(184, 512)
    col[:] = rng.integers(0, 256, (184, 512))
    col[:, 0] = 7                                                      # one all-equal column
    col[:47, 1], col[47:, 1] = 0, 255                                  # the rank boundary exactly at a step
    col[:46, 2], col[46:, 2] = 0, 255
    allm = np.concatenate([mag, hand])
    with ft8.Decoder(device=0, max_frames=4) as dec:                  # 10 frames: chunked
        got = dec.noise_baseline(allm)
    assert np.array_equal(got, spec.noise_baseline(allm))
    assert got[9, 0, 0] == 7 and got[9, 0, 1] == 0 and got[9, 0, 2] == 255 and got[5].max() == 0 and got[6].min() == 255


def _stage_inputs(oracle, iq, cap):
    return spec.oracle_stages(oracle, iq, max_candidates=cap)


def _device_collect(ft8, mag, cands, counts, status, cap, max_frames=8):
    with ft8.Decoder(device=0, max_frames=max_frames, max_candidates=cap) as dec:
        st = np.ascontiguousarray(status).view(ft8.STATUS_DTYPE).reshape(len(counts), cap)
        return dec.collect_messages(mag, cands, counts, st)


@pytest.mark.parametrize("cap", [1, 7, 120, 480])
def test_collect_messages_equals_restatement_mixed_and_cq(oracle, cap):
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    texts, tones = workload.mixed_message_pool(256, seed=4)
    iq = np.concatenate([_mixed_frames(texts, tones, 6, 14, (-14.0, 8.0), 200 + cap), _cq_frames(oracle, 4, 12, 300 + cap)])
    mag, cands, counts, status = _stage_inputs(oracle, iq, cap)
    got, n = _device_collect(ft8, mag, cands, counts, status, cap)
    want, wn = spec.collect(mag, cands, counts, status)
    assert spec.check(got, n, want, wn) is None, spec.check(got, n, want, wn)
    if cap >= 120:
        assert wn.sum() > 40
    for f in range(len(n)):                                           # both sides encode the same bits
        for r in got[f, :n[f]]:
            assert spec.crc_in_a91(r["a91"]) == spec.crc_of_payload(r["a91"]) == int(r["hash"])
            assert bytes(r["pad"]) == b"\0\0\0\0"


def _synthetic_status(ft8, texts, a91s):
    st = np.zeros(len(texts), ft8.STATUS_DTYPE)
    for k, (t, a) in enumerate(zip(texts, a91s)):
        st[k]["ok"] = 1
        st[k]["text"] = t.encode()
        st[k]["a91"] = a
        st[k]["crc_extracted"] = st[k]["crc_calculated"] = spec.crc_in_a91(a)
    return st


def _a91_of(ft8, oracle, text):
    p = ft8.pack77(text)
    a = np.zeros(12, np.uint8)
    a[:10] = p
    a[9] &= 0xF8
    crc = spec.crc_of_payload(a)
    a[9] |= crc >> 11
    a[10] = (crc >> 3) & 0xFF
    a[11] = (crc << 5) & 0xFF
    return a


def test_collect_messages_edges(oracle):
    """hand-made candidate lists on real waterfalls: time offsets with partial symbol sets (to < 0, to + 78 >= 92),
    freq_offset 0 and 248, a frame with more than 50 unique messages, a frame with none, duplicates across chunks"""
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    texts, tones = workload.mixed_message_pool(256, seed=6)
    iq = _mixed_frames(texts, tones, 4, 10, (-10.0, 10.0), 500)
    mag = oracle.waterfall_batch(iq, nthreads=8)
    cap = 120
    B = 4
    cands = np.zeros((B, cap), ft8.CAND_DTYPE)
    status = np.zeros((B, cap), ft8.STATUS_DTYPE)
    counts = np.zeros(B, np.int32)
    pool = [t for t in texts if t is not None][:80]
    a91s = [_a91_of(ft8, oracle, t) for t in pool]
    rng = np.random.default_rng(12)
    # frame 0: edges of the waterfall
    edge = [(-12, 0), (-12, 248), (23, 0), (23, 248), (-5, 100), (14, 17), (0, 248), (13, 0)]
    for k, (to, fo) in enumerate(edge):
        cands[0, k] = (20 + k, to, fo, k & 1, (k >> 1) & 1)
    status[0, :len(edge)] = _synthetic_status(ft8, pool[:len(edge)], a91s[:len(edge)])
    counts[0] = len(edge)
    # frame 1: 80 distinct messages, then 40 repeats: 50 kept, the rest dropped
    for k in range(cap):
        j = k if k < 80 else int(rng.integers(0, 80))
        cands[1, k] = (15, int(rng.integers(-12, 24)), int(rng.integers(0, 249)), int(rng.integers(0, 2)), int(rng.integers(0, 2)))
        status[1, k] = _synthetic_status(ft8, [pool[j]], [a91s[j]])[0]
    counts[1] = cap
    # frame 2: none (every candidate below min_score or not decoded)
    for k in range(20):
        cands[2, k] = (5 if k % 2 else 30, 0, 10 * k, 0, 0)
        if k % 2:
            status[2, k] = _synthetic_status(ft8, [pool[k]], [a91s[k]])[0]
    counts[2] = 20
    # frame 3: few unique messages, repeated across the 64-candidate chunks, same hash different text
    for k in range(100):
        j = [3, 5, 3, 9, 5][k % 5]
        cands[3, k] = (12 + k % 3, int(rng.integers(-12, 24)), int(rng.integers(0, 249)), 0, 1)
        status[3, k] = _synthetic_status(ft8, [pool[j]], [a91s[j]])[0]
    status[3, 77]["text"] = b"FAKE TEXT"                              # hash of pool[3] or [5] with another text: a new message
    counts[3] = 100
    got, n = _device_collect(ft8, mag, cands, counts, status, cap)
    want, wn = spec.collect(mag, cands, counts, status)
    assert list(wn) == [len(edge), 50, 0, 4]
    assert spec.check(got, n, want, wn) is None, spec.check(got, n, want, wn)
    assert len({int(r["snr_db"]) for r in got[0, :n[0]]}) >= 1


def _synth_config2(ft8, workload, dec, B=4096, S=20):
    import torch
    msgs, tones = workload.message_pool()
    sig, picks = workload.frame_signals(0, B, S, tones, snr_range=(-18.0, 0.0))
    iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
    dec.synth_frames(sig, B, S, 1.0, workload.SEED_BASE, iq, first_frame=0)
    dec.synchronize()
    return iq


def _messages_dev(ft8, dec, iq, n, fill=0):
    import torch
    msgs = torch.full((n, ft8.MAX_MESSAGES * 64), fill, dtype=torch.uint8, device="cuda")
    nm = torch.zeros((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_messages_dev(iq, n, msgs, nm)
    dec.synchronize()
    return msgs.cpu().numpy().view(ft8.MESSAGE_DTYPE).reshape(n, ft8.MAX_MESSAGES), nm.cpu().numpy()


def _spots_dev(ft8, dec, iq, n):
    import torch
    spots = torch.zeros((n, ft8.MAX_MESSAGES * 28), dtype=torch.uint8, device="cuda")
    nres = torch.zeros((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_batch_dev(iq, n, spots, nres)
    dec.synchronize()
    return spots.cpu().numpy().view(ft8.RESULT_DTYPE).reshape(n, ft8.MAX_MESSAGES), nres.cpu().numpy()


def _c_field(text, k, prec):
    """the k-th strtok token of text under "%.<prec>s", "(null)" when missing (rtlsdr_ft8d.c:1509-1514)"""
    toks = text.split()
    return (toks[k] if k < len(toks) else "(null)")[:prec]


def test_whole_path_config2(oracle):
    """configs[2] (4096 frames, device pointers): decode_messages == collect_messages on the device's own stage outputs,
    n_msgs == n_results of decode_batch, and every CQ record agrees with decode_batch's spot"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B, cap = 4096, 120
    with ft8.Decoder(device=0, max_frames=B) as dec:
        iq = _synth_config2(ft8, workload, dec, B)
        spots0, nres0 = _spots_dev(ft8, dec, iq, B)
        got, n = _messages_dev(ft8, dec, iq, B)
        spots1, nres1 = _spots_dev(ft8, dec, iq, B)
        # decode_batch is byte-identical before and after a decode_messages call on the same context
        assert spots0.tobytes() == spots1.tobytes() and np.array_equal(nres0, nres1)
        assert np.array_equal(n, nres0) and n.sum() > 20000
        # the stage chain on the device
        mag = torch.empty((B, ft8.MAG_ARRAY), dtype=torch.uint8, device="cuda")
        cands = torch.zeros((B, cap * 8), dtype=torch.uint8, device="cuda")
        counts = torch.zeros((B,), dtype=torch.int32, device="cuda")
        status = torch.zeros((B, cap * 48), dtype=torch.uint8, device="cuda")
        msgs2 = torch.zeros((B, 50 * 64), dtype=torch.uint8, device="cuda")
        n2 = torch.zeros((B,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.waterfall_dev(iq, B, mag)
        dec.find_sync_dev(mag, B, cands, counts)
        dec.decode_candidates_dev(mag, cands, counts, B, status)
        dec.collect_messages_dev(mag, cands, counts, status, B, msgs2, n2)
        dec.synchronize()
        st_msgs = msgs2.cpu().numpy().view(ft8.MESSAGE_DTYPE).reshape(B, 50)
        assert spec.check(got, n, st_msgs, n2.cpu().numpy()) is None
        # the restatement on a slice of the device's own stage outputs
        sl = slice(0, 96)
        m_h = mag[sl].cpu().numpy()
        c_h = cands[sl].cpu().numpy().view(ft8.CAND_DTYPE).reshape(-1, cap)
        k_h = counts[sl].cpu().numpy()
        s_h = status[sl].cpu().numpy().view(ft8.STATUS_DTYPE).reshape(-1, cap)
        want, wn = spec.collect(m_h, c_h, k_h, s_h)
        assert spec.check(got[sl], n[sl], want, wn) is None, spec.check(got[sl], n[sl], want, wn)
    # CQ records against decode_batch's spots
    checked = 0
    for f in range(B):
        for j in range(int(n[f])):
            r = got[f, j]
            text = r["text"].decode()
            if not text.startswith("CQ"):
                continue
            s = spots0[f, j]
            assert s["call"].decode() == _c_field(text, 1, 12) and s["loc"].decode() == _c_field(text, 2, 6), (text, s)
            assert s["freq"] == np.int32(np.float32(r["freq_hz"])) and s["snr"] == r["score"]
            checked += 1
    assert checked > 20000


def test_forms_chunking_and_guard_bands(oracle):
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    texts, tones = workload.mixed_message_pool(256, seed=8)
    iq = _mixed_frames(texts, tones, 13, 12, (-12.0, 8.0), 900)
    with ft8.Decoder(device=0, max_frames=5) as dec:                 # 13 frames: three chunks, the last ragged
        fill = np.full((13, 50 * 64), GUARD, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(13, 50)
        h, hn = dec.decode_messages(iq, fill.copy())
        iq_d = torch.from_numpy(iq).cuda()
        d, dn = _messages_dev(ft8, dec, iq_d, 13, fill=GUARD)
        assert np.array_equal(hn, dn) and h.tobytes() == d.tobytes()   # untouched slots keep the caller's bytes in both forms
        for f in range(13):
            assert h[f, hn[f]:].tobytes() == bytes([GUARD]) * (64 * (50 - hn[f]))
        # guard bands around msgs / n_msgs / base at ragged sizes (device form)
        for nfr in (1, 3, 7):
            pad = 256
            mbuf = torch.full((2 * pad + nfr * 50 * 64,), GUARD, dtype=torch.uint8, device="cuda")
            nbuf = torch.full((2 * pad + 4 * nfr,), GUARD, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dec.decode_messages_dev(iq_d, nfr, mbuf.data_ptr() + pad, nbuf.data_ptr() + pad)
            dec.synchronize()
            mb, nb = mbuf.cpu().numpy(), nbuf.cpu().numpy()
            assert (mb[:pad] == GUARD).all() and (mb[-pad:] == GUARD).all()
            assert (nb[:pad] == GUARD).all() and (nb[-pad:] == GUARD).all()
            assert np.array_equal(nb[pad:pad + 4 * nfr].view(np.int32), hn[:nfr])
            mag_d = torch.from_numpy(oracle.waterfall_batch(iq[:nfr], nthreads=8)).cuda()
            bbuf = torch.full((2 * pad + 512 * nfr,), GUARD, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dec.noise_baseline_dev(mag_d, nfr, bbuf.data_ptr() + pad)
            dec.synchronize()
            bb = bbuf.cpu().numpy()
            assert (bb[:pad] == GUARD).all() and (bb[-pad:] == GUARD).all()
            assert np.array_equal(bb[pad:pad + 512 * nfr].reshape(nfr, 2, 256), spec.noise_baseline(mag_d.cpu().numpy()))


def test_max_frames_one_agrees_with_one_large_call():
    """4097 frames through a context of max_frames = 1 == one call on a context that takes them all"""
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B = 4097
    with ft8.Decoder(device=0, max_frames=B) as big:
        iq = _synth_config2(ft8, workload, big, B)
        a, an = _messages_dev(ft8, big, iq, B)
        with ft8.Decoder(device=0, max_frames=1) as one:
            b, bn = _messages_dev(ft8, one, iq, B)
    assert np.array_equal(an, bn) and a.tobytes() == b.tobytes()


def test_snr_and_dt_accuracy_on_the_device():
    """synth_frames, one CQ signal per frame, 64 frames at each of -18, -12, -6, 0, +10, +20 dB: >= 95 % of the decodes
    within 2 dB of the truth, median |error| <= 1 dB; dt_s within 0.16 s of s0 / 3200 + d0"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    d0 = json.load(open(os.path.join(ROOT, "profiles", "snr_calibration.json")))["d0_s"]
    levels = [-18.0, -12.0, -6.0, 0.0, 10.0, 20.0]
    per = 64
    B = per * len(levels)
    texts, tones = workload.message_pool(B, seed=21)
    rng = np.random.default_rng(77)
    sig = np.zeros((B, 1), ft8.SIGNAL_DTYPE)
    truth = np.repeat(levels, per)
    sig[:, 0]["tones"] = tones
    sig[:, 0]["f0_hz"] = rng.uniform(100.0, 1500.0, B)
    sig[:, 0]["t0_s"] = rng.integers(0, int(1.8 * 3200), B) / 3200.0
    sig[:, 0]["amplitude"] = workload.amplitude_for_snr(truth)
    s0 = np.array([int(np.rint(np.float32(t) * np.float32(3200.0))) for t in sig[:, 0]["t0_s"]])
    with ft8.Decoder(device=0, max_frames=B) as dec:
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, 1, 1.0, 0x534E5231, iq)
        dec.synchronize()
        got, n = _messages_dev(ft8, dec, iq, B)
    err, dts = [], []
    for f in range(B):
        for r in got[f, :n[f]]:
            if r["text"].decode() == texts[f]:
                err.append(int(r["snr_db"]) - truth[f])
                dts.append(float(r["dt_s"]) - (s0[f] / 3200.0 + d0))
    err, dts = np.abs(np.array(err)), np.abs(np.array(dts))
    assert len(err) >= 5 * per, len(err)
    assert (err <= 2.0).mean() >= 0.95 and np.median(err) <= 1.0, (np.median(err), (err <= 2.0).mean())
    assert dts.max() <= 0.16, dts.max()
