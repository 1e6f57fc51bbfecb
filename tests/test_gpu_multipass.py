"""GPU tests of multi-pass decoding (ft8gpu_decode_messages_passes / ft8gpu_mask_messages / ft8gpu_append_messages): the
stage entries and the whole path against the numpy restatement (tests/ft8_spec_multipass.py) on oracle-made inputs, byte
for byte with every output pre-filled with 0xA5; passes=1 against ft8gpu_decode_messages; chunking; the gain on crowded
frames; argument errors; four passes."""
import numpy as np
import pytest

import ft8_spec_messages as sm
import ft8_spec_multipass as spec

pytestmark = pytest.mark.gpu
FILL = 0xA5


def _filled(B):
    import rtlsdr_ft8d_amd as ft8
    return np.full((B, 50 * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(B, 50)


def _cq_frames(oracle, seeds, nsig, snr=(-22.0, 0.0)):
    import synth_util as S
    enc = S.oracle_encode_fn(oracle)
    fr = [S.make_frame(s, nsig, enc, snr_range=snr) for s in seeds]
    return np.stack([f[0] for f in fr]), [f[1] for f in fr]


def _mixed_frames(nframes, nsig, seed):
    import synth_util as S
    from rtlsdr_ft8d_amd import workload
    texts, tones = workload.mixed_message_pool(256, seed=3)
    return np.stack([S.make_mixed_frame(seed + k, nsig, (-16.0, 6.0), texts, tones)[0] for k in range(nframes)])


def _noise_frames(nframes, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 0.1, (nframes, 2, 48000)).astype(np.float32)


def _ragged_batch(oracle):
    """crowded frames (30 signals), single-signal frames and pure-noise frames interleaved: the compaction has gaps"""
    crowded, _ = _cq_frames(oracle, range(5000, 5010), 30)
    single, _ = _cq_frames(oracle, range(6000, 6006), 1, snr=(-12.0, 0.0))
    noise = _noise_frames(6, 7)
    order = [crowded[0], noise[0], single[0], crowded[1], crowded[2], noise[1], single[1], crowded[3], noise[2], noise[3],
             single[2], crowded[4], crowded[5], single[3], noise[4], crowded[6], single[4], crowded[7], noise[5], crowded[8],
             single[5], crowded[9]]
    return np.stack(order)


def _dev_passes(ft8, dec, iq_d, B, passes, nbp=True):
    import torch
    msgs = torch.full((B, 50 * 64), FILL, dtype=torch.uint8, device="cuda")
    n = torch.full((B,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    nb = torch.full((B, passes), -0x5A5A5A5B, dtype=torch.int32, device="cuda") if nbp else None
    torch.cuda.synchronize()
    dec.decode_messages_passes_dev(iq_d, B, passes, msgs, n, nb)
    dec.synchronize()
    m = msgs.cpu().numpy().view(ft8.MESSAGE_DTYPE).reshape(B, 50)
    return m, n.cpu().numpy(), (nb.cpu().numpy() if nbp else None)


def test_one_pass_equals_decode_messages(oracle):
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = np.concatenate([_mixed_frames(7, 14, 100), _cq_frames(oracle, range(110, 116), 20)[0]])
    B = len(iq)
    with ft8.Decoder(device=0, max_frames=5) as dec:
        want, wn = dec.decode_messages(iq, _filled(B))
        got, n, nbp = dec.decode_messages_passes(iq, 1, _filled(B))
        assert np.array_equal(n, wn) and got.tobytes() == want.tobytes() and np.array_equal(nbp[:, 0], wn)
        iq_d = torch.from_numpy(iq).cuda()
        dm, dn, dnb = _dev_passes(ft8, dec, iq_d, B, 1)
        assert np.array_equal(dn, wn) and dm.tobytes() == want.tobytes() and np.array_equal(dnb[:, 0], wn)
    assert wn.sum() > 60


def _pass1(oracle, iq, cap=120):
    stages = sm.oracle_stages(oracle, iq, max_candidates=cap)
    msgs, n = sm.collect(*stages, msgs=_filled(len(iq)))
    return stages, msgs, n


def test_mask_equals_restatement(oracle):
    """64 CQ frames and 64 mixed-traffic frames; first[f] anywhere in [0, n[f]], plus out-of-range first / n values"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = np.concatenate([_cq_frames(oracle, range(200, 264), 20, snr=(-16.0, 4.0))[0], _mixed_frames(64, 14, 300)])
    B = len(iq)
    (mag, _, _, _), msgs, n = _pass1(oracle, iq)
    base = sm.noise_baseline(mag)
    rng = np.random.default_rng(5)
    first = np.array([rng.integers(0, k + 1) for k in n], np.int32)
    first[3], n[3] = -4, n[3]                                          # first < 0: from 0
    first[5], n[5] = n[5] + 2, n[5]                                    # first > n: nothing
    first[7] = 0                                                       # every record
    n[9] = 77                                                          # n > 50: up to 50 (slots past the count are 0xA5 bytes)
    want = spec.mask(mag, base, msgs, first, n)
    assert (want != mag).any(axis=1).sum() > 100
    with ft8.Decoder(device=0, max_frames=48) as dec:                  # 128 frames: chunked
        got = dec.mask_messages(mag, base, msgs, first, n)
        assert got.tobytes() == want.tobytes()
        out = torch.full((B, ft8.MAG_ARRAY), FILL, dtype=torch.uint8, device="cuda")
        ins = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (mag, base, msgs.view(np.uint8), first, n)]
        torch.cuda.synchronize()
        dec.mask_messages_dev(*ins, B, out)
        dec.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes()
        dec.mask_messages_dev(ins[0], *ins[1:], B, ins[0])               # in place
        dec.synchronize()
        assert ins[0].cpu().numpy().tobytes() == want.tobytes()


def test_append_equals_restatement(oracle):
    """pass-2 stage outputs of masked waterfalls, and by hand: a frame already holding 50 records, frames whose messages
    are all found again (deduped; half of them re-appended where the records were cut in two), a frame without candidates"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = np.concatenate([_cq_frames(oracle, range(400, 410), 30)[0], _mixed_frames(6, 16, 420)])
    B, cap = len(iq), 120
    (mag, c1, k1, s1), msgs, n = _pass1(oracle, iq, cap)
    base = sm.noise_baseline(mag)
    W2 = spec.mask(mag, base, msgs, np.zeros(B, np.int32), n)
    c2, k2 = oracle.find_sync_batch(W2, cap, 10, nthreads=8)
    s2 = oracle.decode_candidates_batch(W2, c2, k2, nthreads=8)
    s2 = s2.view(ft8.STATUS_DTYPE).reshape(B, cap)
    s1 = s1.view(ft8.STATUS_DTYPE).reshape(B, cap)
    # frame 0: 50 records (the frame's own, then those of frames 1.. up to 50)
    pool = np.concatenate([msgs[f, :n[f]] for f in range(B)])
    msgs[0] = pool[:50]
    n[0] = 50
    # frame 1: the pass-1 candidates again: every message already known
    c2[1], k2[1], s2[1] = c1[1], k1[1], s1[1]
    # frame 2: the same with only the first half of the records kept: the second half comes back, in candidate order
    c2[2], k2[2], s2[2] = c1[2], k1[2], s1[2]
    n[2] = n[2] // 2
    # frame 3: no candidates
    k2[3] = 0
    want, wn = spec.append(W2, base, c2, k2, s2, msgs, n)
    assert wn[0] == 50 and wn[1] == n[1] and wn[2] > n[2] and wn[3] == n[3]
    assert (wn - n)[4:].sum() >= 1, wn - n
    with ft8.Decoder(device=0, max_frames=6, max_candidates=cap) as dec:      # 16 frames: chunked
        got, gn = dec.append_messages(W2, base, c2, k2, s2, msgs, n)
        assert np.array_equal(gn, wn) and got.tobytes() == want.tobytes(), sm.check(got, gn, want, wn)
        ins = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda() for a in (W2, base, c2, k2, s2)]
        m_d = torch.from_numpy(np.ascontiguousarray(msgs).view(np.uint8)).cuda()
        n_d = torch.from_numpy(n.copy()).cuda()
        torch.cuda.synchronize()
        dec.append_messages_dev(*ins, B, m_d, n_d)
        dec.synchronize()
        assert np.array_equal(n_d.cpu().numpy(), wn)
        assert m_d.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("cap", [120, 7])
@pytest.mark.parametrize("passes", [2, 3])
def test_whole_path_equals_restatement(oracle, cap, passes):
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = _ragged_batch(oracle)
    B = len(iq)
    want, wn, wnbp = spec.decode_passes(oracle, iq, passes, max_candidates=cap, msgs=_filled(B))
    if cap == 120:
        assert (wnbp[:, -1] > wnbp[:, 0]).sum() >= 2                   # later passes find something
    with ft8.Decoder(device=0, max_frames=B, max_candidates=cap) as dec:
        got, n, nbp = dec.decode_messages_passes(iq, passes, _filled(B))
        assert np.array_equal(n, wn) and np.array_equal(nbp, wnbp), (n, wn, nbp, wnbp)
        assert got.tobytes() == want.tobytes(), sm.check(got, n, want, wn)
        dm, dn, dnb = _dev_passes(ft8, dec, torch.from_numpy(iq).cuda(), B, passes)
        assert np.array_equal(dn, wn) and np.array_equal(dnb, wnbp) and dm.tobytes() == want.tobytes()


def test_chunking_and_single_frames(oracle):
    """max_frames 7 walking 20 frames == one call; every frame decoded alone == the batch"""
    import rtlsdr_ft8d_amd as ft8
    iq = _ragged_batch(oracle)[:20]
    with ft8.Decoder(device=0, max_frames=20) as dec:
        a, an, anb = dec.decode_messages_passes(iq, 3, _filled(20))
    with ft8.Decoder(device=0, max_frames=7) as dec:
        b, bn, bnb = dec.decode_messages_passes(iq, 3, _filled(20))
        assert np.array_equal(an, bn) and np.array_equal(anb, bnb) and a.tobytes() == b.tobytes()
        for f in range(20):
            m, k, kb = dec.decode_messages_passes(iq[f:f + 1], 3, _filled(1))
            assert k[0] == an[f] and np.array_equal(kb[0], anb[f]) and m.tobytes() == a[f:f + 1].tobytes(), f
    assert (anb[:, 1] > anb[:, 0]).any()


def test_large_batch_against_restatement_at_both_ends(oracle):
    """4096 synthesised frames in one call (two-part first pass, ranks up to 4095) == max_frames 1000; the first and the
    last 32 frames == the restatement"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B = 4096
    _, tones = workload.message_pool()
    sig, _ = workload.frame_signals(0, B, 20, tones, snr_range=(-18.0, 0.0))
    with ft8.Decoder(device=0, max_frames=B) as dec:
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, 20, 1.0, workload.SEED_BASE, iq)
        dec.synchronize()
        a, an, anb = _dev_passes(ft8, dec, iq, B, 3)
        with ft8.Decoder(device=0, max_frames=1000) as small:
            b, bn, bnb = _dev_passes(ft8, small, iq, B, 3)
        host = torch.cat([iq[:32], iq[-32:]]).cpu().numpy()
    assert np.array_equal(an, bn) and np.array_equal(anb, bnb) and a.tobytes() == b.tobytes()
    assert anb[:, 1].sum() > anb[:, 0].sum()
    want, wn, wnbp = spec.decode_passes(oracle, host, 3, msgs=_filled(64))
    sel = np.r_[0:32, B - 32:B]
    assert np.array_equal(an[sel], wn) and np.array_equal(anb[sel], wnbp)
    assert a[sel].tobytes() == want.tobytes(), sm.check(a[sel], an[sel], want, wn)


def test_gain_on_crowded_frames(oracle):
    """96 frames of 30 CQ signals (seeds 1000..1095, SNR U[-22, 0] dB): passes=2 finds strictly more of the planted
    messages than passes=1, exactly as many as the restatement, and nothing outside the planted set"""
    import rtlsdr_ft8d_amd as ft8
    iq, planted = _cq_frames(oracle, range(1000, 1096), 30)
    want, wn, wnbp = spec.decode_passes(oracle, iq, 2)
    with ft8.Decoder(device=0, max_frames=96) as dec:
        one, n1, _ = dec.decode_messages_passes(iq, 1)
        two, n2, nbp = dec.decode_messages_passes(iq, 2)
    h1, m1 = spec.planted_hits(one, n1, planted)
    h2, m2 = spec.planted_hits(two, n2, planted)
    hw, mw = spec.planted_hits(want, wn, planted)
    assert h2 > h1 and h2 == hw and m1 == m2 == mw == 0, (h1, h2, hw, m1, m2, mw)
    assert np.array_equal(nbp[:, 0], n1) and np.array_equal(n2, wn)
    print(f"planted messages decoded: pass 1 {h1}, after pass 2 {h2} (+{100.0 * (h2 - h1) / h1:.1f} %)")


def test_argument_errors_and_null_counts_table(oracle):
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = _mixed_frames(3, 10, 700)
    with ft8.Decoder(device=0, max_frames=4) as dec:
        for bad in (0, 5, -1):
            with pytest.raises(ft8.Ft8GpuError, match="passes"):
                dec.decode_messages_passes(iq, bad)
        a, an, anb = dec.decode_messages_passes(iq, 2, _filled(3))
        # n_by_pass NULL, host form
        m, n = _filled(3), np.zeros(3, np.int32)
        assert dec.lib.ft8gpu_decode_messages_passes(dec.h, iq.ctypes.data, 3, 2, m.ctypes.data, n.ctypes.data, None, ft8.HOST_PTRS) == 0
        assert np.array_equal(n, an) and m.tobytes() == a.tobytes()
        # and device form
        dm, dn, _ = _dev_passes(ft8, dec, torch.from_numpy(iq).cuda(), 3, 2, nbp=False)
        assert np.array_equal(dn, an) and dm.tobytes() == a.tobytes()
        # NULL arrays are refused
        assert dec.lib.ft8gpu_decode_messages_passes(dec.h, iq.ctypes.data, 3, 2, None, n.ctypes.data, None, ft8.HOST_PTRS) != 0
        assert b"NULL" in dec.lib.ft8gpu_last_error()


def test_four_passes_equal_restatement(oracle):
    """FT8GPU_MAX_PASSES = 4 on the 30-signal frames among single-signal and noise frames: the restatement, host and device
    form; frames on which pass 3 finds nothing, alone in a call as well -- there the pass loop leaves early and the counts are
    carried into the passes that did not run"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = _ragged_batch(oracle)
    B = len(iq)
    want, wn, wnbp = spec.decode_passes(oracle, iq, 4, msgs=_filled(B))
    print("n_by_pass", wnbp.tolist())
    stops = [f for f in range(B) if wnbp[f, 1] > wnbp[f, 0] and wnbp[f, 2] == wnbp[f, 1]]
    assert stops and (wnbp[:, 1] > wnbp[:, 0]).sum() >= 2 and (wnbp[:, 3] == wnbp[:, 0]).any()
    with ft8.Decoder(device=0, max_frames=B) as dec:
        got, n, nbp = dec.decode_messages_passes(iq, 4, _filled(B))
        assert np.array_equal(n, wn) and np.array_equal(nbp, wnbp), (n, wn, nbp.tolist(), wnbp.tolist())
        assert got.tobytes() == want.tobytes(), sm.check(got, n, want, wn)
        dm, dn, dnb = _dev_passes(ft8, dec, torch.from_numpy(iq).cuda(), B, 4)
        assert np.array_equal(dn, wn) and np.array_equal(dnb, wnbp) and dm.tobytes() == want.tobytes()
        for f in stops[:3] + [1]:                                      # 1: a noise frame, the loop leaves before pass 2
            m, k, kb = dec.decode_messages_passes(iq[f:f + 1], 4, _filled(1))
            assert k[0] == wn[f] and np.array_equal(kb[0], wnbp[f]) and m.tobytes() == want[f:f + 1].tobytes(), f
