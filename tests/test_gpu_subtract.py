"""GPU tests of the subtraction in the I/Q samples (ft8gpu_subtract_messages, ft8gpu_decode_messages_subtracted) against the numpy
restatement tests/ft8_spec_subtract.py, byte for byte: crowded frames through the whole path at three passes on a context of two
frames (three chunks, the last ragged), host and device pointers; the committed uncovering seeds; the hand-made records of
tests/subtract_craft.py through the stage entry (windows that leave the frame, every choice of the fine search, R.valid = 0,
counts of 0, 3 and 50, first > 0, overlapping records, a frame of zeros, in place); and the product paths' records before and
after subtraction calls on the same context.  tests/test_subtract_cpu.py proves on the CPU that the hand-made records are what
they are named for."""
import hashlib

import numpy as np
import pytest

import ft8_spec_subtract as ss
import subtract_craft as sc

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, sc.FILL


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


def filled_msgs(ft8, B):
    return np.full((B, 50 * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(B, 50)


def first_difference(got, want, n):
    for f in range(len(n)):
        for i in range(50):
            if got[f, i].tobytes() != want[f, i].tobytes():
                return f"frame {f} slot {i} (count {int(n[f])}): {got[f, i]} != {want[f, i]}"
    return None


def sample_difference(got, want):
    d = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return None if len(d) == 0 else f"{len(d)} samples differ, the first at {d[0].tolist()}: {got[tuple(d[0])]!r} != {want[tuple(d[0])]!r}"


# ---- (i) the whole path -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def radio(oracle):
    """5 frames of 6 off-grid signals within 100 Hz of each other, and the restatement at 3 passes: two frames gain in both later
    passes, one in pass 2 only, one in neither, one decodes nothing at all"""
    import rtlsdr_ft8d_amd as ft8
    import synth_util as su
    enc = su.oracle_encode_fn(oracle)
    iq = np.stack([su.make_frame(410000 + k, 6, enc, snr_range=(-16.0, 6.0), f_range=(900.0, 1000.0))[0] for k in range(5)])
    msgs, n, nbp, res = ss.decode_passes_subtracted(oracle, iq, 3, msgs=filled_msgs(ft8, 5))
    assert nbp.tolist() == [[1, 1, 1], [2, 3, 3], [1, 3, 4], [2, 3, 4], [0, 0, 0]]
    for a in (iq, msgs, n, nbp, res):
        a.setflags(write=False)
    return iq, msgs, n, nbp, res


@pytest.mark.parametrize("form", ["host", "device"])
def test_whole_path_equals_the_restatement(radio, form):
    """max_frames = 2 under 5 frames: three chunks, the last of one frame; slots behind the counts keep their 0xA5"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, n, nbp, res = radio
    B = len(n)
    with ft8.Decoder(device=0, max_frames=2) as dec:
        one_m, one_n = dec.decode_messages(iq, msgs=filled_msgs(ft8, B))
        if form == "host":
            got_m, got_n, got_nbp, got_res = dec.decode_messages_subtracted(iq, passes=3, msgs=filled_msgs(ft8, B))
            p1_m, p1_n, p1_nbp, p1_res = dec.decode_messages_subtracted(iq, passes=1, msgs=filled_msgs(ft8, B))
        else:
            def run(passes):
                iq_d, m_b, n_b = up(iq), guarded(filled_msgs(ft8, B)), guarded(np.zeros(B, np.int32))
                nbp_b, r_b = guarded(np.zeros((B, passes), np.int32)), guarded(np.zeros_like(iq))
                torch.cuda.synchronize()
                dec.decode_messages_subtracted_dev(iq_d, B, passes, m_b[GUARD:], n_b[GUARD:], nbp_b[GUARD:], r_b[GUARD:])
                dec.synchronize()
                assert iq_d.cpu().numpy().tobytes() == iq.tobytes()                      # the caller's frames are never written
                return (unguard(m_b, B * 50 * 64).view(ft8.MESSAGE_DTYPE).reshape(B, 50), unguard(n_b, 4 * B).view(np.int32),
                        unguard(nbp_b, 4 * B * passes).view(np.int32).reshape(B, passes), unguard(r_b, iq.nbytes).view(np.float32).reshape(iq.shape))
            got_m, got_n, got_nbp, got_res = run(3)
            p1_m, p1_n, p1_nbp, p1_res = run(1)
            # without the optional outputs the records are the same
            iq_d, m_b, n_b = up(iq), guarded(filled_msgs(ft8, B)), guarded(np.zeros(B, np.int32))
            torch.cuda.synchronize()
            dec.decode_messages_subtracted_dev(iq_d, B, 3, m_b[GUARD:], n_b[GUARD:])
            dec.synchronize()
            assert unguard(m_b, B * 50 * 64).tobytes() == got_m.tobytes() and unguard(n_b, 4 * B).tobytes() == got_n.tobytes()
    assert got_nbp.tolist() == nbp.tolist() and (got_n == n).all()
    assert got_m.tobytes() == msgs.tobytes(), first_difference(got_m, msgs, n)
    assert got_res.tobytes() == res.tobytes(), sample_difference(got_res, res)
    behind = np.arange(50)[None, :] >= n[:, None]
    assert (got_m.view(np.uint8).reshape(B, 50, 64)[behind] == FILL).all()
    # passes = 1 is ft8gpu_decode_messages, and the residual the frames themselves; slots [0, n1) always are its records
    assert p1_m.tobytes() == one_m.tobytes() and (p1_n == one_n).all() and p1_nbp[:, 0].tolist() == one_n.tolist()
    assert p1_res.tobytes() == iq.tobytes()
    for f in range(B):
        assert got_m[f, :one_n[f]].tobytes() == one_m[f, :one_n[f]].tobytes() and nbp[f, 0] == one_n[f]


# ---- (ii) the committed uncovering seeds --------------------------------------------------------------------------------------------------

def test_uncovering_seeds_on_the_device(oracle):
    """the weak message is in the device's records, and the records are the restatement's"""
    import rtlsdr_ft8d_amd as ft8
    iq = np.stack([sc.uncover_frame(oracle, s) for s in sc.UNCOVER_SEEDS])
    B = len(iq)
    want_m, want_n, want_nbp, want_res = ss.decode_passes_subtracted(oracle, iq, 2, msgs=filled_msgs(ft8, B))
    with ft8.Decoder(device=0, max_frames=4) as dec:
        got_m, got_n, got_nbp, got_res = dec.decode_messages_subtracted(iq, passes=2, msgs=filled_msgs(ft8, B))
        msk_m, msk_n, _nbp = dec.decode_messages_passes(iq, passes=2)
    assert (got_n == want_n).all() and got_nbp.tolist() == want_nbp.tolist()
    assert got_m.tobytes() == want_m.tobytes(), first_difference(got_m, want_m, want_n)
    assert got_res.tobytes() == want_res.tobytes(), sample_difference(got_res, want_res)
    for seed, texts, masked in zip(sc.UNCOVER_SEEDS, sc.texts_of(got_m, got_n), sc.texts_of(msk_m, msk_n)):
        assert texts == [sc.STRONG_TEXT, sc.WEAK_TEXT], (seed, texts)
        assert sc.WEAK_TEXT not in masked, (seed, masked)


# ---- (iii) hand-made records through the stage entry ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def constructed():
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, refined, first, n, where = sc.constructed(ft8)
    fill = np.full((6, 50 * 64), FILL, np.uint8).view(ss.INFO_DTYPE).reshape(6, 50)
    out, info = ss.subtract(iq, msgs, refined, first, n, ss.twiddles(), info=fill)
    for a in (iq, msgs, refined, first, n, fill, out, info):
        a.setflags(write=False)
    return iq, msgs, refined, first, n, where, fill, out, info


@pytest.mark.parametrize("form", ["host", "device", "device_in_place"])
def test_stage_entry_equals_the_restatement_on_constructed_records(constructed, form):
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, refined, first, n, where, fill, want_out, want_info = constructed
    B = 6
    with ft8.Decoder(device=0, max_frames=4 if form == "host" else 6) as dec:
        if form == "host":
            got_out, got_info = dec.subtract_messages(iq, msgs, refined, first, n, info=fill.copy())
            no_info, none = dec.subtract_messages(iq, msgs, refined, first, n, want_info=False)
            assert none is None and no_info.tobytes() == got_out.tobytes()
        else:
            ins = [up(a) for a in (msgs, refined, first, n)]
            x_b, i_b = guarded(iq), guarded(fill)
            o_b = x_b if form == "device_in_place" else guarded(np.zeros_like(iq))
            torch.cuda.synchronize()
            dec.subtract_messages_dev(x_b[GUARD:], ins[0], ins[1], ins[2], ins[3], B, o_b[GUARD:], i_b[GUARD:])
            dec.synchronize()
            for a, b in zip((msgs, refined, first, n), ins):
                assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()          # inputs are inputs
            if form == "device":
                assert unguard(x_b, iq.nbytes).tobytes() == iq.tobytes()
            got_out = unguard(o_b, iq.nbytes).view(np.float32).reshape(iq.shape)
            got_info = unguard(i_b, fill.nbytes).view(ss.INFO_DTYPE).reshape(B, 50)
    names = {v: k for k, v in where.items()}
    for f in range(B):
        for i in range(50):
            assert got_info[f, i].tobytes() == want_info[f, i].tobytes(), (names.get((f, i)), f, i, got_info[f, i], want_info[f, i])
    assert got_out.tobytes() == want_out.tobytes(), sample_difference(got_out, want_out)
    for f in (1, 2, 4):                                                   # counts of 0, a frame of zeros, first >= n_msgs: bit for bit
        assert got_out[f].tobytes() == iq[f].tobytes()
    raw = got_info.view(np.uint8).reshape(B, 50, 64)
    assert (raw[1] == FILL).all() and (raw[2, 3:] == FILL).all() and (raw[3, :2] == FILL).all() and (raw[4] == FILL).all()
    assert got_info[where["not_valid"]].tobytes() == bytes(64)
    for name, d, t in (("truth_d+2_t+2", 2, 2), ("truth_d-2_t-2", -2, -2), ("truth_d+2_t-2_u1", 2, -2), ("truth_d-2_t+2_u3", -2, 2)):
        r = got_info[where[name]]
        assert (r["valid"], r["d_best"], r["t_best"]) == (1, d, t), name


# ---- (iv) the product paths are not moved ----------------------------------------------------------------------------------------------------

def test_product_records_are_unchanged_by_subtraction_calls():
    """ft8gpu_decode_batch, ft8gpu_decode_messages and ft8gpu_decode_messages_passes on 64 frames, before and after subtraction
    calls on the same context"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B, S = 64, 20
    _texts, tones = workload.message_pool()
    sig, _picks = workload.frame_signals(0, B, S, tones, snr_range=(-18.0, 0.0))

    def digest(dec, iq):
        spots = torch.zeros((B, 50 * 28), dtype=torch.uint8, device="cuda")
        nres = torch.zeros((B,), dtype=torch.int32, device="cuda")
        msgs = torch.zeros((B, 50 * 64), dtype=torch.uint8, device="cuda")
        nm = torch.zeros((B,), dtype=torch.int32, device="cuda")
        pm = torch.zeros((B, 50 * 64), dtype=torch.uint8, device="cuda")
        pn = torch.zeros((B,), dtype=torch.int32, device="cuda")
        pbp = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_batch_dev(iq, B, spots, nres)
        dec.decode_messages_dev(iq, B, msgs, nm)
        dec.decode_messages_passes_dev(iq, B, 3, pm, pn, pbp)
        dec.synchronize()
        h = hashlib.sha256()
        for t in (spots, nres, msgs, nm, pm, pn, pbp):
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest(), msgs, nm, int(pn.sum().item())

    with ft8.Decoder(device=0, max_frames=B) as dec:
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, S, 1.0, workload.SEED_BASE, iq, first_frame=0)
        dec.synchronize()
        keep = iq.clone()
        before, msgs, nm, masked_total = digest(dec, iq)
        sm_, sn = torch.zeros_like(msgs), torch.zeros_like(nm)
        sbp = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
        res = torch.zeros_like(iq)
        ref = torch.zeros((B, 50 * 48), dtype=torch.uint8, device="cuda")
        zero = torch.zeros((B,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_messages_subtracted_dev(iq, B, 3, sm_, sn, sbp, res)
        dec.refine_messages_dev(iq, msgs, nm, B, ref)
        dec.subtract_messages_dev(iq, msgs, ref, zero, nm, B, res)
        dec.synchronize()
        assert torch.equal(iq, keep)
        first_pass = sbp[:, 0].cpu().numpy()
        assert (first_pass == nm.cpu().numpy()).all() and int(sn.sum().item()) > int(nm.sum().item())
        print("records after 3 passes: masking", masked_total, "subtraction", int(sn.sum().item()), "first pass", int(nm.sum().item()))
        after, _m, _n, _t = digest(dec, iq)
    assert before == after
