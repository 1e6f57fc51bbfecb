"""GPU tests of the refined time and frequency (ft8gpu_refine_messages, ft8gpu_decode_messages_refined) against the numpy
restatement tests/ft8_spec_refine.py, byte for byte: radio frames through the whole path on a context of two frames (three
chunks, the last ragged), host and device pointers; the constructed records of tests/refine_craft.py through the stage entry
(windows that leave the frame at both ends, the truth on either edge of the search, counts of 0 and 50, a frame of zeros);
the float edges, samples that are not finite and ties of tests/iq_edges_craft.py; the radio frames spread over 259 frames on a
context of 260; and the product path's records before and after a refine call on the same context.  tests/test_refine_cpu.py
and tests/test_iq_edges_cpu.py prove on the CPU that the constructed records are what they are named for."""
import hashlib

import numpy as np
import pytest

import ft8_spec_refine as sr
import iq_edges_craft as ec
import refine_craft as rc

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, rc.FILL


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


def first_difference(got, want, n):
    for f in range(len(n)):
        for i in range(50):
            if got[f, i].tobytes() != want[f, i].tobytes():
                return f"frame {f} slot {i} (n_msgs {int(n[f])}): {got[f, i]} != {want[f, i]}"
    return None


def filled(ft8, B):
    return (np.full((B, 50 * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(B, 50),
            np.full((B, 50 * 48), FILL, np.uint8).view(ft8.REFINED_DTYPE).reshape(B, 50))


# ---- radio frames through the whole path ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def radio(oracle):
    """5 frames of 6 off-grid signals each from the device's synthesiser, what ft8gpu_decode_messages alone returns for them,
    and the restatement on those records"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B, S = 5, 6
    _texts, tones = workload.message_pool()
    sig, _picks = workload.frame_signals(310000, B, S, tones, snr_range=(-12.0, 3.0))
    msgs0, ref0 = filled(ft8, B)
    with ft8.Decoder(device=0, max_frames=B) as dec:
        iq_dev = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, S, 1.0, workload.SEED_BASE + 31, iq_dev, first_frame=310000)
        dec.synchronize()
        iq = iq_dev.cpu().numpy()
        msgs, n = dec.decode_messages(iq, msgs=msgs0.copy())
    assert n.sum() >= 15 and n.min() >= 1, n
    want = sr.refine(iq, msgs, n, sr.twiddles(oracle), refined=ref0)
    for a in (iq, msgs, n, want):
        a.setflags(write=False)
    return iq, msgs, n, want


@pytest.mark.parametrize("form", ["host", "device"])
def test_whole_path_equals_decode_messages_and_the_restatement(radio, form):
    """max_frames = 2 under 5 frames: three chunks, the last of one frame; slots behind the counts keep their 0xA5"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, n, want = radio
    B = len(n)
    msgs0, ref0 = filled(ft8, B)
    with ft8.Decoder(device=0, max_frames=2) as dec:
        if form == "host":
            got_m, got_n, got_r = dec.decode_messages_refined(iq, msgs=msgs0, refined=ref0)
        else:
            iq_d, m_b, r_b, n_b = up(iq), guarded(msgs0), guarded(ref0), guarded(np.zeros(B, np.int32))
            torch.cuda.synchronize()
            dec.decode_messages_refined_dev(iq_d, B, m_b[GUARD:], n_b[GUARD:], r_b[GUARD:])
            dec.synchronize()
            assert iq_d.cpu().numpy().tobytes() == iq.tobytes()
            got_m = unguard(m_b, msgs0.nbytes).view(ft8.MESSAGE_DTYPE).reshape(B, 50)
            got_r = unguard(r_b, ref0.nbytes).view(ft8.REFINED_DTYPE).reshape(B, 50)
            got_n = unguard(n_b, 4 * B).view(np.int32)
    assert (got_n == n).all() and got_m.tobytes() == msgs.tobytes()
    assert got_r.tobytes() == want.tobytes(), first_difference(got_r, want, n)
    behind = np.arange(50)[None, :] >= n[:, None]
    assert (got_r.view(np.uint8).reshape(B, 50, 48)[behind] == FILL).all() and (got_r[~behind]["valid"] == 1).all()
    # the refined values are finer than the grid's: every record moves by less than a cell
    written = got_r.copy()
    written[behind] = np.zeros(1, ft8.REFINED_DTYPE)[0]
    dt, hz, _snr, ok = ft8.refined_estimate(got_m, written)
    assert ok[~behind].all() and not ok[behind].any()
    assert (np.abs(hz - got_m["freq_hz"])[~behind] <= 3.125 * 1.5 + 1e-3).all()
    assert (np.abs(dt - got_m["dt_s"] - 0.08)[~behind] <= (512 + 16) / 3200.0 + 1e-6).all()


# ---- constructed records through the stage entry -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def constructed(oracle):
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, n, where = rc.constructed(ft8)
    fill = np.full((3, 50 * 48), FILL, np.uint8).view(ft8.REFINED_DTYPE).reshape(3, 50)
    want = sr.refine(iq, msgs, n, sr.twiddles(oracle), refined=fill)
    for a in (iq, msgs, n, fill, want):
        a.setflags(write=False)
    return iq, msgs, n, where, fill, want


@pytest.mark.parametrize("form", ["host", "device"])
def test_stage_entry_equals_the_restatement_on_constructed_records(constructed, form):
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, n, where, fill, want = constructed
    with ft8.Decoder(device=0, max_frames=2 if form == "host" else 3) as dec:
        if form == "host":
            got = dec.refine_messages(iq, msgs, n, refined=fill.copy())
        else:
            ins = [up(a) for a in (iq, msgs, n)]
            r_b = guarded(fill)
            torch.cuda.synchronize()
            dec.refine_messages_dev(ins[0], ins[1], ins[2], 3, r_b[GUARD:])
            dec.synchronize()
            for a, b in zip((iq, msgs, n), ins):
                assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()          # inputs are inputs
            got = unguard(r_b, fill.nbytes).view(ft8.REFINED_DTYPE).reshape(3, 50)
    names = {v: k for k, v in where.items()}
    for f in range(3):
        for i in range(50):
            assert got[f, i].tobytes() == want[f, i].tobytes(), (names.get((f, i)), f, i, got[f, i], want[f, i])
    assert (got[1].view(np.uint8) == FILL).all() and (got[2, 3:].view(np.uint8) == FILL).all()
    z = got[2, 0]
    assert z["e_best"] == -16 and z["valid"] == 1 and z.tobytes()[4:] == bytes(44)             # all zeros in: every power is +0
    assert got[where["truth_at_plus16"]]["e_best"] == 16 and got[where["truth_at_minus16"]]["e_best"] == -16


# ---- float edges, ties and 259 frames -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edges(oracle):
    """tests/iq_edges_craft.edges and the refine restatement on it (tests/test_iq_edges_cpu.py proves what each case is)"""
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, _refined, _first, n, where = ec.edges(ft8)
    fill = ec.filled(ft8.REFINED_DTYPE, len(n))
    with np.errstate(all="ignore"):
        want = sr.refine(iq, msgs, n, sr.twiddles(oracle), refined=fill)
    for a in (iq, msgs, n, fill, want):
        a.setflags(write=False)
    return iq, msgs, n, where, fill, want


@pytest.mark.parametrize("form", ["host", "device"])
def test_stage_entry_on_float_edges_and_ties(edges, form):
    """subnormal, vanishing and infinite powers, samples that are not finite, and thirteen equal non-zero maxima from e = 4 on:
    byte for byte, but that a NaN of the restatement is any NaN on the device (only in the cases listed in
    iq_edges_craft.NAN_OUTPUT_CASES)"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, n, where, fill, want = edges
    B = len(n)
    with ft8.Decoder(device=0, max_frames=8 if form == "host" else B) as dec:
        if form == "host":
            got = dec.refine_messages(iq, msgs, n, refined=fill.copy())
        else:
            ins = [up(a) for a in (iq, msgs, n)]
            r_b = guarded(fill)
            torch.cuda.synchronize()
            dec.refine_messages_dev(ins[0], ins[1], ins[2], B, r_b[GUARD:])
            dec.synchronize()
            for a, b in zip((iq, msgs, n), ins):
                assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()          # inputs are inputs
            got = unguard(r_b, fill.nbytes).view(ft8.REFINED_DTYPE).reshape(B, 50)
    print("NaN against NaN:", ec.hold(got, want, where))
    behind = np.arange(50)[None, :] >= n[:, None]
    assert (got.view(np.uint8).reshape(B, 50, 48)[behind] == FILL).all()
    assert got[where["refine_tie"]]["e_best"] == 4 and got[where["nan_behind_window_edge_inside"]]["e_best"] == 0
    assert got[where["scaled_subnormal_powers"]]["e_best"] == 0 and got[where["scaled_zero_powers"]]["e_best"] == -16


@pytest.mark.parametrize("form", ["host", "device"])
def test_whole_path_over_259_frames(radio, form):
    """the radio frames at 0, 130, 255, 256 and 258 of 259 frames, zeros elsewhere, in one chunk on a context of 260: a grid of
    259 x 13 workgroups; a zero frame has no records and its refined slots keep their 0xA5"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq5, msgs5, n5, want5 = radio
    B, at = ec.PIECES_FRAMES, ec.WHOLE_AT
    iq, msgs, n, want = ec.placed(iq5, at), ec.placed(msgs5, at, fill=FILL), ec.placed(n5, at), ec.placed(want5, at, fill=FILL)
    msgs0, ref0 = filled(ft8, B)
    with ft8.Decoder(device=0, max_frames=ec.PIECES_CONTEXT) as dec:
        if form == "host":
            got_m, got_n, got_r = dec.decode_messages_refined(iq, msgs=msgs0, refined=ref0)
        else:
            iq_d, m_b, r_b, n_b = up(iq), guarded(msgs0), guarded(ref0), guarded(np.zeros(B, np.int32))
            torch.cuda.synchronize()
            dec.decode_messages_refined_dev(iq_d, B, m_b[GUARD:], n_b[GUARD:], r_b[GUARD:])
            dec.synchronize()
            got_m = unguard(m_b, msgs0.nbytes).view(ft8.MESSAGE_DTYPE).reshape(B, 50)
            got_r = unguard(r_b, ref0.nbytes).view(ft8.REFINED_DTYPE).reshape(B, 50)
            got_n = unguard(n_b, 4 * B).view(np.int32)
    assert got_n.tolist() == n.tolist() and got_n[255] >= 1 and got_n[256] >= 1 and got_n.sum() == n5.sum()
    assert got_m.tobytes() == msgs.tobytes(), first_difference(got_m, msgs, n)
    assert got_r.tobytes() == want.tobytes(), first_difference(got_r, want, n)


# ---- the product path is not moved ---------------------------------------------------------------------------------------------------------

def test_product_records_are_unchanged_by_a_refine_call():
    """ft8gpu_decode_batch and ft8gpu_decode_messages on 64 frames, before and after refine calls on the same context"""
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
        torch.cuda.synchronize()
        dec.decode_batch_dev(iq, B, spots, nres)
        dec.decode_messages_dev(iq, B, msgs, nm)
        dec.synchronize()
        h = hashlib.sha256()
        for t in (spots, nres, msgs, nm):
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest(), int(nm.sum().item()), msgs, nm

    with ft8.Decoder(device=0, max_frames=B) as dec:
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, S, 1.0, workload.SEED_BASE, iq, first_frame=0)
        dec.synchronize()
        before, total, msgs, nm = digest(dec, iq)
        assert total > 5 * B
        ref = torch.zeros((B, 50 * 48), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dec.refine_messages_dev(iq, msgs, nm, B, ref)
        m2, n2 = torch.zeros_like(msgs), torch.zeros_like(nm)
        ref2 = torch.zeros_like(ref)
        dec.decode_messages_refined_dev(iq, B, m2, n2, ref2)
        dec.synchronize()
        assert torch.equal(m2, msgs) and torch.equal(n2, nm) and torch.equal(ref2, ref)
        valid = ref.cpu().numpy().view(ft8.REFINED_DTYPE).reshape(B, 50)["valid"]
        assert int(valid.sum()) == total
        after, _total, _m, _n = digest(dec, iq)
    assert before == after
