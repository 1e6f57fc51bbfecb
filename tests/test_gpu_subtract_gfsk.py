"""GPU tests of the shaped subtraction entries (ft8gpu_subtract_messages_shaped, ft8gpu_decode_messages_subtracted_shaped) against
the numpy restatement tests/ft8_spec_subtract_gfsk.py, byte for byte at shape 1: the hand-made records of tests/subtract_craft.py
and two late-firsts frames of tests/iq_edges_craft.py through the stage entry in host, device and in-place form; an infinite
sample and a frame scaled by 2^-90; 258 frames on a context of 260 with records on four of them; five crowded GFSK frames through
the whole path at three passes on a context of two frames.  Shape 0 through the new entries gives the bytes of the old ones, a
shape outside {0, 1} is refused with nothing written, and the product paths' records are the same before and after shaped calls.
tests/test_subtract_gfsk_cpu.py proves the restatement on the CPU, the four tone patterns among it: a record's tones always carry
the Costas arrays (tone[0] = 3, tone[78] = 2), so on the device the end extensions e[0] and e[80] are those of every record here."""
import hashlib
import os
import sys

import numpy as np
import pytest

import ft8_spec_subtract as ss
import ft8_spec_subtract_gfsk as sg
import iq_edges_craft as ec
import subtract_craft as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu
GUARD, FILL = 256, sc.FILL
LATE_CASES = ("late_4_8", "late_49_50")


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


def equal_bits(got, want):
    got, want = np.ascontiguousarray(got).reshape(-1).view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    return got.shape == want.shape and bool((got == want).all())


def sample_difference(got, want):
    d = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return None if len(d) == 0 else f"{len(d)} samples differ, the first at {d[0].tolist()}: {got[tuple(d[0])]!r} != {want[tuple(d[0])]!r}"


def info_difference(got, want):
    for f in range(got.shape[0]):
        for i in range(50):
            if got[f, i].tobytes() != want[f, i].tobytes():
                return f"frame {f} slot {i}: {got[f, i]} != {want[f, i]}"
    return None


def stage(dec, form, iq, msgs, refined, first, n, fill, shape):
    """ft8gpu_subtract_messages_shaped in one of three forms -> (iq_out, info); the device forms between guard bands"""
    import torch
    B = len(n)
    if form == "host":
        return dec.subtract_messages(iq, msgs, refined, first, n, info=fill.copy(), shape=shape)
    ins = [up(a) for a in (msgs, refined, first, n)]
    x_b, i_b = guarded(iq), guarded(fill)
    o_b = x_b if form == "device_in_place" else guarded(np.zeros_like(iq))
    torch.cuda.synchronize()
    dec.subtract_messages_dev(x_b[GUARD:], ins[0], ins[1], ins[2], ins[3], B, o_b[GUARD:], i_b[GUARD:], shape=shape)
    dec.synchronize()
    for a, b in zip((msgs, refined, first, n), ins):
        assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()              # inputs are inputs
    if form == "device":
        assert unguard(x_b, iq.nbytes).tobytes() == iq.tobytes()
    return (unguard(o_b, iq.nbytes).view(np.float32).reshape(iq.shape), unguard(i_b, fill.nbytes).view(ss.INFO_DTYPE).reshape(B, 50))


# ---- (i) the stage entry ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def records():
    """8 frames: the six of subtract_craft.constructed (frame 0: 50 records, windows that start before sample 0 and end past
    47999, R.valid = 0, random a91; counts of 0, 3 and 50; first > 0; three overlapping records) and the late firsts (4, 8) and
    (49, 50); and the restatement at shape 1 on them"""
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, refined, first, n, where = sc.constructed(ft8)
    l_iq, l_m, l_R, l_first, l_n, names = ec.late_firsts(ft8)
    k = [names.index(c) for c in LATE_CASES]
    assert (l_first[k].tolist(), l_n[k].tolist()) == ([4, 49], [8, 50])
    iq, msgs, refined = np.concatenate([iq, l_iq[k]]), np.concatenate([msgs, l_m[k]]), np.concatenate([refined, l_R[k]])
    first, n = np.concatenate([first, l_first[k]]).astype(np.int32), np.concatenate([n, l_n[k]]).astype(np.int32)
    fill = ec.filled(ss.INFO_DTYPE, 8)
    out, info = sg.subtract(iq, msgs, refined, first, n, ss.twiddles(), sg.GFSK, info=fill)
    before = [int(info[f, i]["s_best"]) for f in range(8) for i in range(50) if first[f] <= i < n[f] and info[f, i]["valid"] == 1]
    assert min(before) < 0 and max(before) + ss.SPAN > ss.NSAMPLES       # a record cut at either end of the frame, ramp and Q with it
    for a in (iq, msgs, refined, first, n, fill, out, info):
        a.setflags(write=False)
    return iq, msgs, refined, first, n, where, fill, out, info


@pytest.mark.parametrize("form", ["host", "device", "device_in_place"])
def test_stage_entry_at_shape_1_equals_the_restatement(records, form):
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, refined, first, n, where, fill, want_out, want_info = records
    B = 8
    with ft8.Decoder(device=0, max_frames=3 if form == "host" else B) as dec:
        got_out, got_info = stage(dec, form, iq, msgs, refined, first, n, fill, ft8.SUBTRACT_GFSK)
        if form == "host":
            no_info, none = dec.subtract_messages(iq, msgs, refined, first, n, want_info=False, shape=ft8.SUBTRACT_GFSK)
            assert none is None and no_info.tobytes() == got_out.tobytes()
    assert got_info.tobytes() == want_info.tobytes(), info_difference(got_info, want_info)
    assert got_out.tobytes() == want_out.tobytes(), sample_difference(got_out, want_out)
    for f in (1, 2, 4):                                                   # counts of 0, a frame of zeros, first >= n_msgs: bit for bit
        assert got_out[f].tobytes() == iq[f].tobytes()
    raw = got_info.view(np.uint8).reshape(B, 50, 64)                     # 0xA5 kept outside [first, n_msgs)
    assert (raw[1] == FILL).all() and (raw[2, 3:] == FILL).all() and (raw[3, :2] == FILL).all() and (raw[4] == FILL).all()
    assert (raw[6, :4] == FILL).all() and (raw[6, 8:] == FILL).all() and (raw[7, :49] == FILL).all()
    assert got_info[where["not_valid"]].tobytes() == bytes(64)
    assert got_info[6, 7]["valid"] == 1 and got_info[7, 49]["valid"] == 1 and not equal_bits(got_out[6], iq[6]) and not equal_bits(got_out[7], iq[7])


@pytest.mark.parametrize("form", ["host", "device"])
def test_shape_0_through_the_shaped_stage_entry_is_the_existing_entry(records, form):
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, refined, first, n, _where, fill, want_out, _want_info = records
    with ft8.Decoder(device=0, max_frames=8) as dec:
        new_out, new_info = stage(dec, form, iq, msgs, refined, first, n, fill, ft8.SUBTRACT_CPFSK)
        old_out, old_info = stage(dec, form, iq, msgs, refined, first, n, fill, None)
        torch.cuda.synchronize()
    assert new_out.tobytes() == old_out.tobytes() and new_info.tobytes() == old_info.tobytes()
    assert new_out.tobytes() != want_out.tobytes()                        # and shape 1 is another rule


# ---- (ii) float edges ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["host", "device"])
def test_float_edges_at_shape_1(form):
    """one +inf sample inside a record: the NaNs are the restatement's, sample for sample, and everything else its bytes; a frame
    scaled by 2^-90: every power is +0 (d* = t* = -2), the amplitudes are not, and the record is still subtracted"""
    import rtlsdr_ft8d_amd as ft8
    e_iq, e_m, e_R, e_first, e_n, where = ec.edges(ft8)
    pick = [where["inf_sample"][0], where["scaled_zero_powers"][0]]
    assert ec.SCALED_EXP["scaled_zero_powers"] == -90 and e_n[pick].tolist() == [1, 1]
    iq, msgs, refined, first, n = e_iq[pick], e_m[pick], e_R[pick], e_first[pick], e_n[pick]
    with np.errstate(all="ignore"):
        want_out, want_info = sg.subtract(iq, msgs, refined, first, n, ss.twiddles(), sg.GFSK, info=ec.filled(ss.INFO_DTYPE, 2))
    with ft8.Decoder(device=0, max_frames=2) as dec:
        got_out, got_info = stage(dec, form, iq, msgs, refined, first, n, ec.filled(ss.INFO_DTYPE, 2), ft8.SUBTRACT_GFSK)
    nan_want, nan_got = np.isnan(want_out), np.isnan(got_out)
    print("NaN samples:", int(nan_want[0].sum()), "restated,", int(nan_got[0].sum()), "on the device")
    assert nan_want[0].sum() > 0 and not nan_want[1].any() and (nan_got == nan_want).all()
    assert (got_out.view(np.uint32)[~nan_want] == want_out.view(np.uint32)[~nan_want]).all()
    for k in ("k4", "s_best", "d_best", "t_best", "valid"):
        assert (got_info[k] == want_info[k]).all(), k
    pf_nan = np.isnan(want_info["pf"]) | np.isnan(want_info["pt"])
    assert ((np.isnan(got_info["pf"]) | np.isnan(got_info["pt"])) == pf_nan).all()
    for k in ("pf", "pt"):
        keep = ~np.isnan(want_info[k])
        assert (got_info[k].view(np.uint32)[keep] == want_info[k].view(np.uint32)[keep]).all(), k
    assert got_info[1].tobytes() == want_info[1].tobytes()
    r = got_info[1, 0]
    assert r["valid"] == 1 and (r["d_best"], r["t_best"]) == (-2, -2) and r["pf"].tobytes() == bytes(20) and r["pt"].tobytes() == bytes(20)
    assert not equal_bits(got_out[1], iq[1])                             # powers of +0 under amplitudes that are not


# ---- (iii) the 256-frame pieces ------------------------------------------------------------------------------------------------------------

PIECES_AT, PIECES_PICK = (0, 255, 256, 257), (3, 0, 6, 5)               # frame 255 holds the 50 records, 256 the late firsts (4, 8)


@pytest.mark.parametrize("form", ["host", "device"])
def test_stage_entry_at_shape_1_in_pieces_of_256_frames(records, form):
    """258 frames on a context of 260: subtract_chunk's pieces of 256 and 2, records on frames 0, 255, 256 and 257 only (their
    restatement is the stage fixture's: frames are independent); every other frame is noise with no records and comes back bit
    for bit"""
    import rtlsdr_ft8d_amd as ft8
    iq8, msgs8, refined8, first8, n8, _where, _fill, out8, info8 = records
    B, pick = 258, list(PIECES_PICK)
    noise = np.random.default_rng(77).normal(0.0, 0.1, (2, ss.NSAMPLES)).astype(np.float32)
    iq = np.stack([np.roll(noise, f, axis=1) for f in range(B)])
    msgs, refined = ec.placed(msgs8[pick], PIECES_AT, B, fill=FILL), ec.placed(refined8[pick], PIECES_AT, B, fill=FILL)
    first, n = ec.placed(first8[pick], PIECES_AT, B), ec.placed(n8[pick], PIECES_AT, B)
    want_out, want_info = iq.copy(), ec.placed(info8[pick], PIECES_AT, B, fill=FILL)
    for at, k in zip(PIECES_AT, pick):
        iq[at], want_out[at] = iq8[k], out8[k]
    assert n[255] == 70 and (first[256], n[256]) == (4, 8) and int(np.abs(n).sum()) == 70 + 5 + 8 + 3
    with ft8.Decoder(device=0, max_frames=260) as dec:
        got_out, got_info = stage(dec, form, iq, msgs, refined, first, n, ec.filled(ss.INFO_DTYPE, B), ft8.SUBTRACT_GFSK)
    for f in PIECES_AT:
        assert got_info[f].tobytes() == want_info[f].tobytes(), (f, info_difference(got_info[f:f + 1], want_info[f:f + 1]))
        assert got_out[f].tobytes() == want_out[f].tobytes(), (f, sample_difference(got_out[f], want_out[f]))
    assert equal_bits(got_info, want_info) and equal_bits(got_out, want_out)
    assert not equal_bits(got_out[255], iq[255]) and not equal_bits(got_out[256], iq[256])      # both pieces carried work


# ---- (iv) the whole path ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def radio(oracle):
    """5 frames of 6 off-grid GFSK signals within 100 Hz of each other from the restated synthesiser (tests/ft8_spec_gfsk.py
    through tools/gfsk_effect.waveform), and the restatement at 3 passes and shape 1"""
    import rtlsdr_ft8d_amd as ft8
    import synth_util as su
    from gfsk_effect import waveform
    enc = su.oracle_encode_fn(oracle)
    with waveform("gfsk"):
        iq = np.stack([su.make_frame(410000 + k, 6, enc, snr_range=(-16.0, 6.0), f_range=(900.0, 1000.0))[0] for k in range(5)])
    msgs, n, nbp, res = sg.decode_passes_subtracted(oracle, iq, 3, sg.GFSK, msgs=filled_msgs(ft8, 5))
    print("n_by_pass:", nbp.tolist())
    assert (nbp[:, 1] > nbp[:, 0]).sum() >= 2 and (nbp[:, 2] > nbp[:, 1]).sum() >= 1          # later passes carry work
    for a in (iq, msgs, n, nbp, res):
        a.setflags(write=False)
    return iq, msgs, n, nbp, res


@pytest.mark.parametrize("form", ["host", "device"])
def test_whole_path_at_shape_1_equals_the_restatement(radio, form):
    """max_frames = 2 under 5 frames: three chunks, the last of one frame; with and without the residual; slots behind the counts
    keep their 0xA5"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, n, nbp, res = radio
    B, G = len(n), ft8.SUBTRACT_GFSK
    with ft8.Decoder(device=0, max_frames=2) as dec:
        if form == "host":
            got_m, got_n, got_nbp, got_res = dec.decode_messages_subtracted(iq, passes=3, msgs=filled_msgs(ft8, B), shape=G)
            m2, n2, nbp2, none = dec.decode_messages_subtracted(iq, passes=3, msgs=filled_msgs(ft8, B), want_residual=False, shape=G)
            assert none is None
            old = dec.decode_messages_subtracted(iq, passes=3, msgs=filled_msgs(ft8, B))
            new0 = dec.decode_messages_subtracted(iq, passes=3, msgs=filled_msgs(ft8, B), shape=ft8.SUBTRACT_CPFSK)
        else:
            iq_d = up(iq)

            def run(shape, with_residual=True):
                m_b, n_b, nbp_b = guarded(filled_msgs(ft8, B)), guarded(np.zeros(B, np.int32)), guarded(np.zeros((B, 3), np.int32))
                r_b = guarded(np.zeros_like(iq)) if with_residual else None
                torch.cuda.synchronize()
                dec.decode_messages_subtracted_dev(iq_d, B, 3, m_b[GUARD:], n_b[GUARD:], nbp_b[GUARD:], r_b[GUARD:] if with_residual else None,
                                                   shape=shape)
                dec.synchronize()
                return (unguard(m_b, B * 50 * 64).view(ft8.MESSAGE_DTYPE).reshape(B, 50), unguard(n_b, 4 * B).view(np.int32),
                        unguard(nbp_b, 12 * B).view(np.int32).reshape(B, 3),
                        unguard(r_b, iq.nbytes).view(np.float32).reshape(iq.shape) if with_residual else None)
            got_m, got_n, got_nbp, got_res = run(G)
            m2, n2, nbp2, _none = run(G, with_residual=False)
            old, new0 = run(None), run(ft8.SUBTRACT_CPFSK)
            assert equal_bits(iq_d.cpu().numpy(), iq)                     # the caller's frames are never written
    assert got_n.tolist() == n.tolist() and got_nbp.tolist() == nbp.tolist()
    assert equal_bits(got_m, msgs) and equal_bits(got_res, res), sample_difference(got_res, res)
    assert equal_bits(m2, msgs) and n2.tolist() == n.tolist() and nbp2.tolist() == nbp.tolist()
    behind = np.arange(50)[None, :] >= n[:, None]
    assert (got_m.view(np.uint8).reshape(B, 50, 64)[behind] == FILL).all()
    for a, b in zip(old, new0):                                           # shape 0 gives the bytes of the existing entry
        assert equal_bits(a, b)
    assert not equal_bits(old[3], got_res)                                # ... which are not those of shape 1


# ---- (v) a shape that is none -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [2, -1])
def test_a_shape_outside_0_and_1_is_refused_and_nothing_is_written(records, shape):
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, msgs, refined, first, n = (a[3:5] for a in records[:5])
    with ft8.Decoder(device=0, max_frames=2) as dec:
        ins = [up(a) for a in (iq, msgs, refined, first, n)]
        o_b, i_b = guarded(np.full_like(iq.view(np.uint8), FILL)), guarded(ec.filled(ss.INFO_DTYPE, 2))
        m_b, n_b, nbp_b = guarded(filled_msgs(ft8, 2)), guarded(np.full(8, FILL, np.uint8)), guarded(np.full(24, FILL, np.uint8))
        torch.cuda.synchronize()
        with pytest.raises(ft8.Ft8GpuError, match="shape"):
            dec.subtract_messages_dev(ins[0], ins[1], ins[2], ins[3], ins[4], 2, o_b[GUARD:], i_b[GUARD:], shape=shape)
        with pytest.raises(ft8.Ft8GpuError, match="shape"):
            dec.decode_messages_subtracted_dev(ins[0], 2, 3, m_b[GUARD:], n_b[GUARD:], nbp_b[GUARD:], o_b[GUARD:], shape=shape)
        with pytest.raises(ft8.Ft8GpuError, match="shape"):
            dec.subtract_messages(iq, msgs, refined, first, n, shape=shape)
        with pytest.raises(ft8.Ft8GpuError, match="shape"):
            dec.decode_messages_subtracted(iq, passes=3, shape=shape)
        dec.synchronize()
        for b, nbytes in ((o_b, iq.nbytes), (i_b, 2 * 50 * 64), (m_b, 2 * 50 * 64), (n_b, 8), (nbp_b, 24)):
            assert (unguard(b, nbytes) == FILL).all()
        # the context is as good as before
        out, _info = dec.subtract_messages(iq, msgs, refined, first, n, shape=ft8.SUBTRACT_GFSK)
    assert out.tobytes() == records[7][3:5].tobytes()


# ---- (vi) the product paths are not moved ----------------------------------------------------------------------------------------------------------

def test_product_records_are_unchanged_by_shaped_calls():
    """ft8gpu_decode_batch, ft8gpu_decode_messages and ft8gpu_decode_messages_subtracted on 64 frames, before and after shaped
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
        sm_ = torch.zeros((B, 50 * 64), dtype=torch.uint8, device="cuda")
        sn = torch.zeros((B,), dtype=torch.int32, device="cuda")
        sbp = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
        res = torch.zeros_like(iq)
        torch.cuda.synchronize()
        dec.decode_batch_dev(iq, B, spots, nres)
        dec.decode_messages_dev(iq, B, msgs, nm)
        dec.decode_messages_subtracted_dev(iq, B, 3, sm_, sn, sbp, res)
        dec.synchronize()
        h = hashlib.sha256()
        for t in (spots, nres, msgs, nm, sm_, sn, sbp, res):
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest(), msgs, nm, int(sn.sum().item())

    with ft8.Decoder(device=0, max_frames=B) as dec:
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, S, 1.0, workload.SEED_BASE, iq, first_frame=0)
        dec.synchronize()
        keep = iq.clone()
        before, msgs, nm, cpfsk_total = digest(dec, iq)
        gm, gn = torch.zeros_like(msgs), torch.zeros_like(nm)
        gbp = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
        res = torch.zeros_like(iq)
        ref = torch.zeros((B, 50 * 48), dtype=torch.uint8, device="cuda")
        zero = torch.zeros((B,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_messages_subtracted_dev(iq, B, 3, gm, gn, gbp, res, shape=ft8.SUBTRACT_GFSK)
        dec.refine_messages_dev(iq, msgs, nm, B, ref)
        dec.subtract_messages_dev(iq, msgs, ref, zero, nm, B, res, shape=ft8.SUBTRACT_GFSK)
        dec.subtract_messages_dev(iq, msgs, ref, zero, nm, B, res, shape=ft8.SUBTRACT_CPFSK)
        dec.synchronize()
        assert torch.equal(iq, keep)
        assert (gbp[:, 0].cpu().numpy() == nm.cpu().numpy()).all() and int(gn.sum().item()) > int(nm.sum().item())
        print("records after 3 passes on CPFSK frames: CPFSK reference", cpfsk_total, "GFSK reference", int(gn.sum().item()),
              "first pass", int(nm.sum().item()))
        after, _m, _n, _t = digest(dec, iq)
    assert before == after
