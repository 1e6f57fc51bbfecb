"""GPU tests of the subtraction in the I/Q samples (ft8gpu_subtract_messages, ft8gpu_decode_messages_subtracted) against the numpy
restatement tests/ft8_spec_subtract.py, byte for byte: crowded frames through the whole path at three passes on a context of two
frames (three chunks, the last ragged), host and device pointers; the committed uncovering seeds; the hand-made records of
tests/subtract_craft.py through the stage entry (windows that leave the frame, every choice of the fine search, R.valid = 0,
counts of 0, 3 and 50, first > 0, overlapping records, a frame of zeros, in place); the product paths' records before and
after subtraction calls on the same context; and the constructions of tests/iq_edges_craft.py: float edges, samples that are not
finite, non-zero ties and every order of R.pf[1 .. 3] with hand-made R and with the refine kernel's own, first >= 4 with records
behind it, and 259 frames on a context of 260 through the stage entry and the whole path (subtract_chunk's pieces of 256 and 3).
tests/test_subtract_cpu.py and tests/test_iq_edges_cpu.py prove on the CPU that the hand-made records are what they are named
for."""
import hashlib

import numpy as np
import pytest

import ft8_spec_subtract as ss
import iq_edges_craft as ec
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


# ---- (v) float edges, ties and u* -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edges(oracle):
    """tests/iq_edges_craft.edges and the restatements on it (tests/test_iq_edges_cpu.py proves what each case is)"""
    import rtlsdr_ft8d_amd as ft8
    batch = ec.edges(ft8)
    want = ec.edges_expected(oracle, batch)
    for a in batch[:5] + tuple(want.values()):
        a.setflags(write=False)
    return batch, want


def subtract_stage(dec, form, iq, msgs, refined, first, n, fill):
    """ft8gpu_subtract_messages in one of three forms -> (iq_out, info); the device forms between guard bands"""
    import torch
    B = len(n)
    if form == "host":
        return dec.subtract_messages(iq, msgs, refined, first, n, info=fill.copy())
    ins = [up(a) for a in (msgs, refined, first, n)]
    x_b, i_b = guarded(iq), guarded(fill)
    o_b = x_b if form == "device_in_place" else guarded(np.zeros_like(iq))
    torch.cuda.synchronize()
    dec.subtract_messages_dev(x_b[GUARD:], ins[0], ins[1], ins[2], ins[3], B, o_b[GUARD:], i_b[GUARD:])
    dec.synchronize()
    for a, b in zip((msgs, refined, first, n), ins):
        assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()              # inputs are inputs
    if form == "device":
        assert unguard(x_b, iq.nbytes).tobytes() == iq.tobytes()
    return (unguard(o_b, iq.nbytes).view(np.float32).reshape(iq.shape), unguard(i_b, fill.nbytes).view(ss.INFO_DTYPE).reshape(B, 50))


@pytest.mark.parametrize("form", ["host", "device", "device_in_place"])
def test_stage_entry_on_float_edges_ties_and_ustar(edges, form):
    """subnormal, vanishing and infinite powers, samples that are not finite, non-zero ties and every order of R.pf[1 .. 3], with
    the hand-made R: byte for byte, but that a NaN of the restatement is any NaN on the device (only in the cases listed in
    iq_edges_craft.NAN_OUTPUT_CASES)"""
    import rtlsdr_ft8d_amd as ft8
    (iq, msgs, refined, first, n, where), want = edges
    B = len(n)
    with ft8.Decoder(device=0, max_frames=8 if form == "host" else B) as dec:
        got_out, got_info = subtract_stage(dec, form, iq, msgs, refined, first, n, ec.filled(ss.INFO_DTYPE, B))
    in_info, in_out = ec.hold(got_info, want["info"], where), ec.hold(got_out, want["out"], where)
    print("NaN against NaN, hand-made R:", {k: (in_info[k], in_out[k]) for k in in_info})
    for name, (_pf, us) in ec.USTAR.items():
        r = got_info[where[name]]
        assert int(r["k4"]) - int(r["d_best"]) == 4 * (ec.F_SIG + us - 2), name
    behind = np.arange(50)[None, :] >= n[:, None]
    assert (got_info.view(np.uint8).reshape(B, 50, 64)[behind] == FILL).all()


@pytest.mark.parametrize("form", ["host", "device"])
def test_refine_then_subtract_on_float_edges_ties_and_ustar(edges, form):
    """the same frames with R from the refine kernel itself, as the pass loop pairs the two stages"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    (iq, msgs, _hand_made, first, n, where), want = edges
    B = len(n)
    with ft8.Decoder(device=0, max_frames=8 if form == "host" else B) as dec:
        if form == "host":
            got_ref = dec.refine_messages(iq, msgs, n, refined=ec.filled(ft8.REFINED_DTYPE, B))
            got_out, got_info = dec.subtract_messages(iq, msgs, got_ref, first, n, info=ec.filled(ss.INFO_DTYPE, B))
        else:
            ins = [up(a) for a in (iq, msgs, first, n)]
            r_b, o_b, i_b = guarded(ec.filled(ft8.REFINED_DTYPE, B)), guarded(np.zeros_like(iq)), guarded(ec.filled(ss.INFO_DTYPE, B))
            torch.cuda.synchronize()
            dec.refine_messages_dev(ins[0], ins[1], ins[3], B, r_b[GUARD:])
            dec.subtract_messages_dev(ins[0], ins[1], r_b[GUARD:], ins[2], ins[3], B, o_b[GUARD:], i_b[GUARD:])
            dec.synchronize()
            got_ref = unguard(r_b, B * 50 * 48).view(ft8.REFINED_DTYPE).reshape(B, 50)
            got_out = unguard(o_b, iq.nbytes).view(np.float32).reshape(iq.shape)
            got_info = unguard(i_b, B * 50 * 64).view(ss.INFO_DTYPE).reshape(B, 50)
    in_ref, in_info, in_out = ec.hold(got_ref, want["refined"], where), ec.hold(got_info, want["pair_info"], where), ec.hold(got_out, want["pair_out"], where)
    print("NaN against NaN, the refine kernel's R:", {k: (in_ref[k], in_info[k], in_out[k]) for k in in_ref})


# ---- (vi) late firsts ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def late():
    import rtlsdr_ft8d_amd as ft8
    batch = ec.late_firsts(ft8)
    out, info = ec.late_expected(batch)
    for a in batch[:5] + (out, info):
        a.setflags(write=False)
    return batch, out, info


@pytest.mark.parametrize("form", ["host", "device"])
def test_stage_entry_on_late_firsts(late, form):
    """first >= 4 with records behind it: estimate workgroups skipped whole and in part, the apply kernel's headers read from
    record `first` on, a skipped record as the first header; info outside [first, n_msgs) keeps the caller's 0xA5"""
    import rtlsdr_ft8d_amd as ft8
    (iq, msgs, refined, first, n, names), want_out, want_info = late
    B = len(n)
    with ft8.Decoder(device=0, max_frames=3 if form == "host" else B) as dec:
        got_out, got_info = subtract_stage(dec, form, iq, msgs, refined, first, n, ec.filled(ss.INFO_DTYPE, B))
    raw = got_info.view(np.uint8).reshape(B, 50, 64)
    for f, name in enumerate(names):
        for i in range(50):
            assert got_info[f, i].tobytes() == want_info[f, i].tobytes(), (name, i, got_info[f, i], want_info[f, i])
        assert got_out[f].tobytes() == want_out[f].tobytes(), (name, sample_difference(got_out[f], want_out[f]))
        assert (raw[f, :first[f]] == FILL).all() and (raw[f, n[f]:] == FILL).all(), name
        if n[f] > first[f]:
            assert got_info[f, n[f] - 1]["valid"] == 1 and got_out[f].tobytes() != iq[f].tobytes(), name
        else:
            assert got_out[f].tobytes() == iq[f].tobytes(), name
    assert got_info[names.index("late_48_50_invalid_48"), 48].tobytes() == bytes(64)


# ---- (vii) the 256-frame pieces ------------------------------------------------------------------------------------------------------------------

def equal_bits(got, want):
    got, want = np.ascontiguousarray(got).reshape(-1).view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    return got.shape == want.shape and bool((got == want).all())


@pytest.fixture(scope="module")
def pieces(constructed, late):
    """259 frames: zeros with n_msgs = 0, but the six frames of `constructed` and the late-firsts frame (5, 11) at
    iq_edges_craft.STAGE_AT; the expected outputs are those fixtures' own, placed (frames are independent)"""
    import rtlsdr_ft8d_amd as ft8
    _iq, _msgs, _refined, _first, _n, _where, _fill, c_out, c_info = constructed
    (_l_iq, _l_m, _l_R, _l_first, _l_n, l_names), l_out, l_info = late
    k = l_names.index("late_5_11")
    pick = lambda a, l: np.stack([l[k] if s == "late" else a[s] for s in ec.STAGE_ORDER])
    iq, msgs, refined, first, n = ec.pieces_stage(ft8)
    assert iq[4].tobytes() == _l_iq[k].tobytes() and iq[3].tobytes() == _iq[0].tobytes() and first.tolist() == [2, 0, 0, -3, 5, 7, 0]
    at = ec.STAGE_AT
    full = (ec.placed(iq, at), ec.placed(msgs, at, fill=FILL), ec.placed(refined, at, fill=FILL), ec.placed(first, at), ec.placed(n, at))
    want_out, want_info = ec.placed(pick(c_out, l_out), at), ec.placed(pick(c_info, l_info), at, fill=FILL)
    for a in full + (want_out, want_info):
        a.setflags(write=False)
    return full, want_out, want_info


@pytest.mark.parametrize("form", ["host", "device"])
def test_stage_entry_in_pieces_of_256_frames(pieces, form):
    """one chunk of 259 frames on a context of 260: subtract_chunk's pieces of 256 and 3, with records in frames 255 and 256"""
    import rtlsdr_ft8d_amd as ft8
    (iq, msgs, refined, first, n), want_out, want_info = pieces
    B = ec.PIECES_FRAMES
    assert B == len(n) == 259 and n[255] == 70 and (first[256], n[256]) == (5, 11)
    with ft8.Decoder(device=0, max_frames=ec.PIECES_CONTEXT) as dec:
        got_out, got_info = subtract_stage(dec, form, iq, msgs, refined, first, n, ec.filled(ss.INFO_DTYPE, B))
        if form == "host":
            no_info, none = dec.subtract_messages(iq, msgs, refined, first, n, want_info=False)
            assert none is None and equal_bits(no_info, want_out)
    for f in ec.STAGE_AT:
        assert got_info[f].tobytes() == want_info[f].tobytes(), (f, first_difference(got_info[f:f + 1], want_info[f:f + 1], n[f:f + 1]))
        assert got_out[f].tobytes() == want_out[f].tobytes(), (f, sample_difference(got_out[f], want_out[f]))
    assert equal_bits(got_info, want_info) and equal_bits(got_out, want_out)
    assert not equal_bits(got_out[255], iq[255]) and not equal_bits(got_out[256], iq[256])      # both pieces carried work


def place_whole(radio, B, at):
    iq, msgs, n, nbp, res = radio
    return (ec.placed(iq, at, B), ec.placed(msgs, at, B, fill=FILL), ec.placed(n, at, B), ec.placed(nbp, at, B), ec.placed(res, at, B))


@pytest.mark.parametrize("form", ["host", "device"])
def test_whole_path_in_pieces_of_256_frames(radio, form):
    """the radio frames at 0, 130, 255, 256 and 258 of 259 frames, zeros elsewhere, at three passes on a context of 260: the pass
    loop's subtract_chunk in pieces of 256 and 3; with and without the residual"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    B = ec.PIECES_FRAMES
    iq, msgs, n, nbp, res = place_whole(radio, B, ec.WHOLE_AT)
    assert nbp[255].tolist() == [1, 3, 4] and nbp[256].tolist() == [2, 3, 4]                    # both pieces subtract in both later passes
    with ft8.Decoder(device=0, max_frames=ec.PIECES_CONTEXT) as dec:
        if form == "host":
            got_m, got_n, got_nbp, got_res = dec.decode_messages_subtracted(iq, passes=3, msgs=filled_msgs(ft8, B))
            m2, n2, nbp2, none = dec.decode_messages_subtracted(iq, passes=3, msgs=filled_msgs(ft8, B), want_residual=False)
            assert none is None
        else:
            iq_d = up(iq)
            def run(with_residual):
                m_b, n_b, nbp_b = guarded(filled_msgs(ft8, B)), guarded(np.zeros(B, np.int32)), guarded(np.zeros((B, 3), np.int32))
                r_b = guarded(np.zeros_like(iq)) if with_residual else None
                torch.cuda.synchronize()
                dec.decode_messages_subtracted_dev(iq_d, B, 3, m_b[GUARD:], n_b[GUARD:], nbp_b[GUARD:], r_b[GUARD:] if with_residual else None)
                dec.synchronize()
                return (unguard(m_b, B * 50 * 64).view(ft8.MESSAGE_DTYPE).reshape(B, 50), unguard(n_b, 4 * B).view(np.int32),
                        unguard(nbp_b, 12 * B).view(np.int32).reshape(B, 3),
                        unguard(r_b, iq.nbytes).view(np.float32).reshape(iq.shape) if with_residual else None)
            got_m, got_n, got_nbp, got_res = run(True)
            m2, n2, nbp2, _none = run(False)
            assert equal_bits(iq_d.cpu().numpy(), iq)
    assert got_n.tolist() == n.tolist() and got_nbp.tolist() == nbp.tolist()
    assert equal_bits(got_m, msgs), first_difference(got_m, msgs, n)
    for f in ec.WHOLE_AT:
        assert got_res[f].tobytes() == res[f].tobytes(), (f, sample_difference(got_res[f], res[f]))
    assert equal_bits(got_res, res)                                       # a zero frame: no records, itself as residual
    assert equal_bits(m2, msgs) and n2.tolist() == n.tolist() and nbp2.tolist() == nbp.tolist()
    assert not equal_bits(got_res[255], iq[255]) and not equal_bits(got_res[256], iq[256])
