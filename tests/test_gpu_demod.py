"""GPU tests of the demodulation from the I/Q samples (ft8gpu_demod_candidates, ft8gpu_decode_messages_demod) against the numpy
restatement tests/ft8_spec_demod.py, byte for byte: radio frames near BP's threshold through the whole path on a context of
two frames (three chunks, the last ragged), host and device pointers; the hand-made candidates of tests/demod_craft.py through
the stage entry under every parameter edge; the product path's records before and after stage calls on the same context; empty
calls and refused arguments.  tests/test_demod_cpu.py proves on the CPU that the hand-made inputs are what they are named for."""
import hashlib

import numpy as np
import pytest

import demod_craft as dc
import ft8_spec_demod as sdm

pytestmark = pytest.mark.gpu
GUARD, FILL, CAP = 256, dc.FILL, dc.CAP


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


# ---- radio frames through the whole path ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def radio(oracle):
    """5 frames of 6 off-grid signals near BP's threshold (tests/demod_craft.py), what ft8gpu_decode_messages alone returns for
    them, and the restatement of the whole path on the oracle's stages"""
    import rtlsdr_ft8d_amd as ft8
    import ft8_spec_messages as sm
    iq, planted = dc.radio(ft8, oracle)
    B = len(iq)
    msgs0 = np.full((B, 50 * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(B, 50)
    with ft8.Decoder(device=0, max_frames=B, max_candidates=CAP) as dec:
        msgs1, n1 = dec.decode_messages(iq, msgs=msgs0.copy())
    stages = sm.oracle_stages(oracle, iq, CAP, 10, 4, 20)
    info = []
    want_m, want_n, want_nbs = sdm.decode_demod(oracle, iq, sdm.SETS, sdm.MAX_HARD_ERRORS, msgs=msgs0, max_candidates=CAP, stages=stages,
                                                bp=oracle.bp_decode, trace=info)
    for a in (iq, msgs0, msgs1, n1, want_m, want_n, want_nbs):
        a.setflags(write=False)
    return iq, planted, msgs0, msgs1, n1, want_m, want_n, want_nbs, info[0]


@pytest.mark.parametrize("form", ["host", "device"])
def test_whole_path_equals_decode_messages_and_the_restatement(radio, form):
    """max_frames = 2 under 5 frames: three chunks, the last of one frame; slots behind the counts keep their 0xA5"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, planted, msgs0, msgs1, n1, want_m, want_n, want_nbs, info = radio
    B = len(n1)
    failed = (info["result"] > 1).sum()
    assert (want_nbs[:, 1] - want_nbs[:, 0]).sum() >= 1 and failed >= 1, "BP fails on some, the restatement recovers at least one"
    with ft8.Decoder(device=0, max_frames=2, max_candidates=CAP) as dec:
        if form == "host":
            got_m, got_n, got_nbs = dec.decode_messages_demod(iq, msgs=msgs0.copy())
        else:
            iq_d, m_b, n_b, s_b = up(iq), guarded(msgs0), guarded(np.zeros(B, np.int32)), guarded(np.zeros((B, 2), np.int32))
            torch.cuda.synchronize()
            dec.decode_messages_demod_dev(iq_d, B, sdm.SETS, sdm.MAX_HARD_ERRORS, CAP, m_b[GUARD:], n_b[GUARD:], s_b[GUARD:])
            dec.synchronize()
            assert iq_d.cpu().numpy().tobytes() == iq.tobytes()
            got_m = unguard(m_b, msgs0.nbytes).view(ft8.MESSAGE_DTYPE).reshape(B, 50)
            got_n = unguard(n_b, 4 * B).view(np.int32)
            got_nbs = unguard(s_b, 8 * B).view(np.int32).reshape(B, 2)
    assert (got_nbs[:, 0] == n1).all()
    for f in range(B):
        assert got_m[f, :n1[f]].tobytes() == msgs1[f, :n1[f]].tobytes(), f
    assert (got_n == want_n).all() and (got_nbs == want_nbs).all(), (got_nbs, want_nbs)
    for f in range(B):
        for r in range(50):
            assert got_m[f, r].tobytes() == want_m[f, r].tobytes(), (f, r, got_m[f, r], want_m[f, r])
    behind = np.arange(50)[None, :] >= got_n[:, None]
    assert (got_m.view(np.uint8).reshape(B, 50, 64)[behind] == FILL).all()
    for f in range(B):
        gained = got_m[f, n1[f]:got_n[f]]
        assert all(1 <= int(m["pad"][3]) <= 3 for m in gained) and all(m["text"].decode() in planted[f] for m in gained)


# ---- hand-made candidates through the stage entry -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def constructed(oracle):
    import rtlsdr_ft8d_amd as ft8
    iq, cands, counts, status, where = dc.constructed(ft8, oracle)
    fill_st = np.full((4, CAP * 48), FILL, np.uint8).view(ft8.STATUS_DTYPE).reshape(4, CAP)
    fill_info = np.full((4, CAP * 16), FILL, np.uint8).view(sdm.INFO_DTYPE).reshape(4, CAP)
    for a in (iq, cands, counts, status, fill_st, fill_info):
        a.setflags(write=False)
    return dict(iq=iq, cands=cands, counts=counts, status=status, where=where, fill_st=fill_st, fill_info=fill_info, cache={})


def demod_dev(dec, d, counts, sets, gate, mpf, in_place):
    """the device form between guard bands -> (status_out bytes, info bytes); the inputs stay as they are"""
    import torch
    ins = [up(a) for a in (d["iq"], d["cands"], counts, d["status"])]
    out_b, info_b = guarded(d["status"] if in_place else d["fill_st"]), guarded(d["fill_info"])
    torch.cuda.synchronize()
    dec.demod_candidates_dev(ins[0], ins[1], ins[2], out_b[GUARD:] if in_place else ins[3], 4, sets, gate, mpf, out_b[GUARD:], info_b[GUARD:])
    dec.synchronize()
    for a, b in zip((d["iq"], d["cands"], counts) + (() if in_place else (d["status"],)), ins):
        assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()                  # inputs are inputs
    return unguard(out_b, d["fill_st"].nbytes).tobytes(), unguard(info_b, d["fill_info"].nbytes).tobytes()


# (sets, gate, max_per_frame, counts or None for the crafted ones)
CASES = [(s, 174, CAP, None) for s in range(1, 8)] + [(7, 0, CAP, None), (7, sdm.MAX_HARD_ERRORS, CAP, None), (7, 174, 0, None),
                                                       (7, 174, 1, None), (5, 174, 3, None), (7, 174, CAP, (3, 0, 3, CAP))]


@pytest.mark.parametrize("ieee", [False, True])
def test_stage_entry_equals_the_restatement_on_hand_made_candidates(constructed, oracle, ieee):
    import rtlsdr_ft8d_amd as ft8
    d = constructed
    seen = set()
    with ft8.Decoder(device=0, max_frames=4, max_candidates=CAP) as dec, ft8.Decoder(device=0, max_frames=3, max_candidates=CAP) as dec3:
        for k in (dec, dec3):
            k.set_debug_flags(ft8.DBG_FORCE_IEEE_DIV if ieee else 0)
        for sets, gate, mpf, cnt in CASES:
            counts = d["counts"] if cnt is None else np.array(cnt, np.int32)
            want_st, want_info = sdm.demod_candidates(oracle, d["iq"], d["cands"], counts, d["status"], sets, gate, mpf,
                                                      status_out=d["fill_st"], info=d["fill_info"], bp=oracle.bp_decode, cache=d["cache"])
            want_in, _ = sdm.demod_candidates(oracle, d["iq"], d["cands"], counts, d["status"], sets, gate, mpf, status_out=d["status"],
                                              info=d["fill_info"], bp=oracle.bp_decode, cache=d["cache"])
            seen |= set(int(r) for f in range(4) for r in want_info[f, :counts[f]]["result"])
            st, info = dec3.demod_candidates(d["iq"], d["cands"], counts, d["status"], sets, gate, mpf, status_out=d["fill_st"],
                                             info=d["fill_info"])                               # host form, two chunks
            for f in range(4):
                for i in range(CAP):
                    assert info[f, i].tobytes() == want_info[f, i].tobytes(), (sets, gate, mpf, f, i, info[f, i], want_info[f, i])
            assert st.tobytes() == want_st.tobytes(), (sets, gate, mpf, "host")
            assert demod_dev(dec, d, counts, sets, gate, mpf, False) == (want_st.tobytes(), want_info.tobytes()), (sets, gate, mpf, "device")
            assert demod_dev(dec, d, counts, sets, gate, mpf, True) == (want_in.tobytes(), want_info.tobytes()), (sets, gate, mpf, "in place")
            if cnt is None and mpf == CAP:
                w = d["where"]
                assert want_info[w["truth_at_e+4_d+2"]]["e_best"] == 4 and want_info[w["truth_at_e+4_d+2"]]["d_best"] == 2
                assert want_info[w["truth_at_e-4_d-2"]]["e_best"] == -4 and want_info[w["truth_at_e-4_d-2"]]["d_best"] == -2
                assert (want_info[1, :3]["result"] == 6).all() and (want_info[2, 20:]["result"] == 6).all()
                assert want_info[w["already_decoded"]].tobytes() == bytes(16) and want_info[w["bp_left_no_errors"]].tobytes() == bytes(16)
            if mpf == 1:
                assert [int((want_info[f, :counts[f]]["set"] != 0).sum()) for f in range(4)] == [1, 1, 1, 0]
    assert {0, 1, 2, 6, 7} <= seen


# ---- the product path is not moved ---------------------------------------------------------------------------------------------------------

def test_product_records_are_unchanged_by_stage_calls():
    """ft8gpu_decode_batch and ft8gpu_decode_messages on 64 frames, before and after stage calls on the same context"""
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
        m2, n2 = torch.zeros_like(msgs), torch.zeros_like(nm)
        nbs = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_messages_demod_dev(iq, B, sdm.SETS, sdm.MAX_HARD_ERRORS, 16, m2, n2, nbs)
        dec.synchronize()
        h_nbs, h_nm, h_n2 = nbs.cpu().numpy(), nm.cpu().numpy(), n2.cpu().numpy()
        assert (h_nbs[:, 0] == h_nm).all() and (h_nbs[:, 1] == h_n2).all() and (h_n2 >= h_nm).all()
        a, b = msgs.cpu().numpy().reshape(B, 50, 64), m2.cpu().numpy().reshape(B, 50, 64)
        for f in range(B):
            assert a[f, :h_nm[f]].tobytes() == b[f, :h_nm[f]].tobytes()
        after, _total, _m, _n = digest(dec, iq)
    assert before == after


# ---- empty calls and refused arguments ---------------------------------------------------------------------------------------------------------

def test_empty_calls_and_refused_arguments():
    import ctypes as C
    import rtlsdr_ft8d_amd as ft8
    iq = np.zeros((1, 2, ft8.NSAMPLES), np.float32)
    cands = np.zeros((1, CAP), ft8.CAND_DTYPE)
    counts = np.zeros(1, np.int32)
    status = np.zeros((1, CAP), ft8.STATUS_DTYPE)
    with ft8.Decoder(device=0, max_frames=2, max_candidates=CAP) as dec:
        st, info = dec.demod_candidates(iq[:0], cands[:0], counts[:0], status[:0])
        assert st.shape == (0, CAP) and info.shape == (0, CAP)
        m, n, nbs = dec.decode_messages_demod(iq[:0])
        assert m.shape == (0, 50) and n.shape == (0,)
        st, info = dec.demod_candidates(iq, cands, counts, status, status_out=np.full((1, CAP * 48), FILL, np.uint8),
                                        info=np.full((1, CAP * 16), FILL, np.uint8))
        assert (st.view(np.uint8) == FILL).all() and (info.view(np.uint8) == FILL).all()      # counts of 0: nothing is written
        for kw, word in ((dict(sets=0), "sets"), (dict(sets=8), "sets"), (dict(max_hard_errors=-1), "max_hard_errors"),
                         (dict(max_hard_errors=175), "max_hard_errors"), (dict(max_per_frame=-1), "max_per_frame"),
                         (dict(max_per_frame=CAP + 1), "max_per_frame")):
            with pytest.raises(ft8.Ft8GpuError, match=word):
                dec.demod_candidates(iq, cands, counts, status, **kw)
            with pytest.raises(ft8.Ft8GpuError, match=word):
                dec.decode_messages_demod(iq, **kw)
        L = dec.lib
        p = ft8.DemodParams(7, 36, CAP)
        assert L.ft8gpu_demod_candidates(dec.h, None, cands.ctypes.data, counts.ctypes.data, status.ctypes.data, 1, C.byref(p),
                                         status.ctypes.data, status.ctypes.data, ft8.HOST_PTRS) == -1
        assert b"NULL" in L.ft8gpu_last_error()
        assert L.ft8gpu_demod_candidates(dec.h, iq.ctypes.data, cands.ctypes.data, counts.ctypes.data, status.ctypes.data, 1, None,
                                         status.ctypes.data, status.ctypes.data, ft8.HOST_PTRS) == -1
        assert b"params" in L.ft8gpu_last_error()
        assert L.ft8gpu_demod_candidates(dec.h, iq.ctypes.data, cands.ctypes.data, counts.ctypes.data, status.ctypes.data, -1, C.byref(p),
                                         status.ctypes.data, status.ctypes.data, ft8.HOST_PTRS) == -1
        assert L.ft8gpu_decode_messages_demod(dec.h, iq.ctypes.data, 1, C.byref(p), None, counts.ctypes.data, None, ft8.HOST_PTRS) == -1
        assert L.ft8gpu_decode_messages_demod(dec.h, 8, 1, C.byref(p), 16, 16, None, ft8.DEVICE_PTRS) == -1
        assert b"aligned" in L.ft8gpu_last_error()
