"""GPU tests of the demodulation from the I/Q samples (ft8gpu_demod_candidates, ft8gpu_decode_messages_demod) against the numpy
restatement tests/ft8_spec_demod.py, byte for byte: radio frames near BP's threshold through the whole path on a context of
two frames (three chunks, the last ragged), host and device pointers; the hand-made candidates of tests/demod_craft.py through
the stage entry under every parameter edge; the constructed signals of tests/demod_edges_craft.py (results 3 and 4, acceptance by
set 2 and set 3 with the gate at and below their nhard, soft bits below the division guard's bound, subnormal, infinite and NaN
powers, extreme records, the frame's edges), lists of 70 and 7 candidates, ldpc_iters of 1, 5 and 50; the product path's records
before and after stage calls on the same context; empty calls and refused arguments.  tests/test_demod_cpu.py proves on the CPU
that the hand-made inputs are what they are named for."""
import hashlib

import numpy as np
import pytest

import demod_craft as dc
import demod_edges_craft as de
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

STAGE = {}                                    # the radio fixture's candidate counts and the stage's status records (restatement)


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
    info, cache = [], {}
    want_m, want_n, want_nbs = sdm.decode_demod(oracle, iq, sdm.SETS, sdm.MAX_HARD_ERRORS, msgs=msgs0, max_candidates=CAP, stages=stages,
                                                bp=oracle.bp_decode, trace=info, cache=cache)
    _mag, cands, counts, status = stages
    st2, _info = sdm.demod_candidates(oracle, iq, cands, counts, status, sdm.SETS, sdm.MAX_HARD_ERRORS, bp=oracle.bp_decode, cache=cache)
    STAGE["counts"], STAGE["status"] = counts, st2.view(ft8.STATUS_DTYPE).reshape(B, CAP)
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


def test_whole_path_does_not_append_what_bp_already_has(radio):
    """the five frames show candidates the stage accepts whose message BP had decoded at another candidate (27 of the 39
    accepted): none of them is appended; a gained record carries its own candidate's accepted set in pad[3]"""
    import rtlsdr_ft8d_amd as ft8
    iq, _planted, msgs0, _msgs1, n1, want_m, want_n, _want_nbs, info = radio
    B = len(n1)
    with ft8.Decoder(device=0, max_frames=B, max_candidates=CAP) as dec:
        got_m, got_n, got_nbs = dec.decode_messages_demod(iq, msgs=msgs0.copy())
    assert (got_n == want_n).all() and (got_nbs[:, 0] == n1).all() and got_m.tobytes() == want_m.tobytes()
    known = 0
    for f in range(B):
        bp_texts = [bytes(m["text"]) for m in got_m[f, :n1[f]]]
        gained = got_m[f, n1[f]:got_n[f]]
        for m in gained:
            r = info[f, int(m["cand_index"])]
            assert r["result"] == 1 and int(m["pad"][3]) == int(r["set"]) and bytes(m["text"]) not in bp_texts, (f, m)
            assert bytes(m["text"]) == bytes(STAGE["status"][f, int(m["cand_index"])]["text"])
        for i in range(int(STAGE["counts"][f])):
            if info[f, i]["result"] == 1 and bytes(STAGE["status"][f, i]["text"]) in bp_texts:
                known += 1
                assert i not in [int(m["cand_index"]) for m in gained], (f, i)
    assert known >= 1, "no accepted candidate repeats a BP record: choose another seed for the fixture"


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
    dec.demod_candidates_dev(ins[0], ins[1], ins[2], out_b[GUARD:] if in_place else ins[3], len(d["iq"]), sets, gate, mpf, out_b[GUARD:],
                             info_b[GUARD:])
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


# ---- constructed signals for every branch and edge -----------------------------------------------------------------------------------------

def as_inputs(ft8, iq, cands, counts, status, where=None):
    B, cap = cands.shape
    fill_st = np.full((B, cap * 48), FILL, np.uint8).view(ft8.STATUS_DTYPE).reshape(B, cap)
    fill_info = np.full((B, cap * 16), FILL, np.uint8).view(sdm.INFO_DTYPE).reshape(B, cap)
    for a in (iq, cands, counts, status, fill_st, fill_info):
        a.setflags(write=False)
    return dict(iq=iq, cands=cands, counts=counts, status=status, where=where, fill_st=fill_st, fill_info=fill_info, cache={})


def three_forms(oracle, dec_host, dec_dev, d, sets, gate, mpf, iters=20):
    """the host form (on dec_host, whose max_frames cuts the frames in two chunks), the device form between guard bands and the
    device form in place against the restatement, byte for byte -> the restatement's info"""
    B, cap = d["cands"].shape
    kw = dict(iters=iters, bp=oracle.bp_decode, cache=d["cache"])
    want_st, want_info = sdm.demod_candidates(oracle, d["iq"], d["cands"], d["counts"], d["status"], sets, gate, mpf, status_out=d["fill_st"],
                                              info=d["fill_info"], **kw)
    want_in, _ = sdm.demod_candidates(oracle, d["iq"], d["cands"], d["counts"], d["status"], sets, gate, mpf, status_out=d["status"],
                                      info=d["fill_info"], **kw)
    assert B > dec_host.max_frames >= (B + 1) // 2 and dec_dev.max_frames >= B
    st, info = dec_host.demod_candidates(d["iq"], d["cands"], d["counts"], d["status"], sets, gate, mpf, status_out=d["fill_st"], info=d["fill_info"])
    for f in range(B):
        for i in range(cap):
            assert info[f, i].tobytes() == want_info[f, i].tobytes(), (sets, gate, mpf, f, i, info[f, i], want_info[f, i])
            assert st[f, i].tobytes() == want_st[f, i].tobytes(), (sets, gate, mpf, f, i, "host")
    assert demod_dev(dec_dev, d, d["counts"], sets, gate, mpf, False) == (want_st.tobytes(), want_info.tobytes()), (sets, gate, mpf, "device")
    assert demod_dev(dec_dev, d, d["counts"], sets, gate, mpf, True) == (want_in.tobytes(), want_info.tobytes()), (sets, gate, mpf, "in place")
    return want_info


@pytest.fixture(scope="module")
def edges(oracle):
    import rtlsdr_ft8d_amd as ft8
    return as_inputs(ft8, *de.constructed(ft8, oracle))


@pytest.mark.parametrize("ieee", [False, True])
def test_stage_entry_equals_the_restatement_on_constructed_edges(edges, oracle, ieee):
    """18 frames (the host form in two chunks of 9) under every mask at gate 174, and under the gates nhard and nhard - 1 of the
    signals that set 2 and set 3 accept"""
    import rtlsdr_ft8d_amd as ft8
    d, w = edges, edges["where"]
    B = len(d["iq"])
    nh = w["nhard"]
    seen, accepted = set(), set()
    with ft8.Decoder(device=0, max_frames=B, max_candidates=CAP) as dec, ft8.Decoder(device=0, max_frames=(B + 1) // 2, max_candidates=CAP) as dec2:
        for k in (dec, dec2):
            k.set_debug_flags(ft8.DBG_FORCE_IEEE_DIV if ieee else 0)
        for sets in range(1, 8):
            info = three_forms(oracle, dec2, dec, d, sets, 174, CAP)
            last = sets.bit_length()
            assert [(int(info[w[n]]["result"]), int(info[w[n]]["set"])) for n in ("crc_refuses", "unpack_refuses", "all_zero_word")] == \
                [(3, last), (4, last), (7, last)]
            assert info[w["good_behind_a_refusal"]]["result"] == 1
            seen |= set(int(r) for f in range(B) for r in info[f, :d["counts"][f]]["result"])
            accepted |= set(int(r["set"]) for f in range(B) for r in info[f, :d["counts"][f]] if r["result"] == 1)
        assert (int(info[w["set2_accepts"]]["set"]), int(info[w["set3_accepts"]]["set"])) == (2, 3)
        assert info[w["scaled_nan_psync"]]["psync"].view(np.uint32) == 0x7FC00000 and info[w["nan_payload"]]["psync"].view(np.uint32) == 0x7FC00000
        assert info[w["scaled_inf_psync"]]["psync"].view(np.uint32) == 0x7F800000 and info[w["scaled_inf_psync"]]["e_best"] > -4
        assert 0 < info[w["scaled_subnormal_psync"]]["psync"].view(np.uint32) < 0x00800000
        for name, n in (("set2_accepts", 2), ("set3_accepts", 3)):
            info = three_forms(oracle, dec2, dec, d, 7, nh[name], CAP)
            r = info[w[name]]
            assert (r["result"], r["set"], r["nhard"]) == (1, n, nh[name]), (name, r)
            info = three_forms(oracle, dec2, dec, d, 7, nh[name] - 1, CAP)
            r = info[w[name]]
            assert r["result"] != 1 and r["set"] == 3 and (n == 2 or (r["result"], r["nhard"]) == (2, nh[name])), (name, r)
            info = three_forms(oracle, dec2, dec, d, 1 << (n - 1), nh[name] - 1, CAP)
            r = info[w[name]]
            assert (r["result"], r["set"], r["nhard"]) == (2, n, nh[name]), (name, r)
            seen |= set(int(r) for f in range(B) for r in info[f, :d["counts"][f]]["result"])
    assert {0, 1, 2, 3, 4, 6, 7} <= seen and 5 not in seen and accepted == {1, 2, 3}


LONG_MPF = {70: (0, 1, 43, 44, 63, 64, 65, 70), 7: (0, 3, 7)}
LONG_INPUTS = {}                              # max_candidates: the inputs, with the restatement's analyses of their three records


@pytest.mark.parametrize("ieee", [False, True])
@pytest.mark.parametrize("cap", [70, 7])
def test_long_lists_reach_the_second_chunk_of_the_selection(oracle, cap, ieee):
    """max_candidates = 70: the selection kernel ranks in two chunks of 64 with a carried base (the 43rd qualifying record is
    record 63, the 44th record 64) and the last of 18 workgroups per frame has two waves; max_candidates = 7: two workgroups,
    the second with three"""
    import rtlsdr_ft8d_amd as ft8
    if cap not in LONG_INPUTS:
        LONG_INPUTS[cap] = as_inputs(ft8, *de.long_lists(ft8, cap))
    d = LONG_INPUTS[cap]
    B = len(d["iq"])
    q = (d["status"]["ok"] == 0) & (d["status"]["ldpc_errors"] != 0) & (np.arange(cap)[None, :] < d["counts"][:, None])
    with ft8.Decoder(device=0, max_frames=B, max_candidates=cap) as dec, ft8.Decoder(device=0, max_frames=B // 2, max_candidates=cap) as dec2:
        for k in (dec, dec2):
            k.set_debug_flags(ft8.DBG_FORCE_IEEE_DIV if ieee else 0)
        for mpf in LONG_MPF[cap]:
            three_forms(oracle, dec2, dec, d, 7, 174, mpf)
            _st, info = dec.demod_candidates(d["iq"], d["cands"], d["counts"], d["status"], 7, 174, mpf)
            for f in range(B):
                first = np.flatnonzero(q[f])[:mpf]
                assert np.flatnonzero(info[f]["set"] != 0).tolist() == first.tolist(), (mpf, f)
                assert len(first) == min(mpf, int(q[f].sum()))


@pytest.mark.parametrize("ieee", [False, True])
@pytest.mark.parametrize("iters", [1, 5, 50])
def test_ldpc_iters_is_the_context_s(edges, oracle, iters, ieee):
    """the refusals and the weak signals on contexts with ldpc_iters 1, 5 and 50; the restatement runs bp_decode with the same"""
    import rtlsdr_ft8d_amd as ft8
    w = edges["where"]
    frames = sorted({w[n][0] for n in ("crc_refuses", "set2_accepts", "set3_accepts")})
    assert len(frames) == 2
    d = as_inputs(ft8, *(edges[k][frames].copy() for k in ("iq", "cands", "counts", "status")))
    with ft8.Decoder(device=0, max_frames=2, max_candidates=CAP, ldpc_iters=iters) as dec, \
            ft8.Decoder(device=0, max_frames=1, max_candidates=CAP, ldpc_iters=iters) as dec2:
        for k in (dec, dec2):
            k.set_debug_flags(ft8.DBG_FORCE_IEEE_DIV if ieee else 0)
        info = three_forms(oracle, dec2, dec, d, 7, 174, CAP, iters=iters)
    results = [int(r) for f in range(2) for r in info[f, :d["counts"][f]]["result"]]
    assert 7 in results and (iters == 1 or {1, 3, 4} <= set(results)), results


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
