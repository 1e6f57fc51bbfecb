"""GPU tests of a-priori decoding (ft8gpu_ap_candidates / ft8gpu_decode_messages_ap): the stage entry against the restatement
(tests/ft8_spec_ap.py) byte for byte in status and info, every output pre-filled with 0xA5 -- on radio frames, on the
constructed soft bits of tests/ap_craft.py at ldpc_iters 1 / 5 / 20 / 50 with both division streams, at max_candidates 1..5
and 1024 on nine frames with ragged counts -- in the host form (chunked), the device form and the device form in place; the
frozen fixture; the whole path against the chain of restatements (multi-pass, AP, OSD) with its tags and stage counts; the
identity with ft8gpu_decode_messages_deep at nhyp = 0; refused arguments.  tests/test_ap_cpu.py proves on the CPU that the
frames and cases are what they are taken for."""
import ctypes as C
import os

import numpy as np
import pytest

import ap_craft as ac
import ft8_spec_ap as sa
import ft8_spec_messages as sm
import osd_craft as oc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
RECOMMENDED = 40
OSD_GATE = 83                                            # the whole path's OSD gate: none, so that OSD gains behind AP on these frames


def _filled_msgs(B):
    import rtlsdr_ft8d_amd as ft8
    return np.full((B, 50 * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(B, 50)


def _fills(B, cap):
    st = np.full((B, cap, 48), FILL, np.uint8)
    info = np.full((B, cap * 8), FILL, np.uint8).view(sa.INFO_DTYPE).reshape(B, cap)
    return st, info


def _first_difference(got_info, want_info):
    bad = np.argwhere(got_info.view(np.uint64).reshape(want_info.shape) != want_info.view(np.uint64).reshape(want_info.shape))
    if not len(bad):
        return None
    f, i = bad[0]
    return len(bad), (int(f), int(i)), got_info[f, i], want_info[f, i]


def _check_three_forms(ft8, dec, oracle, mag, cands, counts, status_in, hyps, gate, iters, cache, what):
    """host form, device form out of place, device form in place against the restatement; returns its info records"""
    import torch
    B, cap = cands.shape
    fill_st, fill_info = _fills(B, cap)
    want_st, want_info = sa.ap_candidates(oracle, mag, cands, counts, status_in, hyps, gate, status_out=fill_st, info=fill_info,
                                          iters=iters, cache=cache)
    got_st, got_info = dec.ap_candidates(mag, cands, counts, status_in, hyps, gate, status_out=fill_st, info=fill_info)
    assert got_info.tobytes() == want_info.tobytes(), (what, _first_difference(got_info, want_info))
    assert got_st.tobytes() == want_st.tobytes(), what
    ins = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda() for a in (mag, cands, counts, status_in)]
    out_d = torch.full((B, cap, 48), FILL, dtype=torch.uint8, device="cuda")
    info_d = torch.full((B, cap, 8), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dec.ap_candidates_dev(*ins, B, hyps, gate, out_d, info_d)
    dec.synchronize()
    assert info_d.cpu().numpy().tobytes() == want_info.tobytes() and out_d.cpu().numpy().tobytes() == want_st.tobytes(), what
    same = ins[3].clone()
    info_d.fill_(FILL)
    torch.cuda.synchronize()
    dec.ap_candidates_dev(ins[0], ins[1], ins[2], same, B, hyps, gate, same, info_d)
    dec.synchronize()
    w2, _ = sa.ap_candidates(oracle, mag, cands, counts, status_in, hyps, gate, status_out=status_in, iters=iters, cache=cache)
    assert same.cpu().numpy().tobytes() == w2.tobytes() and info_d.cpu().numpy().tobytes() == want_info.tobytes(), what
    return want_info


def test_recommended_gate_is_the_headers():
    import rtlsdr_ft8d_amd as ft8
    hdr = open(os.path.join(ROOT, "include", "ft8gpu.h")).read()
    assert f"#define FT8GPU_AP_MAX_HARD_ERRORS {RECOMMENDED}\n" in hdr and ft8.AP_MAX_HARD_ERRORS == RECOMMENDED
    assert "#define FT8GPU_AP_MAX_HYPOTHESES 4\n" in hdr and ft8.AP_MAX_HYPOTHESES == sa.MAX_HYPOTHESES == 4


# ---- radio frames ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def radio(oracle):
    """the eight chosen frames at cap 120 with ragged counts, computed once and not changed"""
    iq, planted = ac.radio_frames(oracle)
    mag = oracle.waterfall_batch(iq, nthreads=8)
    cands, counts = oracle.find_sync_batch(mag, 120, 10, nthreads=8)
    counts[1] //= 2                                                    # ragged: records behind the count stay 0xA5
    counts[6] = 0
    for a in (iq, mag, cands, counts):
        a.setflags(write=False)
    return iq, planted, mag, cands, counts


@pytest.mark.parametrize("pipeline_form", [False, True])
def test_stage_entry_equals_restatement_on_radio_frames(oracle, radio, pipeline_form):
    """status_in from the counting or the pipeline form of the LDPC kernel (ldpc_errors exact, or 0 / 83); "CQ ? ?" without a
    gate and at the recommended one, and with "CQ DX ? ?" behind it; host form chunked by max_frames 3"""
    import rtlsdr_ft8d_amd as ft8
    iq, planted, mag, cands, counts = radio
    cq, cqdx = sa.cq_hypothesis(), sa.from_text("CQ DX ? ?")
    with ft8.Decoder(device=0, max_frames=3) as dec:
        dec.set_debug_flags(ft8.DBG_PIPELINE_FORM if pipeline_form else 0)
        status_in = dec.decode_candidates(mag, cands, counts)
        if pipeline_form:
            assert set(np.unique(np.concatenate([status_in[f, :counts[f]]["ldpc_errors"] for f in range(len(mag))]))) <= {0, 83}
        seen, accepted = set(), 0
        for hyps, gate, cache in (([cq], 174, {}), ([cq], RECOMMENDED, {}), ([cq, cqdx], 18, {})):
            info = _check_three_forms(ft8, dec, oracle, mag, cands, counts, status_in, hyps, gate, 20, cache, (len(hyps), gate))
            seen |= set(int(r) for f in range(len(mag)) for r in info[f, :counts[f]]["results"].ravel())
            accepted += int((info["result"] == 1).sum())
        assert {0, 1, 2, 7} <= seen and accepted >= 9, (seen, accepted)      # 2: refused by the gate 18, then "CQ DX ? ?" is tried


# ---- constructed soft bits -----------------------------------------------------------------------------------------------------

_constructed = {}


def _built(oracle):
    if "b" not in _constructed:
        cases, frames, mag, configs = ac.build(oracle)
        for a in (mag, frames["cands"], frames["counts"], frames["status_in"]):
            a.setflags(write=False)
        _constructed["b"] = (cases, frames, mag, configs)
    return _constructed["b"]


@pytest.mark.parametrize("force_ieee", [False, True])
@pytest.mark.parametrize("iters", [1, 5, 20, 50])
def test_stage_entry_equals_restatement_on_constructed_cases(oracle, iters, force_ieee):
    """every configuration of ap_craft.configs (hypothesis tables of 1, 2 and 4, masks of 1, 32 and 77 bits, gates on both
    sides of the planted messages' hard errors) at four iteration counts, with the guarded fast divisions and with
    FT8GPU_DBG_FORCE_IEEE_DIV; host form chunked by max_frames 2 over 3 frames"""
    import rtlsdr_ft8d_amd as ft8
    cases, frames, mag, configs = _built(oracle)
    cands = frames["cands"].view(ft8.CAND_DTYPE).reshape(len(mag), -1)
    caches = _constructed.setdefault(("caches", iters), {})           # the restatement's attempts, shared by both division streams
    seen = set()
    with ft8.Decoder(device=0, max_frames=2, max_candidates=oc.CAP, ldpc_iters=iters) as dec:
        dec.set_debug_flags(ft8.DBG_FORCE_IEEE_DIV if force_ieee else 0)
        for name, hyps, gate in configs:
            cache = caches.setdefault(name.split("_gate_")[0] if "_gate_" in name else name, {})
            info = _check_three_forms(ft8, dec, oracle, mag, cands, frames["counts"], frames["status_in"], hyps, gate, iters, cache,
                                      (name, iters, force_ieee))
            seen |= set(int(r) for f in range(len(mag)) for r in info[f, :frames["counts"][f]]["result"])
    assert {0, 1, 6, 7} <= seen and (iters != ac.ITERS or seen == {0, 1, 2, 3, 4, 6, 7, 8}), (iters, seen)


def test_frozen_constructed_fixture_on_the_device():
    import rtlsdr_ft8d_amd as ft8
    d = np.load(os.path.join(ROOT, "tests", "golden", "ap_constructed.npz"))
    B = len(d["counts"])
    frames = dict(cands=d["cands"].view(oc.CAND_DTYPE).reshape(B, -1), counts=d["counts"], status_in=d["status_in"], vec=d["vec"])
    mag = oc.waterfalls(d["vectors"], frames)
    cands = frames["cands"].view(ft8.CAND_DTYPE).reshape(B, -1)
    with ft8.Decoder(device=0, max_frames=B, max_candidates=cands.shape[1]) as dec:
        for name, gate in zip(d["configs"], d["gates"]):
            hyps = d[f"hyps_{name}"].view(sa.HYP_DTYPE).copy()
            st, info = dec.ap_candidates(mag, cands, d["counts"], d["status_in"], list(hyps), int(gate), status_out=d["status_in"])
            assert info.view(np.uint8).tobytes() == d[f"info_{name}"].tobytes(), name
            assert st.tobytes() == ac.fixture_status(d, str(name)).tobytes(), name


# ---- other caps ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 2, 3, 4, 5, 1024])
def test_stage_entry_at_other_caps(oracle, radio, cap):
    """max_candidates 1..4 is one workgroup per frame (the frame index needs no division), 5 is two, 1024 is 256: nine frames
    -- the eight radio frames and a noise frame -- so that a wrong frame index shows, with ragged counts and guard bands
    behind them.  At 1024 min_score is 0 and the lists are full before they are cut."""
    import rtlsdr_ft8d_amd as ft8
    ms = 0 if cap > 5 else 10
    iq = np.concatenate([radio[0], ac.radio_frames(oracle, ac.NOISE_SEEDS[:1], 0)[0]])
    B = len(iq)
    assert B == 9
    mag = oracle.waterfall_batch(iq, nthreads=8)
    cands, counts = oracle.find_sync_batch(mag, cap, ms, nthreads=8)
    if cap > 5:
        assert (counts == cap).all()
        counts[:] = [cap, 0, 1, 700, 4, 5, 1023, 64, 3]               # ragged: every kind of block -- full, partly used, unused
    else:
        counts[3] = 0
    hyps = [sa.cq_hypothesis(), sa.from_text("CQ DX ? ?")] if cap <= 5 else [sa.cq_hypothesis()]
    with ft8.Decoder(device=0, max_frames=4, max_candidates=cap, min_score=ms) as dec:
        status_in = dec.decode_candidates(mag, cands, counts)
        info = _check_three_forms(ft8, dec, oracle, mag, cands, counts, status_in, hyps, 174, 20, {}, cap)
    attempted = int(sum((info[f, :counts[f]]["result"] != 0).sum() for f in range(B)))
    assert attempted >= (1500 if cap > 5 else 1), attempted
    if cap > 5:
        assert (info["result"] == 1).sum() >= 5


# ---- the whole path --------------------------------------------------------------------------------------------------------------

_whole = {}


def _dev_ap(ft8, dec, iq_d, B, passes, hyps, gate, order, osd_gate, nbs=True):
    import torch
    msgs = torch.full((B, 50 * 64), FILL, dtype=torch.uint8, device="cuda")
    n = torch.full((B,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    nb = torch.full((B, passes, 3), -0x5A5A5A5B, dtype=torch.int32, device="cuda") if nbs else None
    torch.cuda.synchronize()
    dec.decode_messages_ap_dev(iq_d, B, passes, hyps, gate, order, osd_gate, msgs, n, nb)
    dec.synchronize()
    return msgs.cpu().numpy().view(ft8.MESSAGE_DTYPE).reshape(B, 50), n.cpu().numpy(), (nb.cpu().numpy() if nbs else None)


@pytest.mark.parametrize("osd_order", [-1, 1])
@pytest.mark.parametrize("passes", [1, 2])
def test_whole_path_equals_the_chain_of_restatements(oracle, radio, passes, osd_order):
    """eight frames: every pass as tests/ft8_spec_multipass.py, then AP ("CQ ? ?", "CQ DX ? ?") and OSD (order 1, no gate) in place on the pass's records, each followed by the append step.  Host and device form; pad[1] = 1 + hyp
    on what AP gained, pad[0] = nhard on what OSD gained, n_by_stage the counts after BP, AP and OSD."""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = radio[0]
    B = len(iq)
    hyps = [sa.cq_hypothesis(), sa.from_text("CQ DX ? ?")]
    want, wn, wnbs = sa.decode_ap(oracle, iq, passes, hyps, RECOMMENDED, osd_order, OSD_GATE, msgs=_filled_msgs(B),
                                  searches=_whole.setdefault("searches", {}), cache=_whole.setdefault("cache", {}))
    with ft8.Decoder(device=0, max_frames=5) as dec:                  # chunks of 5 and 3
        got, n, nbs = dec.decode_messages_ap(iq, passes, hyps, RECOMMENDED, osd_order, OSD_GATE, _filled_msgs(B))
        assert np.array_equal(n, wn) and np.array_equal(nbs, wnbs), (n, wn, nbs.tolist(), wnbs.tolist())
        assert got.tobytes() == want.tobytes(), sm.check(got, n, want, wn)
        dm, dn, dnbs = _dev_ap(ft8, dec, torch.from_numpy(np.array(iq)).cuda(), B, passes, hyps, RECOMMENDED, osd_order,
                               OSD_GATE)
        assert np.array_equal(dn, wn) and np.array_equal(dnbs, wnbs) and dm.tobytes() == want.tobytes()
    by_ap = (nbs[:, :, 1] - nbs[:, :, 0]).sum(axis=1)
    by_osd = (nbs[:, :, 2] - nbs[:, :, 1]).sum(axis=1)
    print(f"passes {passes} osd_order {osd_order}: n_by_stage {nbs.tolist()}")
    assert by_ap.sum() >= 8 and (osd_order < 0) == (by_osd.sum() == 0)
    for f in range(B):
        pad = got[f, :n[f]]["pad"]
        assert ((pad[:, 1] > 0).sum(), (pad[:, 0] > 0).sum()) == (by_ap[f], by_osd[f]) and not pad[:, 2:].any()
        assert set(pad[:, 1]) <= {0, 1, 2} and not ((pad[:, 0] > 0) & (pad[:, 1] > 0)).any()
        assert (np.diff(nbs[f].reshape(-1)) >= 0).all() and nbs[f, -1, 2] == n[f]


def test_without_hypotheses_the_whole_path_is_the_deep_entry(oracle, radio):
    """nhyp = 0: the messages, the counts and the stage counts of ft8gpu_decode_messages_deep (the AP column repeats BP's);
    n_by_stage NULL is accepted"""
    import rtlsdr_ft8d_amd as ft8
    iq = radio[0]
    B = len(iq)
    with ft8.Decoder(device=0, max_frames=B) as dec:
        for passes, order in ((1, -1), (2, 1)):
            want, wn, wnbs = dec.decode_messages_deep(iq, passes, order, ft8.OSD_MAX_HARD_ERRORS, _filled_msgs(B))
            got, n, nbs = dec.decode_messages_ap(iq, passes, (), 0, order, ft8.OSD_MAX_HARD_ERRORS, _filled_msgs(B))
            assert np.array_equal(n, wn) and got.tobytes() == want.tobytes()
            assert np.array_equal(nbs[:, :, 0], wnbs[:, :, 0]) and np.array_equal(nbs[:, :, 1], wnbs[:, :, 0])
            assert np.array_equal(nbs[:, :, 2], wnbs[:, :, 1])
        m, k = _filled_msgs(B), np.zeros(B, np.int32)
        p = ft8._ap_params(2, (), 0, 1, ft8.OSD_MAX_HARD_ERRORS)
        assert dec.lib.ft8gpu_decode_messages_ap(dec.h, iq.ctypes.data, B, C.byref(p), m.ctypes.data, k.ctypes.data, None, ft8.HOST_PTRS) == 0
        assert np.array_equal(k, wn) and m.tobytes() == want.tobytes()


def test_refused_arguments_leave_the_outputs_alone(oracle, radio):
    import rtlsdr_ft8d_amd as ft8
    iq, planted, mag, cands, counts = radio
    mag, cands, counts = mag[:2], np.array(cands[:2]), np.array(counts[:2])
    cq = sa.cq_hypothesis()
    outside = cq.copy()
    outside["bits"][5] |= 0x01                                         # bit 47 is not masked
    empty = np.zeros(1, sa.HYP_DTYPE)[0]
    past = cq.copy()
    past["mask"][9] |= 0x04                                            # bit 77
    with ft8.Decoder(device=0, max_frames=2) as dec:
        status = dec.decode_candidates(mag, cands, counts)
        fill_st, fill_info = _fills(2, 120)

        def stage(hyps, nhyp, gate):
            st, info = fill_st.copy(), fill_info.copy()
            h = ac.hyps_array(hyps)
            rc = dec.lib.ft8gpu_ap_candidates(dec.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status.ctypes.data, 2,
                                              h.ctypes.data, nhyp, gate, st.ctypes.data, info.ctypes.data, ft8.HOST_PTRS)
            assert st.tobytes() == fill_st.tobytes() and info.tobytes() == fill_info.tobytes()
            return rc, dec.lib.ft8gpu_last_error().decode()

        for hyps, nhyp, gate, word in (([cq], 0, 40, "nhyp"), ([cq] * 5, 5, 40, "nhyp"), ([cq], -1, 40, "nhyp"),
                                       ([cq, outside], 2, 40, "hypothesis 1 has bits outside its mask"), ([cq], 1, 175, "max_hard_errors"),
                                       ([cq], 1, -1, "max_hard_errors"), ([empty], 1, 40, "masks no bit"), ([past], 1, 40, "past the 77")):
            rc, err = stage(hyps, nhyp, gate)
            assert rc != 0 and word in err, (nhyp, gate, err)
        assert dec.lib.ft8gpu_ap_candidates(dec.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status.ctypes.data, 2,
                                            None, 1, 40, fill_st.ctypes.data, fill_info.ctypes.data, ft8.HOST_PTRS) != 0
        assert b"hyps" in dec.lib.ft8gpu_last_error()
        h = ac.hyps_array([cq])
        assert dec.lib.ft8gpu_ap_candidates(dec.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status.ctypes.data, 2,
                                            h.ctypes.data, 1, 40, None, fill_info.ctypes.data, ft8.HOST_PTRS) != 0
        assert b"NULL" in dec.lib.ft8gpu_last_error()
        # gates 0 and 174 are the ends of the accepted range
        dec.ap_candidates(mag, cands, counts, status, [cq], 0)
        dec.ap_candidates(mag, cands, counts, status, [cq], 174)
        # the whole path
        for passes, hyps, gate, order, osd_gate, word in ((0, [cq], 40, 1, 27, "passes"), (5, [cq], 40, 1, 27, "passes"),
                                                         (1, [cq] * 5, 40, 1, 27, "nhyp"), (1, [cq], 175, 1, 27, "max_hard_errors"),
                                                         (1, [outside], 40, -1, 27, "outside its mask"), (1, [cq], 40, 3, 27, "osd_order"),
                                                         (1, [cq], 40, 1, 84, "max_hard_errors")):
            msgs = _filled_msgs(1)
            with pytest.raises(ft8.Ft8GpuError, match=word):
                dec.decode_messages_ap(iq[:1], passes, hyps, gate, order, osd_gate, msgs)
            assert msgs.tobytes() == _filled_msgs(1).tobytes()
        k = np.zeros(1, np.int32)
        assert dec.lib.ft8gpu_decode_messages_ap(dec.h, iq.ctypes.data, 1, None, msgs.ctypes.data, k.ctypes.data, None, ft8.HOST_PTRS) != 0
        assert b"params" in dec.lib.ft8gpu_last_error()
