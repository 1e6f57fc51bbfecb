"""GPU tests of ordered-statistics decoding (ft8gpu_osd_candidates / ft8gpu_decode_messages_deep): the stage entry and the
whole path against the numpy restatement (tests/ft8_spec_osd.py), byte for byte with every output pre-filled with 0xA5; the
frozen fixture; the two identity properties of the whole path; chunking; refused arguments; the gain on the 96 crowded
frames of profiles/osd_gain.json; the parameter edges -- max_candidates 1..5, 480 and 1024, ldpc_iters 1 and 50, four passes,
a cap grown by ft8gpu_set_params on a live context.  Constructed soft bits: tests/test_gpu_osd_constructed.py."""
import json
import os

import numpy as np
import pytest

import ft8_spec_messages as sm
import ft8_spec_multipass as mp
import ft8_spec_osd as so

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
RECOMMENDED = 27
CONFIGS = [(order, gate) for order in (0, 1, 2) for gate in (83, RECOMMENDED, 20)]


def _filled_msgs(B):
    import rtlsdr_ft8d_amd as ft8
    return np.full((B, 50 * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(B, 50)


def _cq_frames(oracle, seeds, nsig, snr=(-22.0, 0.0)):
    import synth_util as S
    enc = S.oracle_encode_fn(oracle)
    fr = [S.make_frame(s, nsig, enc, snr_range=snr) for s in seeds]
    return np.stack([f[0] for f in fr]), [f[1] for f in fr]


def _mixed_frames(seeds, nsig):
    import synth_util as S
    from rtlsdr_ft8d_amd import workload
    texts, tones = workload.mixed_message_pool(1024, seed=7)
    return np.stack([S.make_mixed_frame(s, nsig, (-22.0, 0.0), texts, tones)[0] for s in seeds])


def _workloads(oracle):
    """the three workloads of profiles/osd_gain.json (20 CQ signals, one weak signal, noise only), mixed traffic, and an
    all-zero frame: 16 frames, the zero frame last"""
    return np.concatenate([_cq_frames(oracle, range(1000, 1005), 20)[0], _cq_frames(oracle, range(1000, 1003), 1, (-24.0, -14.0))[0],
                           _cq_frames(oracle, range(5000, 5003), 0)[0], _mixed_frames(range(1000, 1004), 20),
                           np.zeros((1, 2, 48000), np.float32)])


def test_recommended_gate_is_the_headers():
    import rtlsdr_ft8d_amd as ft8
    hdr = open(os.path.join(ROOT, "include", "ft8gpu.h")).read()
    assert f"#define FT8GPU_OSD_MAX_HARD_ERRORS {RECOMMENDED}\n" in hdr and ft8.OSD_MAX_HARD_ERRORS == RECOMMENDED


@pytest.mark.parametrize("pipeline_form", [False, True])
@pytest.mark.parametrize("cap", [120, 33])
def test_stage_entry_equals_restatement(oracle, cap, pipeline_form):
    """orders 0 / 1 / 2 x gates 83 / recommended / 20, status_in from the counting or the pipeline form of the LDPC kernel,
    ragged counts, a frame of fabricated candidates on an all-zero waterfall (non-finite soft bits); host form chunked by
    max_frames 7, device form out of place and in place"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = _workloads(oracle)
    B = len(iq)
    mag = oracle.waterfall_batch(iq, nthreads=8)
    cands, counts = oracle.find_sync_batch(mag, cap, 10, nthreads=8)
    assert counts[B - 1] == 0 and not mag[B - 1].any()
    for i in range(5):                                                 # the zero frame: every soft bit is 0 / 0
        cands[B - 1, i] = (10, 2 * i - 3, 40 * i + 3, i & 1, (i >> 1) & 1)
    counts[B - 1] = 5
    counts[1] //= 2                                                    # ragged: records behind the count stay 0xA5
    counts[2] = 0
    counts[6] = min(int(counts[6]), 3)
    with ft8.Decoder(device=0, max_frames=7, max_candidates=cap) as dec:
        dec.set_debug_flags(ft8.DBG_PIPELINE_FORM if pipeline_form else 0)
        status_in = dec.decode_candidates(mag, cands, counts)
        st = status_in
        want_errors = {0, 83} if pipeline_form else None
        if want_errors:
            assert set(np.unique(np.concatenate([st[f, :counts[f]]["ldpc_errors"] for f in range(B)]))) <= want_errors
        fill_st = np.full((B, cap, 48), FILL, np.uint8)
        fill_info = np.full((B, cap), FILL, np.uint8).repeat(8, axis=1).view(so.INFO_DTYPE).reshape(B, cap)
        searches, results = {}, set()
        ins = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda() for a in (mag, cands, counts, status_in)]
        for order, gate in CONFIGS:
            want_st, want_info = so.osd_candidates(oracle, mag, cands, counts, status_in, order, gate, status_out=fill_st,
                                                   info=fill_info, searches=searches)
            got_st, got_info = dec.osd_candidates(mag, cands, counts, status_in, order, gate, status_out=fill_st, info=fill_info)
            bad = np.argwhere(got_info.view(np.uint64) != want_info.view(np.uint64))
            assert got_info.tobytes() == want_info.tobytes(), (order, gate, bad[:4], got_info[tuple(bad[0])], want_info[tuple(bad[0])])
            assert got_st.tobytes() == want_st.tobytes(), (order, gate)
            results |= set(int(r) for f in range(B) for r in want_info[f, :counts[f]]["result"])
            # device pointers, one call over the chunks; then in place
            out_d = torch.full((B, cap, 48), FILL, dtype=torch.uint8, device="cuda")
            info_d = torch.full((B, cap, 8), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dec.osd_candidates_dev(*ins, B, order, gate, out_d, info_d)
            dec.synchronize()
            assert out_d.cpu().numpy().tobytes() == want_st.tobytes() and info_d.cpu().numpy().tobytes() == want_info.tobytes()
            if gate == RECOMMENDED:
                inplace = ins[3].clone()
                torch.cuda.synchronize()
                dec.osd_candidates_dev(ins[0], ins[1], ins[2], inplace, B, order, gate, inplace, info_d)
                dec.synchronize()
                w2, _ = so.osd_candidates(oracle, mag, cands, counts, status_in, order, gate, status_out=status_in, searches=searches)
                assert inplace.cpu().numpy().tobytes() == w2.tobytes() and info_d.cpu().numpy().tobytes() == want_info.tobytes()
        assert {0, 2, 3, 6} <= results and (1 in results or cap == 33), results


def test_frozen_fixture_on_the_device():
    import rtlsdr_ft8d_amd as ft8
    d = np.load(os.path.join(ROOT, "tests", "golden", "osd_frame.npz"))
    cands = d["cands"].view(ft8.CAND_DTYPE).reshape(1, -1)
    with ft8.Decoder(device=0, max_frames=1) as dec:
        for order, gate in d["configs"]:
            st, info = dec.osd_candidates(d["mag"], cands, d["counts"], d["status_in"], int(order), int(gate))
            assert info.tobytes() == d[f"info_o{order}_g{gate}"].tobytes(), (order, gate)
            assert st.tobytes() == d[f"status_o{order}_g{gate}"].tobytes(), (order, gate)


def _deep_batch(oracle):
    crowded, _ = _cq_frames(oracle, range(1000, 1004), 20)
    dense, _ = _cq_frames(oracle, range(5000, 5003), 30)
    single, _ = _cq_frames(oracle, range(1000, 1002), 1, (-24.0, -14.0))
    noise, _ = _cq_frames(oracle, range(5000, 5002), 0)
    return np.stack([crowded[0], noise[0], dense[0], single[0], crowded[1], crowded[2], noise[1], dense[1], single[1], crowded[3],
                     dense[2]])


def _dev_deep(ft8, dec, iq_d, B, passes, order, gate, nbs=True):
    import torch
    msgs = torch.full((B, 50 * 64), FILL, dtype=torch.uint8, device="cuda")
    n = torch.full((B,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    nb = torch.full((B, passes, 2), -0x5A5A5A5B, dtype=torch.int32, device="cuda") if nbs else None
    torch.cuda.synchronize()
    dec.decode_messages_deep_dev(iq_d, B, passes, order, gate, msgs, n, nb)
    dec.synchronize()
    return msgs.cpu().numpy().view(ft8.MESSAGE_DTYPE).reshape(B, 50), n.cpu().numpy(), (nb.cpu().numpy() if nbs else None)


@pytest.mark.parametrize("passes", [1, 2])
def test_whole_path_equals_restatement(oracle, passes):
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = _deep_batch(oracle)
    B = len(iq)
    iq_d = torch.from_numpy(iq).cuda()
    searches = {}
    gained = 0
    with ft8.Decoder(device=0, max_frames=B) as dec:
        for order, gate in ((1, 83), (2, RECOMMENDED), (2, 83)):
            want, wn, wnbs = so.decode_deep(oracle, iq, passes, order, gate, msgs=_filled_msgs(B), searches=searches)
            got, n, nbs = dec.decode_messages_deep(iq, passes, order, gate, _filled_msgs(B))
            assert np.array_equal(n, wn) and np.array_equal(nbs, wnbs), (order, gate, n, wn, nbs.tolist(), wnbs.tolist())
            assert got.tobytes() == want.tobytes(), (order, gate, sm.check(got, n, want, wn))
            dm, dn, dnbs = _dev_deep(ft8, dec, iq_d, B, passes, order, gate)
            assert np.array_equal(dn, wn) and np.array_equal(dnbs, wnbs) and dm.tobytes() == want.tobytes()
            gained += int((wnbs[:, :, 1] - wnbs[:, :, 0]).sum())
            for f in range(B):                                         # pad[0]: nhard of what OSD gained, 0 for BP's records
                tags = got[f, :n[f]]["pad"][:, 0]
                assert (tags > 0).sum() == (nbs[f, :, 1] - nbs[f, :, 0]).sum() and not got[f, :n[f]]["pad"][:, 1:].any()
    assert gained >= 3


def test_identities_chunking_and_refused_arguments(oracle):
    """osd_order -1 == ft8gpu_decode_messages_passes; passes 1: the slots below the BP count == ft8gpu_decode_messages;
    max_frames 4 walking 11 frames == one call; out-of-range arguments are refused with a message"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = _deep_batch(oracle)
    B = len(iq)
    with ft8.Decoder(device=0, max_frames=B) as dec:
        want, wn, wnbp = dec.decode_messages_passes(iq, 2, _filled_msgs(B))
        got, n, nbs = dec.decode_messages_deep(iq, 2, -1, 0, _filled_msgs(B))
        assert np.array_equal(n, wn) and got.tobytes() == want.tobytes()
        assert np.array_equal(nbs[:, :, 0], wnbp) and np.array_equal(nbs[:, :, 1], wnbp)
        one, n1 = dec.decode_messages(iq, _filled_msgs(B))
        deep, nd, nbs1 = dec.decode_messages_deep(iq, 1, 2, 83, _filled_msgs(B))
        assert np.array_equal(nbs1[:, 0, 0], n1) and (nd >= n1).all() and nd.sum() > n1.sum()
        for f in range(B):
            assert deep[f, :n1[f]].tobytes() == one[f, :n1[f]].tobytes(), f
            assert deep[f, nd[f]:].tobytes() == one[f, nd[f]:].tobytes()      # behind the count: the caller's bytes
        whole = dec.decode_messages_deep(iq, 2, 2, RECOMMENDED, _filled_msgs(B))
        # n_by_stage NULL, host and device form
        m, k = _filled_msgs(B), np.zeros(B, np.int32)
        p = ft8.DeepParams(2, 2, RECOMMENDED)
        import ctypes as C
        assert dec.lib.ft8gpu_decode_messages_deep(dec.h, iq.ctypes.data, B, C.byref(p), m.ctypes.data, k.ctypes.data, None, ft8.HOST_PTRS) == 0
        assert np.array_equal(k, whole[1]) and m.tobytes() == whole[0].tobytes()
        dm, dn, _ = _dev_deep(ft8, dec, torch.from_numpy(iq).cuda(), B, 2, 2, RECOMMENDED, nbs=False)
        assert np.array_equal(dn, whole[1]) and dm.tobytes() == whole[0].tobytes()
        # refused
        for passes, order, gate, word in ((0, 1, 27, "passes"), (5, 1, 27, "passes"), (1, 3, 27, "osd_order"), (1, -2, 27, "osd_order"),
                                         (1, 1, 84, "max_hard_errors"), (1, 1, -1, "max_hard_errors")):
            with pytest.raises(ft8.Ft8GpuError, match=word):
                dec.decode_messages_deep(iq[:1], passes, order, gate)
        assert dec.lib.ft8gpu_decode_messages_deep(dec.h, iq.ctypes.data, B, None, m.ctypes.data, k.ctypes.data, None, ft8.HOST_PTRS) != 0
        assert b"params" in dec.lib.ft8gpu_last_error()
        mag = oracle.waterfall_batch(iq[:2], nthreads=2)
        cands, counts = oracle.find_sync_batch(mag, 120, 10, nthreads=2)
        status = dec.decode_candidates(mag, cands, counts)
        for order, gate, word in ((3, 27, "order"), (-1, 27, "order"), (1, 84, "max_hard_errors"), (1, -1, "max_hard_errors")):
            with pytest.raises(ft8.Ft8GpuError, match=word):
                dec.osd_candidates(mag, cands, counts, status, order, gate)
        info = np.zeros((2, 120), ft8.OSD_INFO_DTYPE)
        assert dec.lib.ft8gpu_osd_candidates(dec.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status.ctypes.data, 2, 1, 27,
                                             None, info.ctypes.data, ft8.HOST_PTRS) != 0
        assert b"NULL" in dec.lib.ft8gpu_last_error()
    with ft8.Decoder(device=0, max_frames=4) as dec:
        chunked = dec.decode_messages_deep(iq, 2, 2, RECOMMENDED, _filled_msgs(B))
        assert np.array_equal(chunked[1], whole[1]) and np.array_equal(chunked[2], whole[2]) and chunked[0].tobytes() == whole[0].tobytes()
        # the stage entry, chunked against one call
        mag = oracle.waterfall_batch(iq, nthreads=8)
        cands, counts = oracle.find_sync_batch(mag, 120, 10, nthreads=8)
        status = dec.decode_candidates(mag, cands, counts)
        a = dec.osd_candidates(mag, cands, counts, status, 2, RECOMMENDED)
    with ft8.Decoder(device=0, max_frames=B) as dec:
        b = dec.osd_candidates(mag, cands, counts, status, 2, RECOMMENDED)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (a[1]["result"] == 1).sum() >= 1


def test_gain_on_the_crowded_frames_of_the_profile(oracle):
    """96 frames of 20 CQ signals (seeds 1000..1095, SNR U[-22, 0] dB), one pass: at orders 1 and 2, gates recommended and
    83, the device finds as many planted messages and as many outside the planted set as the restatement and as
    profiles/osd_gain.json records"""
    import rtlsdr_ft8d_amd as ft8
    prof = json.load(open(os.path.join(ROOT, "profiles", "osd_gain.json")))
    row = [r for r in prof["rows"] if r["name"] == "cq20"][0]
    assert row["frames"] == 96 and row["seeds"] == [1000, 1095]
    iq, planted = _cq_frames(oracle, range(1000, 1096), 20)
    searches = {}
    with ft8.Decoder(device=0, max_frames=96) as dec:
        one, n1 = dec.decode_messages(iq)
        h1, m1 = mp.planted_hits(one, n1, planted)
        assert (h1, m1) == (row["bp_planted"], row["bp_outside"])
        for order in (1, 2):
            for gate in (RECOMMENDED, 83):
                got, n, nbs = dec.decode_messages_deep(iq, 1, order, gate)
                want, wn, wnbs = so.decode_deep(oracle, iq, 1, order, gate, searches=searches)
                assert np.array_equal(n, wn) and np.array_equal(nbs, wnbs) and got.tobytes() == want.tobytes()
                h, m = mp.planted_hits(got, n, planted)
                rec = row["orders"][str(order)][str(gate)]
                print(f"order {order} gate {gate}: planted {h1} -> {h} (+{h - h1}), outside {m}; profile +{rec['new_planted']} / {rec['outside']}")
                assert (h - h1, m - m1) == (rec["new_planted"], rec["outside"]), (order, gate, h - h1, m - m1, rec)
                assert h > h1


# ---- parameter edges: other caps, other iteration counts, four passes, a cap that grows on a live context ---------------------

EDGE_CAPS = [1, 2, 3, 4, 5, 480, 1024]
_edge = {}


def _edge_frames(oracle):
    """frames 0..3 of _deep_batch: crowded, noise, dense (30 signals), one weak signal"""
    if "iq" not in _edge:
        _edge["iq"] = _deep_batch(oracle)[:4]
        _edge["iq"].setflags(write=False)
    return _edge["iq"]


def _edge_min_score(cap):
    return 0 if cap > 5 else 10                                        # at 0 every position of the scan survives: the long lists fill


def _edge_searches(cap):
    """the first pass's pattern searches at a cap, shared by the stage entry's test and the deep path's (same frames, same lists)"""
    return _edge.setdefault(("searches", cap), {})


@pytest.mark.parametrize("cap", EDGE_CAPS)
def test_stage_entry_at_other_caps(oracle, cap):
    """ft8gpu_osd_candidates at both ends of the accepted range of max_candidates on a crowded and a noise frame, status_in from
    the device's own LDPC kernel; above cap 5 min_score is 0 and both lists are full (records up to index cap - 1).  Host form,
    device form, device form in place."""
    import torch
    import rtlsdr_ft8d_amd as ft8
    ms = _edge_min_score(cap)
    mag = oracle.waterfall_batch(_edge_frames(oracle)[:2], nthreads=2)
    cands, counts = oracle.find_sync_batch(mag, cap, ms, nthreads=2)
    if cap > 5:
        assert counts.tolist() == [cap, cap]
    B = 2
    fill_st = np.full((B, cap, 48), FILL, np.uint8)
    fill_info = np.full((B, cap * 8), FILL, np.uint8).view(so.INFO_DTYPE).reshape(B, cap)
    searches = _edge_searches(cap)
    attempted = 0
    with ft8.Decoder(device=0, max_frames=B, max_candidates=cap, min_score=ms) as dec:
        status_in = dec.decode_candidates(mag, cands, counts)
        ins = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda() for a in (mag, cands, counts, status_in)]
        for order, gate in ((0, 83), (1, RECOMMENDED), (2, RECOMMENDED), (2, 83)):
            want_st, want_info = so.osd_candidates(oracle, mag, cands, counts, status_in, order, gate, status_out=fill_st, info=fill_info,
                                                   searches=searches)
            got_st, got_info = dec.osd_candidates(mag, cands, counts, status_in, order, gate, status_out=fill_st, info=fill_info)
            assert got_info.tobytes() == want_info.tobytes() and got_st.tobytes() == want_st.tobytes(), (cap, order, gate)
            out_d = torch.full((B, cap, 48), FILL, dtype=torch.uint8, device="cuda")
            info_d = torch.full((B, cap, 8), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dec.osd_candidates_dev(*ins, B, order, gate, out_d, info_d)
            dec.synchronize()
            assert out_d.cpu().numpy().tobytes() == want_st.tobytes() and info_d.cpu().numpy().tobytes() == want_info.tobytes()
            inplace = ins[3].clone()
            torch.cuda.synchronize()
            dec.osd_candidates_dev(ins[0], ins[1], ins[2], inplace, B, order, gate, inplace, info_d)
            dec.synchronize()
            w2, _ = so.osd_candidates(oracle, mag, cands, counts, status_in, order, gate, status_out=status_in, searches=searches)
            assert inplace.cpu().numpy().tobytes() == w2.tobytes() and info_d.cpu().numpy().tobytes() == want_info.tobytes()
            attempted += int(sum((want_info[f, :counts[f]]["result"] != 0).sum() for f in range(B)))
    assert attempted >= (6 * cap if cap > 5 else 1), attempted         # above cap 5 nearly every record of the full lists is attempted


def _deep_both_forms(ft8, dec, iq, passes, order, gate, want, wn, wnbs, what):
    import torch
    B = len(iq)
    got, n, nbs = dec.decode_messages_deep(iq, passes, order, gate, _filled_msgs(B))
    assert np.array_equal(n, wn) and np.array_equal(nbs, wnbs), (what, n, wn, nbs.tolist(), wnbs.tolist())
    assert got.tobytes() == want.tobytes(), (what, sm.check(got, n, want, wn))
    dm, dn, dnbs = _dev_deep(ft8, dec, torch.from_numpy(np.array(iq)).cuda(), B, passes, order, gate)
    assert np.array_equal(dn, wn) and np.array_equal(dnbs, wnbs) and dm.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("cap,iters", [(cap, 20) for cap in EDGE_CAPS] + [(120, 1), (120, 50)])
def test_deep_path_at_other_caps_and_iteration_counts(oracle, cap, iters):
    """ft8gpu_decode_messages_deep, 2 passes, order 2, the recommended gate: four frames at caps 1..5 and at ldpc_iters 1 and 50,
    the crowded and the dense frame at cap 480, the crowded frame alone at cap 1024 (full lists: the restatement's searches
    set the size); host and device form, n_by_stage too"""
    import rtlsdr_ft8d_amd as ft8
    ms = _edge_min_score(cap)
    iq = _edge_frames(oracle)
    iq = iq[:1] if cap == 1024 else (iq[[0, 2]] if cap == 480 else iq)
    B = len(iq)
    searches = _edge_searches(cap) if iters == 20 and cap != 480 else {}      # at 480 frame 1 is another frame than the stage entry's
    want, wn, wnbs = so.decode_deep(oracle, iq, 2, 2, RECOMMENDED, max_candidates=cap, min_score=ms, msgs=_filled_msgs(B), searches=searches,
                                    iters=iters)
    with ft8.Decoder(device=0, max_frames=B, max_candidates=cap, min_score=ms, ldpc_iters=iters) as dec:
        _deep_both_forms(ft8, dec, iq, 2, 2, RECOMMENDED, want, wn, wnbs, (cap, iters))
    print(f"cap {cap} iters {iters}: n_by_stage {wnbs.tolist()}")
    assert wn.sum() >= 1 and (cap < 120 or (wnbs[:, :, 1] > wnbs[:, :, 0]).any())      # at the reference's cap and above, OSD gains


def test_deep_path_with_four_passes(oracle):
    """three dense frames (30 signals), a noise frame, a weak single signal, a crowded frame: pass 3 runs for the frames that
    gained in pass 2 and finds nothing, so pass 4 does not run and their counts are carried into its stages; the noise and
    the single-signal frame stop after pass 1.  Every frame alone as well: there the pass loop itself leaves early."""
    import rtlsdr_ft8d_amd as ft8
    b = _deep_batch(oracle)
    iq = b[[2, 7, 10, 1, 3, 0]]
    B = len(iq)
    searches = {}
    want, wn, wnbs = so.decode_deep(oracle, iq, 4, 2, RECOMMENDED, msgs=_filled_msgs(B), searches=searches)
    print("n_by_stage", wnbs.tolist())
    after = wnbs[:, :, 1]
    assert ((after[:, 1] > after[:, 0]) & (after[:, 3] == after[:, 1])).sum() >= 3, "no frame on which pass 3 finds nothing"
    assert (after[:, 3] == after[:, 0]).any()                          # and one the second pass never runs for
    with ft8.Decoder(device=0, max_frames=B) as dec:
        _deep_both_forms(ft8, dec, iq, 4, 2, RECOMMENDED, want, wn, wnbs, "batch")
        for f in range(B):
            got, n, nbs = dec.decode_messages_deep(iq[f:f + 1], 4, 2, RECOMMENDED, _filled_msgs(1))
            assert n[0] == wn[f] and np.array_equal(nbs[0], wnbs[f]) and got.tobytes() == want[f:f + 1].tobytes(), f


def test_cap_growth_on_a_live_context(oracle):
    """one context: an OSD call and a deep call at cap 33, ft8gpu_set_params to 480 (the OSD records and the later passes'
    candidate set are allocated anew), the same calls, back to 33, the same calls -- each time byte for byte what a fresh
    context created at that cap gives"""
    import rtlsdr_ft8d_amd as ft8
    iq = _edge_frames(oracle)
    B = len(iq)
    mag = oracle.waterfall_batch(iq, nthreads=4)

    def calls(dec, cap):
        cands, counts = oracle.find_sync_batch(mag, cap, 0, nthreads=4)
        assert (counts == cap).all()
        status = dec.decode_candidates(mag, cands, counts)
        fill_st = np.full((B, cap, 48), FILL, np.uint8)
        fill_info = np.full((B, cap * 8), FILL, np.uint8).view(so.INFO_DTYPE).reshape(B, cap)
        st, info = dec.osd_candidates(mag, cands, counts, status, 2, RECOMMENDED, status_out=fill_st, info=fill_info)
        msgs, n, nbs = dec.decode_messages_deep(iq, 2, 2, RECOMMENDED, _filled_msgs(B))
        assert (info["result"] != 0).sum() > B * cap // 2 and n.sum() >= 20
        return [a.tobytes() for a in (status, st, info, msgs, n, nbs)]

    fresh = {}
    for cap in (33, 480):
        with ft8.Decoder(device=0, max_frames=B, max_candidates=cap, min_score=0) as dec:
            fresh[cap] = calls(dec, cap)
    assert fresh[33] != fresh[480]
    with ft8.Decoder(device=0, max_frames=B, max_candidates=33, min_score=0) as dec:
        for cap in (33, 480, 33, 480):
            dec.set_params(max_candidates=cap)
            got = calls(dec, cap)
            assert [a == b for a, b in zip(got, fresh[cap])] == [True] * 6, cap
