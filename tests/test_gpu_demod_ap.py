"""GPU tests of a-priori decoding on the soft bits demodulated from the I/Q samples (ft8gpu_demod_soft,
ft8gpu_ap_soft_candidates, ft8gpu_decode_messages_demod_ap) against the restatement tests/ft8_spec_apsoft.py, byte for byte:
the radio frames of tests/test_gpu_demod.py through ft8gpu_demod_soft under every mask and max_per_frame edge, host, device and
in-place forms, each on a context of two frames (every call chunked) and the device forms on one chunk too; the constructed rows of tests/apsoft_craft.py straight into
ft8gpu_ap_soft_candidates under every hypothesis table and gate of tests/ap_craft.py, with and without the IEEE division, at
ldpc_iters 1, 5 and 50 and on lists of 7 and 70 candidates; the whole path on the radio frames and on eight frames of one station
at -21 dB; the product paths' records before and after; empty calls and refused arguments.  tests/test_demod_ap_cpu.py proves on
the CPU that the constructed rows are what they are named for."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import ap_craft as ac
import apsoft_craft as xc
import demod_craft as dc
import ft8_spec_ap as sa
import ft8_spec_apsoft as sx
import ft8_spec_demod as sdm
import ft8_spec_messages as sm

pytestmark = pytest.mark.gpu
GUARD, FILL, CAP = 256, dc.FILL, dc.CAP
ROW_BYTES = 3 * sx.STRIDE * 4
assert CAP == 24 == xc.CAP and FILL == xc.FILL


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


def filled(shape_bytes, dtype, shape):
    a = np.full(shape_bytes, FILL, np.uint8).view(dtype).reshape(shape)
    a.setflags(write=False)
    return a


# ---- ft8gpu_demod_soft on radio frames ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def radio(oracle):
    """5 frames of 6 off-grid signals near BP's threshold (tests/demod_craft.py) and the oracle's stages for them"""
    import rtlsdr_ft8d_amd as ft8
    iq, planted = dc.radio(ft8, oracle)
    stages = sm.oracle_stages(oracle, iq, CAP, 10, 4, 20)
    B = len(iq)
    d = dict(iq=iq, planted=planted, stages=stages, cache={}, fill_st=filled((B, CAP * 48), ft8.STATUS_DTYPE, (B, CAP)),
             fill_info=filled((B, CAP * 16), sdm.INFO_DTYPE, (B, CAP)), fill_soft=filled((B, CAP * ROW_BYTES), np.float32, (B, CAP, 3, sx.STRIDE)),
             msgs0=filled((B, 50 * 64), ft8.MESSAGE_DTYPE, (B, 50)))
    iq.setflags(write=False)
    return d


SOFT_CASES = [(s, CAP, None) for s in range(1, 8)] + [(7, 0, None), (7, 1, None), (5, 3, None), (7, CAP, (3, 0, 24, 1, 9))]


def test_demod_soft_equals_demod_candidates_and_the_restatement(radio, oracle):
    """status_out and info are those of ft8gpu_demod_candidates, soft is the restatement's; host form (three chunks), device form
    between guard bands, in place; 0xA5 stays behind the counts and in the guard bands of all three arrays"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    d = radio
    _mag, cands, counts0, status = d["stages"]
    status = np.ascontiguousarray(status).view(ft8.STATUS_DTYPE).reshape(len(counts0), CAP)
    B = len(counts0)
    written = 0
    with ft8.Decoder(device=0, max_frames=2, max_candidates=CAP) as dec, ft8.Decoder(device=0, max_frames=B, max_candidates=CAP) as big:
        for sets, mpf, cnt in SOFT_CASES:
            counts = counts0 if cnt is None else np.minimum(np.array(cnt, np.int32), counts0)
            want_st, want_info, want_soft = sx.demod_soft(oracle, d["iq"], cands, counts, status, sets, 174, mpf, status_out=d["fill_st"],
                                                          info=d["fill_info"], soft=d["fill_soft"], bp=oracle.bp_decode, cache=d["cache"])
            want_in, _i, _s = sx.demod_soft(oracle, d["iq"], cands, counts, status, sets, 174, mpf, status_out=status, info=d["fill_info"],
                                            soft=d["fill_soft"], bp=oracle.bp_decode, cache=d["cache"])
            ref_st, ref_info = dec.demod_candidates(d["iq"], cands, counts, status, sets, 174, mpf, status_out=d["fill_st"], info=d["fill_info"])
            st, info, soft = dec.demod_soft(d["iq"], cands, counts, status, sets, 174, mpf, status_out=d["fill_st"], info=d["fill_info"],
                                            soft=d["fill_soft"])
            assert st.tobytes() == ref_st.tobytes() == want_st.tobytes() and info.tobytes() == ref_info.tobytes() == want_info.tobytes()
            for f in range(B):
                for i in range(CAP):
                    assert soft[f, i].tobytes() == want_soft[f, i].tobytes(), (sets, mpf, f, i, "host")
            behind = np.arange(CAP)[None, :] >= counts[:, None]
            assert (soft.view(np.uint8).reshape(B, CAP, ROW_BYTES)[behind] == FILL).all()
            written += int((np.abs(want_soft[~behind]).max(axis=-1) > 0).sum())
            for in_place, on in ((False, big), (True, big), (False, dec), (True, dec)):     # one chunk, and three chunks of two frames
                ins = [up(a) for a in (d["iq"], cands, counts, status)]
                out_b, info_b, soft_b = guarded(status if in_place else d["fill_st"]), guarded(d["fill_info"]), guarded(d["fill_soft"])
                torch.cuda.synchronize()
                on.demod_soft_dev(ins[0], ins[1], ins[2], out_b[GUARD:] if in_place else ins[3], B, sets, 174, mpf, out_b[GUARD:],
                                  info_b[GUARD:], soft_b[GUARD:])
                on.synchronize()
                for a, b in zip((d["iq"], cands, counts) + (() if in_place else (status,)), ins):
                    assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()              # inputs are inputs
                assert unguard(out_b, want_st.nbytes).tobytes() == (want_in if in_place else want_st).tobytes(), (sets, mpf, in_place)
                assert unguard(info_b, want_info.nbytes).tobytes() == want_info.tobytes(), (sets, mpf, in_place)
                assert unguard(soft_b, want_soft.nbytes).tobytes() == want_soft.tobytes(), (sets, mpf, in_place)
    assert written >= 100, "the frames leave rows to write"


# ---- ft8gpu_ap_soft_candidates on constructed rows ------------------------------------------------------------------------------------

CRAFTED = {}


def crafted(oracle, cap=CAP, counts=None):
    import rtlsdr_ft8d_amd as ft8
    if cap not in CRAFTED:
        soft, cnt, status, where = xc.build(ft8, oracle, cap, counts)
        B = len(cnt)
        CRAFTED[cap] = dict(soft=soft, counts=cnt, status=status, where=where, fill_st=filled((B, cap * 48), ft8.STATUS_DTYPE, (B, cap)),
                            fill_info=filled((B, cap * 20), sx.INFO_DTYPE, (B, cap)))
    return CRAFTED[cap]


def ap_soft_three_forms(oracle, dec_host, dec_dev, d, sets, hyps, gate, iters=20):
    """host form (chunked on dec_host), device form between guard bands, device form in place, against the restatement -> its info"""
    import torch
    B, cap = d["status"].shape
    want_st, want_info = sx.ap_soft_candidates(oracle, d["soft"], d["counts"], d["status"], sets, hyps, gate, status_out=d["fill_st"],
                                               info=d["fill_info"], iters=iters)
    want_in, _ = sx.ap_soft_candidates(oracle, d["soft"], d["counts"], d["status"], sets, hyps, gate, status_out=d["status"],
                                       info=d["fill_info"], iters=iters)
    assert dec_host.max_frames < B <= dec_dev.max_frames
    st, info = dec_host.ap_soft_candidates(d["soft"], d["counts"], d["status"], sets, hyps, gate, status_out=d["fill_st"], info=d["fill_info"])
    for f in range(B):
        for i in range(cap):
            assert info[f, i].tobytes() == want_info[f, i].tobytes(), (sets, gate, f, i, info[f, i], want_info[f, i])
            assert st[f, i].tobytes() == want_st[f, i].tobytes(), (sets, gate, f, i, "host")
    for in_place, on in ((False, dec_dev), (True, dec_dev), (False, dec_host), (True, dec_host)):        # one chunk, and chunked
        ins = [up(a) for a in (d["soft"], d["counts"], d["status"])]
        out_b, info_b = guarded(d["status"] if in_place else d["fill_st"]), guarded(d["fill_info"])
        torch.cuda.synchronize()
        on.ap_soft_candidates_dev(ins[0], ins[1], out_b[GUARD:] if in_place else ins[2], B, sets, hyps, gate, out_b[GUARD:], info_b[GUARD:])
        on.synchronize()
        for a, b in zip((d["soft"], d["counts"]) + (() if in_place else (d["status"],)), ins):
            assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()                      # inputs are inputs
        assert unguard(out_b, want_st.nbytes).tobytes() == (want_in if in_place else want_st).tobytes(), (sets, gate, in_place)
        assert unguard(info_b, want_info.nbytes).tobytes() == want_info.tobytes(), (sets, gate, in_place)
    return want_info


@pytest.mark.parametrize("ieee", [False, True])
def test_ap_soft_equals_the_restatement_on_constructed_rows(oracle, ieee):
    """every hypothesis table (1, 2 and 4 hypotheses) and gate of tests/ap_craft.py, then every mask under "CQ ? ?"; counts 22, 0, 3, cap
    and 17; which division ran never shows"""
    import rtlsdr_ft8d_amd as ft8
    d = crafted(oracle)
    w = d["where"]
    cases = ac.build_cases(oracle)
    seen, nhyps = set(), set()
    with ft8.Decoder(device=0, max_frames=5, max_candidates=CAP) as dec, ft8.Decoder(device=0, max_frames=2, max_candidates=CAP) as dec2:
        for k in (dec, dec2):
            k.set_debug_flags(ft8.DBG_FORCE_IEEE_DIV if ieee else 0)
        for name, hyps, gate in ac.configs(cases):
            info = ap_soft_three_forms(oracle, dec2, dec, d, 7, ac.hyps_array(hyps), gate)
            nhyps.add(len(hyps))
            seen |= set(int(r) for f in range(len(d["counts"])) for r in info[f, :d["counts"][f]]["result"])
            if name == "cq":
                assert [int(info[w[n]]["set"]) for n in ("set1", "set2", "set3", "zero_between", "unusable")] == [1, 2, 3, 3, 0]
            if name == "four":
                assert (info[w["dx"]]["result"], info[w["dx"]]["hyp"]) == (1, 2)
        for sets in range(1, 7):
            ap_soft_three_forms(oracle, dec2, dec, d, sets, ac.hyps_array([sa.cq_hypothesis()]), 174)
    assert {0, 1, 2, 3, 4, 6, 7, 8} <= seen and 5 not in seen and {1, 4} <= nhyps


@pytest.mark.parametrize("ieee", [False, True])
@pytest.mark.parametrize("cap", [70, 7])
def test_ap_soft_on_long_and_short_lists(oracle, cap, ieee):
    """max_candidates = 70: 18 workgroups per frame, the last with two waves; 7: two workgroups, the second with three"""
    import rtlsdr_ft8d_amd as ft8
    d = crafted(oracle, cap, {70: (70, 66, 1), 7: (7, 5, 0)}[cap])
    cases = ac.build_cases(oracle)
    cfg = {name: (hyps, gate) for name, hyps, gate in ac.configs(cases)}
    with ft8.Decoder(device=0, max_frames=3, max_candidates=cap) as dec, ft8.Decoder(device=0, max_frames=2, max_candidates=cap) as dec2:
        for k in (dec, dec2):
            k.set_debug_flags(ft8.DBG_FORCE_IEEE_DIV if ieee else 0)
        for name in ("cq", "four"):
            info = ap_soft_three_forms(oracle, dec2, dec, d, 7, ac.hyps_array(cfg[name][0]), cfg[name][1])
            assert (info[0, :cap]["result"] == 1).sum() >= 3


@pytest.mark.parametrize("ieee", [False, True])
@pytest.mark.parametrize("iters", [1, 5, 50])
def test_ap_soft_runs_the_context_s_ldpc_iters(oracle, iters, ieee):
    import rtlsdr_ft8d_amd as ft8
    d = crafted(oracle)
    with ft8.Decoder(device=0, max_frames=5, max_candidates=CAP, ldpc_iters=iters) as dec, \
            ft8.Decoder(device=0, max_frames=2, max_candidates=CAP, ldpc_iters=iters) as dec2:
        for k in (dec, dec2):
            k.set_debug_flags(ft8.DBG_FORCE_IEEE_DIV if ieee else 0)
        info = ap_soft_three_forms(oracle, dec2, dec, d, 7, ac.hyps_array([sa.cq_hypothesis(), sa.from_text("CQ DX ? ?")]), 174, iters=iters)
    results = set(int(r) for r in info[0, :d["counts"][0]]["result"])
    assert 7 in results and (iters == 1 or 1 in results) and int(info[0, :d["counts"][0]]["iters"].max()) <= iters


# ---- the whole path ------------------------------------------------------------------------------------------------------------------

SEEDED = (3301, 3303, 3306, 3317, 3322, 3330, 3300, 3309)     # of the snr-21 row: the demodulation gains on some, AP on 3303, 3322, 3330


@pytest.fixture(scope="module")
def seeded(oracle):
    import rtlsdr_ft8d_amd as ft8
    import synth_util as S
    enc = S.oracle_encode_fn(oracle)
    fr = [S.make_frame(s, 1, enc, snr_range=(-21.0, -21.0)) for s in SEEDED]
    iq = np.ascontiguousarray(np.stack([f[0] for f in fr]), np.float32)
    B = len(iq)
    return dict(iq=iq, planted=[f[1] for f in fr], stages=sm.oracle_stages(oracle, iq, CAP, 10, 4, 20), cache={},
                msgs0=filled((B, 50 * 64), ft8.MESSAGE_DTYPE, (B, 50)))


def whole_path(oracle, d, form):
    """the entry on a context of two frames against the restatement, and the nhyp = 0 identity -> (records, counts, n_by_stage)"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, msgs0 = d["iq"], d["msgs0"]
    B = len(iq)
    hyps = [sa.from_text("CQ ? ?")]
    if "want" not in d:
        d["want"] = sx.decode_demod_ap(oracle, iq, sdm.SETS, 174, None, hyps, sx.MAX_HARD_ERRORS, msgs=msgs0, max_candidates=CAP,
                                       stages=d["stages"], bp=oracle.bp_decode, cache=d["cache"])
    want_m, want_n, want_nbs = d["want"]
    with ft8.Decoder(device=0, max_frames=2, max_candidates=CAP) as dec:
        if form == "host":
            got_m, got_n, got_nbs = dec.decode_messages_demod_ap(iq, msgs=msgs0.copy())
            none_m, none_n, none_nbs = dec.decode_messages_demod_ap(iq, hyps=(), msgs=msgs0.copy())
            ref_m, ref_n, ref_nbs = dec.decode_messages_demod(iq, msgs=msgs0.copy())
        else:
            out = []
            for h in (hyps, ()):
                iq_d, m_b, n_b, s_b = up(iq), guarded(msgs0), guarded(np.zeros(B, np.int32)), guarded(np.zeros((B, 3), np.int32))
                torch.cuda.synchronize()
                dec.decode_messages_demod_ap_dev(iq_d, B, sdm.SETS, 174, CAP, h, sx.MAX_HARD_ERRORS, m_b[GUARD:], n_b[GUARD:], s_b[GUARD:])
                dec.synchronize()
                assert iq_d.cpu().numpy().tobytes() == iq.tobytes()
                out.append((unguard(m_b, msgs0.nbytes).view(ft8.MESSAGE_DTYPE).reshape(B, 50), unguard(n_b, 4 * B).view(np.int32),
                            unguard(s_b, 12 * B).view(np.int32).reshape(B, 3)))
            (got_m, got_n, got_nbs), (none_m, none_n, none_nbs) = out
            ref_m, ref_n, ref_nbs = dec.decode_messages_demod(iq, msgs=msgs0.copy())
    assert (got_n == want_n).all() and (got_nbs == want_nbs).all(), (got_nbs, want_nbs)
    for f in range(B):
        for r in range(50):
            assert got_m[f, r].tobytes() == want_m[f, r].tobytes(), (f, r, got_m[f, r], want_m[f, r])
    behind = np.arange(50)[None, :] >= got_n[:, None]
    assert (got_m.view(np.uint8).reshape(B, 50, 64)[behind] == FILL).all()
    assert none_m.tobytes() == ref_m.tobytes() and (none_n == ref_n).all() and (none_nbs[:, :2] == ref_nbs).all()
    assert (none_nbs[:, 2] == none_nbs[:, 1]).all() and (got_nbs[:, :2] == ref_nbs).all()
    return got_m, got_n, got_nbs


@pytest.mark.parametrize("form", ["host", "device"])
def test_whole_path_on_radio_frames(radio, oracle, form):
    m, n, nbs = whole_path(oracle, radio, form)
    assert int((nbs[:, 2] - nbs[:, 1]).sum()) >= 1 and int((nbs[:, 1] - nbs[:, 0]).sum()) >= 1
    for f in range(len(n)):
        for r in range(int(nbs[f, 1]), int(n[f])):
            assert m[f, r]["pad"][1] == 1 and 1 <= m[f, r]["pad"][3] <= 3 and m[f, r]["text"].decode() in radio["planted"][f]


@pytest.mark.parametrize("form", ["host", "device"])
def test_whole_path_on_one_station_at_minus_21_db(seeded, oracle, form):
    m, n, nbs = whole_path(oracle, seeded, form)
    assert (nbs[:, 0] == 0).all() and int(nbs[:, 1].sum()) >= 3 and int((nbs[:, 2] - nbs[:, 1]).sum()) >= 3
    for f in range(len(n)):
        for r in range(int(n[f])):
            assert m[f, r]["text"].decode() in seeded["planted"][f]
        for r in range(int(nbs[f, 1]), int(n[f])):
            assert m[f, r]["pad"][1] == 1 and 1 <= m[f, r]["pad"][3] <= 3


def test_product_records_are_unchanged_by_the_new_entries():
    """ft8gpu_decode_batch, ft8gpu_decode_messages and ft8gpu_decode_messages_demod on 64 frames, before and after calls of the three
    new entries on the same context, the stage entries in device and in host form (which agree)"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B, S = 64, 20
    _texts, tones = workload.message_pool()
    sig, _picks = workload.frame_signals(0, B, S, tones, snr_range=(-18.0, 0.0))

    def digest(dec, iq):
        spots = torch.zeros((B, 50 * 28), dtype=torch.uint8, device="cuda")
        nres = torch.zeros((B,), dtype=torch.int32, device="cuda")
        msgs, m2 = (torch.zeros((B, 50 * 64), dtype=torch.uint8, device="cuda") for _ in range(2))
        nm, n2 = (torch.zeros((B,), dtype=torch.int32, device="cuda") for _ in range(2))
        nbs = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_batch_dev(iq, B, spots, nres)
        dec.decode_messages_dev(iq, B, msgs, nm)
        dec.decode_messages_demod_dev(iq, B, sdm.SETS, sdm.MAX_HARD_ERRORS, 16, m2, n2, nbs)
        dec.synchronize()
        h = hashlib.sha256()
        for t in (spots, nres, msgs, nm, m2, n2, nbs):
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest(), m2, n2, nbs

    with ft8.Decoder(device=0, max_frames=B) as dec:
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, S, 1.0, workload.SEED_BASE, iq, first_frame=0)
        dec.synchronize()
        before, m2, n2, nbs = digest(dec, iq)
        m3, n3 = torch.zeros_like(m2), torch.zeros_like(n2)
        nbs3 = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_messages_demod_ap_dev(iq, B, sdm.SETS, sdm.MAX_HARD_ERRORS, 16, ["CQ ? ?"], sx.MAX_HARD_ERRORS, m3, n3, nbs3)
        dec.synchronize()
        # the two stage entries, device form on the whole batch and host form on its first frames (the context's staging buffers)
        CAPB = dec.max_candidates
        u8 = lambda k: torch.zeros((k,), dtype=torch.uint8, device="cuda")
        mag, cands, status, counts = u8(B * ft8.MAG_ARRAY), u8(B * CAPB * 8), u8(B * CAPB * 48), torch.zeros((B,), dtype=torch.int32, device="cuda")
        st2, inf, st3, ainf = u8(B * CAPB * 48), u8(B * CAPB * 16), u8(B * CAPB * 48), u8(B * CAPB * 20)
        soft = torch.zeros((B * CAPB * 3 * sx.STRIDE,), dtype=torch.float32, device="cuda")
        dec.waterfall_dev(iq, B, mag)
        dec.find_sync_dev(mag, B, cands, counts)
        dec.decode_candidates_dev(mag, cands, counts, B, status)
        dec.demod_soft_dev(iq, cands, counts, status, B, sdm.SETS, sdm.MAX_HARD_ERRORS, 16, st2, inf, soft)
        dec.ap_soft_candidates_dev(soft, counts, st2, B, sdm.SETS, ["CQ ? ?"], sx.MAX_HARD_ERRORS, st3, ainf)
        dec.synchronize()
        H = 3
        h_iq, h_counts = iq[:H].cpu().numpy(), counts[:H].cpu().numpy()
        h_cands = cands.cpu().numpy().view(ft8.CAND_DTYPE).reshape(B, CAPB)[:H]
        h_status = status.cpu().numpy().view(ft8.STATUS_DTYPE).reshape(B, CAPB)[:H]
        g_st, g_inf, g_soft = dec.demod_soft(h_iq, h_cands, h_counts, h_status, sdm.SETS, sdm.MAX_HARD_ERRORS, 16)
        assert g_st.tobytes() == st2.cpu().numpy()[:H * CAPB * 48].tobytes() and g_soft.tobytes() == soft.cpu().numpy()[:H * CAPB * 3 * sx.STRIDE].tobytes()
        g_st3, g_ainf = dec.ap_soft_candidates(g_soft, h_counts, g_st, sdm.SETS, ["CQ ? ?"], sx.MAX_HARD_ERRORS)
        assert g_st3.tobytes() == st3.cpu().numpy()[:H * CAPB * 48].tobytes() and g_ainf.tobytes() == ainf.cpu().numpy()[:H * CAPB * 20].tobytes()
        assert g_inf.tobytes() == inf.cpu().numpy()[:H * CAPB * 16].tobytes()
        h2, h3, hb2, hb3 = n2.cpu().numpy(), n3.cpu().numpy(), nbs.cpu().numpy(), nbs3.cpu().numpy()
        assert (hb3[:, :2] == hb2).all() and (hb3[:, 2] == h3).all() and (h3 >= h2).all()
        a, b = m2.cpu().numpy().reshape(B, 50, 64), m3.cpu().numpy().reshape(B, 50, 64)
        for f in range(B):
            assert a[f, :h2[f]].tobytes() == b[f, :h2[f]].tobytes()
        after, _m, _n, _b = digest(dec, iq)
    assert before == after


# ---- empty calls and refused arguments ------------------------------------------------------------------------------------------------

def test_empty_calls_and_refused_arguments():
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = np.zeros((1, 2, ft8.NSAMPLES), np.float32)
    cands = np.zeros((1, CAP), ft8.CAND_DTYPE)
    counts = np.zeros(1, np.int32)
    status = np.zeros((1, CAP), ft8.STATUS_DTYPE)
    soft = np.zeros((1, CAP, 3, sx.STRIDE), np.float32)
    info = np.zeros((1, CAP), sx.INFO_DTYPE)
    cq = ac.hyps_array([sa.cq_hypothesis()])
    with ft8.Decoder(device=0, max_frames=2, max_candidates=CAP) as dec:
        L = dec.lib

        def refused(rc, word):
            assert rc == -1 and word in L.ft8gpu_last_error(), (rc, L.ft8gpu_last_error())

        st, inf, sf = dec.demod_soft(iq[:0], cands[:0], counts[:0], status[:0])
        assert st.shape == (0, CAP) and inf.shape == (0, CAP) and sf.shape == (0, CAP, 3, sx.STRIDE)
        st, inf = dec.ap_soft_candidates(soft[:0], counts[:0], status[:0])
        assert st.shape == (0, CAP) and inf.shape == (0, CAP)
        m, n, nbs = dec.decode_messages_demod_ap(iq[:0])
        assert m.shape == (0, 50) and n.shape == (0,) and nbs.shape == (0, 3)
        fill = np.full((1, CAP * ROW_BYTES), FILL, np.uint8).view(np.float32)
        st, inf, sf = dec.demod_soft(iq, cands, counts, status, status_out=np.full((1, CAP * 48), FILL, np.uint8),
                                     info=np.full((1, CAP * 16), FILL, np.uint8), soft=fill)
        assert all((a.view(np.uint8) == FILL).all() for a in (st, inf, sf))                # counts of 0: nothing is written
        st, inf = dec.ap_soft_candidates(fill, counts, status, status_out=np.full((1, CAP * 48), FILL, np.uint8),
                                         info=np.full((1, CAP * 20), FILL, np.uint8))
        assert (st.view(np.uint8) == FILL).all() and (inf.view(np.uint8) == FILL).all()
        p = ft8.DemodParams(7, 174, CAP)
        host = (dec.h, iq.ctypes.data, cands.ctypes.data, counts.ctypes.data, status.ctypes.data, 1, C.byref(p), status.ctypes.data,
                np.zeros((1, CAP), sdm.INFO_DTYPE).ctypes.data)
        refused(L.ft8gpu_demod_soft(*host, None, ft8.HOST_PTRS), b"NULL")                  # a NULL soft
        dev = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        base = dev.data_ptr()
        assert base % 16 == 0
        refused(L.ft8gpu_demod_soft(dec.h, base, base, base, base, 1, C.byref(p), base, base, base + 4, ft8.DEVICE_PTRS), b"soft must be 16-byte aligned")
        ap = (counts.ctypes.data, status.ctypes.data, 1)
        tail = (status.ctypes.data, info.ctypes.data, ft8.HOST_PTRS)
        refused(L.ft8gpu_ap_soft_candidates(dec.h, None, *ap, 7, cq.ctypes.data, 1, 40, *tail), b"NULL")
        refused(L.ft8gpu_ap_soft_candidates(dec.h, base + 8, base, base, 1, 7, cq.ctypes.data, 1, 40, base, base, ft8.DEVICE_PTRS),
                b"soft must be 16-byte aligned")
        for sets in (0, 8):
            refused(L.ft8gpu_ap_soft_candidates(dec.h, soft.ctypes.data, *ap, sets, cq.ctypes.data, 1, 40, *tail), b"sets %d out of range [1, 7]" % sets)
            with pytest.raises(ft8.Ft8GpuError, match="sets"):
                dec.demod_soft(iq, cands, counts, status, sets=sets)
            with pytest.raises(ft8.Ft8GpuError, match="sets"):
                dec.decode_messages_demod_ap(iq, sets=sets)
        for nhyp in (0, 5):
            refused(L.ft8gpu_ap_soft_candidates(dec.h, soft.ctypes.data, *ap, 7, np.zeros(5, sa.HYP_DTYPE).ctypes.data, nhyp, 40, *tail),
                    b"nhyp %d out of range [1, 4]" % nhyp)
        refused(L.ft8gpu_ap_soft_candidates(dec.h, soft.ctypes.data, *ap, 7, cq.ctypes.data, 1, 175, *tail), b"max_hard_errors 175 out of range [0, 174]")
        refused(L.ft8gpu_ap_soft_candidates(dec.h, soft.ctypes.data, *ap, 7, None, 1, 40, *tail), b"hyps is NULL")
        bad = {}
        for name, edit in (("bits outside its mask", lambda h: h["bits"].__setitem__(5, 0xFF)), ("past the 77 payload bits", lambda h: h["mask"].__setitem__(9, 0xFF)),
                           ("masks no bit", lambda h: (h["mask"].fill(0), h["bits"].fill(0)))):
            h = ac.hyps_array([sa.cq_hypothesis(), sa.cq_hypothesis()])
            edit(h[1])
            bad[name] = h
        for name, h in bad.items():
            refused(L.ft8gpu_ap_soft_candidates(dec.h, soft.ctypes.data, *ap, 7, h.ctypes.data, 2, 40, *tail), b"hypothesis 1")
            text = L.ft8gpu_last_error()
            assert name.encode() in text
            mag = np.zeros((1, ft8.MAG_ARRAY), np.uint8)
            a = np.zeros((1, CAP), sa.INFO_DTYPE)
            assert L.ft8gpu_ap_candidates(dec.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status.ctypes.data, 1, h.ctypes.data, 2,
                                          40, status.ctypes.data, a.ctypes.data, ft8.HOST_PTRS) == -1
            assert L.ft8gpu_last_error() == text                                           # ft8gpu_ap_candidates refuses it with the same text
            with pytest.raises(ft8.Ft8GpuError, match="hypothesis 1"):
                dec.decode_messages_demod_ap(iq, hyps=list(h))
        with pytest.raises(ft8.Ft8GpuError, match="nhyp 5 out of range"):
            dec.decode_messages_demod_ap(iq, hyps=[sa.cq_hypothesis()] * 5)
        with pytest.raises(ft8.Ft8GpuError, match="max_hard_errors 175"):
            dec.decode_messages_demod_ap(iq, ap_max_hard_errors=175)
        q = ft8.DemodApParams(ft8.DemodParams(7, 174, CAP), 0, 0)
        refused(L.ft8gpu_decode_messages_demod_ap(dec.h, iq.ctypes.data, 1, None, status.ctypes.data, counts.ctypes.data, None, ft8.HOST_PTRS), b"params")
        refused(L.ft8gpu_decode_messages_demod_ap(dec.h, iq.ctypes.data, 1, C.byref(q), None, counts.ctypes.data, None, ft8.HOST_PTRS), b"NULL")
        refused(L.ft8gpu_decode_messages_demod_ap(dec.h, 8, 1, C.byref(q), 16, 16, None, ft8.DEVICE_PTRS), b"aligned")
