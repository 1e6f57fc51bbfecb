"""GPU tests of the call hints (ft8gpu_hint_candidates, ft8gpu_hint_update, ft8gpu_decode_messages_hinted) against the
restatement tests/ft8_spec_hint.py, byte for byte: the constructed frames frozen in tests/golden/hint_constructed.npz under
every configuration, in the host form (chunked), the device form between guard bands and the device form in place; radio frames
at max_candidates from 1 to 1024 with ragged counts, tables that hold the planted calls among unrelated ones, and on the same
device arrays the identity with ft8gpu_ap_candidates given each candidate's tried hypotheses; the update rule over 1 x 12,
4 x 3 and 12 x 1 cuts of the same records; the whole path on the 3 x 4 stream scenario as one call and as four calls of one
slot, and with an empty table against ft8gpu_decode_messages.  tests/test_hint_cpu.py proves on the CPU that the cases are
what they are named for."""
import numpy as np
import pytest

import ap_craft as ac
import ft8_spec_hint as sh
import hint_craft as hc
import osd_craft as oc

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, hc.FILL
SCENARIO = dict(tries=2, max_bad_per_64=16, max_hard_errors=40)


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def guarded(a):
    """a device copy of a's bytes between two guard bands of FILL"""
    import torch
    b = torch.full((GUARD + a.nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    b[GUARD:GUARD + a.nbytes] = up(a)
    return b


def unguard(b, nbytes):
    h = b.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + nbytes:] == FILL).all(), "a guard band was written"
    return h[GUARD:GUARD + nbytes].copy()


def fills(B, cap):
    return np.full((B, cap, 48), FILL, np.uint8), np.full((B, cap * 16), FILL, np.uint8).view(sh.INFO_DTYPE).reshape(B, cap)


def hint_dev(dec, mag, cands, counts, status_in, states, params, status_out, info, in_place=False):
    """the device form between guard bands -> (status_out bytes, info bytes); the inputs stay as they are"""
    import torch
    B = len(counts)
    ins = [up(a) for a in (mag, cands, counts, status_in, states)]
    out_b, info_b = guarded(np.ascontiguousarray(status_out).view(np.uint8)), guarded(np.ascontiguousarray(info).view(np.uint8))
    torch.cuda.synchronize()
    dec.hint_candidates_dev(ins[0], ins[1], ins[2], out_b[GUARD:] if in_place else ins[3], B, ins[4], *params, out_b[GUARD:], info_b[GUARD:])
    dec.synchronize()
    for a, b in zip((mag, cands, counts, states), (ins[0], ins[1], ins[2], ins[4])):
        assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()          # inputs are inputs, the states read-only
    return unguard(out_b, status_out.nbytes).tobytes(), unguard(info_b, info.nbytes).tobytes()


def first_difference(got_info, want_info, B, cap):
    g = np.frombuffer(got_info, sh.INFO_DTYPE).reshape(B, cap)
    w = np.frombuffer(want_info, sh.INFO_DTYPE).reshape(B, cap)
    bad = np.argwhere((g.view(np.uint64).reshape(B, cap, 2) != w.view(np.uint64).reshape(B, cap, 2)).any(axis=2))
    f, i = (int(x) for x in bad[0])
    return len(bad), (f, i), g[f, i], w[f, i]


# ---- the constructed frames ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    d = hc.load_golden()
    B, cap = d["cands"].shape
    frames = dict(cands=d["cands"], counts=d["counts"], status_in=d["status_in"], vec=d["vec"])
    d["mag"] = oc.waterfalls(d["vectors"], frames)
    d["fill_st"], d["fill_info"] = fills(B, cap)
    behind = np.arange(cap)[None, :] >= d["counts"][:, None]
    assert (d["status_in"][behind] == FILL).all()                      # in place on status_in: FILL behind the counts already
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@pytest.mark.parametrize("form", ["host", "device", "in_place"])
def test_stage_entry_equals_the_frozen_restatement(golden, form):
    """every configuration of the fixture; the host form is chunked by max_frames 5 over the fixture's frames"""
    import rtlsdr_ft8d_amd as ft8
    d = golden
    B, cap = d["cands"].shape
    assert B > 1 and cap == oc.CAP
    cands = d["cands"].view(ft8.CAND_DTYPE).reshape(B, cap)
    below = np.arange(cap)[None, :] < d["counts"][:, None]
    with ft8.Decoder(device=0, max_frames=5 if form == "host" else B, max_candidates=cap, ldpc_iters=hc.ITERS) as dec:
        for k, name in enumerate(d["names"]):
            params = tuple(int(x) for x in d["params"][k])
            states = hc.states_for(d["states"][k], B).view(ft8.HINT_STATE_DTYPE)
            want_in = hc.golden_status(d, k)
            want_info = np.array(d["fill_info"], copy=True)
            want_info[below] = d[f"info_{k}"].view(sh.INFO_DTYPE).reshape(B, cap)[below]
            want_out = np.array(d["fill_st"], copy=True)
            want_out[below] = want_in[below]
            if form == "host":
                st, info = dec.hint_candidates(d["mag"], cands, d["counts"], d["status_in"], states, *params, status_out=d["fill_st"],
                                               info=d["fill_info"])
                got, want = (st.tobytes(), info.tobytes()), (want_out.tobytes(), want_info.tobytes())
            elif form == "device":
                got = hint_dev(dec, d["mag"], cands, d["counts"], d["status_in"], states, params, d["fill_st"], d["fill_info"])
                want = (want_out.tobytes(), want_info.tobytes())
            else:
                got = hint_dev(dec, d["mag"], cands, d["counts"], d["status_in"], states, params, d["status_in"], d["fill_info"], in_place=True)
                want = (want_in.tobytes(), want_info.tobytes())
            assert got[1] == want[1], (name, form, first_difference(got[1], want[1], B, cap))
            assert got[0] == want[0], (name, form)


# ---- radio frames, any max_candidates ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def radio(oracle):
    iq, planted = ac.radio_frames(oracle)
    iq.setflags(write=False)
    return iq, planted


def radio_tables(planted, seed=0x7AB1E, unrelated=236):
    """one table per frame: the frame's planted CQ messages as "? CALL ?" and "CQ CALL ?" and `unrelated` entries of every kind
    from other calls, shuffled over the 512 entries; every seventh entry is old"""
    import synth_util as su
    rng = np.random.default_rng(seed)
    states = sh.new_state(len(planted))
    states["slot"] = 40
    for f, texts in enumerate(planted):
        entries = []
        for k, t in enumerate(texts):
            f1, f2 = hc.fields_of_text(t)
            entries.append((2, 0, f2, 0) if k % 2 else (3, f1, f2, 0))
        while len(entries) < len(texts) + unrelated:
            f1, f2 = hc.fields_of_text(su.random_message(rng, cq=False))
            kind = int(rng.integers(1, 4))
            entries.append((kind, f1 if kind & 1 else 0, f2 if kind & 2 else 0, int(rng.integers(0, 2))))
        for j, (kind, a, b, phase) in zip(rng.permutation(sh.ENTRIES)[:len(entries)], entries):
            hc.put(states[f:f + 1], int(j), kind, a, b, phase, stamp=10 if j % 7 == 0 else 30)
    return states


@pytest.mark.parametrize("cap", [1, 2, 3, 4, 5, 45, 120, 1024])
def test_radio_frames_at_any_max_candidates(oracle, radio, cap):
    """the device's own stages on radio frames, counts made ragged (one frame 0, one full), guard records behind them: the
    host form, the device form and the device form in place against the restatement; at 120 it gains planted messages, and
    the stage's statuses equal ft8gpu_ap_candidates on the same device arrays with each candidate's tried hypotheses"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, planted = radio
    B = 8 if cap <= 120 else 3
    states = radio_tables(planted[:B])
    with ft8.Decoder(device=0, max_frames=B, max_candidates=cap) as dec:
        mag = dec.waterfall(iq[:B])
        cands, counts = dec.find_sync(mag)
        status = dec.decode_candidates(mag, cands, counts)
        counts = np.array(counts, copy=True)
        counts[1] = 0
        for f in range(2, B):
            counts[f] = min(int(counts[f]), max(1, (int(counts[f]) * (f + 1)) // B))
        status_in = np.array(status, copy=True).view(np.uint8).reshape(B, cap, 48)
        status_in[np.arange(cap)[None, :] >= counts[:, None]] = FILL
        fill_st, fill_info = fills(B, cap)
        cache = {}
        for params in ((2, 16, 40, 0, 0), (4, 20, 174, 20, 1)):
            want_st, want_info = sh.hint_candidates(oracle, mag, cands, counts, status_in, states, *params, status_out=fill_st, info=fill_info,
                                                    cache=cache)
            want_in = sh.hint_candidates(oracle, mag, cands, counts, status_in, states, *params, status_out=status_in, cache=cache)[0]
            st, info = dec.hint_candidates(mag, cands, counts, status_in, states.view(ft8.HINT_STATE_DTYPE), *params, status_out=fill_st,
                                           info=fill_info)
            assert info.tobytes() == want_info.tobytes(), (cap, params, "host", first_difference(info.tobytes(), want_info.tobytes(), B, cap))
            assert st.tobytes() == want_st.tobytes(), (cap, params, "host")
            got = hint_dev(dec, mag, cands, counts, status_in, states, params, fill_st, fill_info)
            assert got == (want_st.tobytes(), want_info.tobytes()), (cap, params, "device")
            got = hint_dev(dec, mag, cands, counts, status_in, states, params, status_in, fill_info, in_place=True)
            assert got == (want_in.tobytes(), want_info.tobytes()), (cap, params, "in place")
            if cap != 120:
                continue
            sin, sout = status_in.view(ft8.STATUS_DTYPE).reshape(B, cap), want_st.view(ft8.STATUS_DTYPE).reshape(B, cap)
            gained = tried = 0
            for f in range(B):
                bp = {sin[f, i]["text"] for i in range(counts[f]) if sin[f, i]["ok"]}
                new = {sout[f, i]["text"] for i in range(counts[f]) if want_info[f, i]["result"] == 1}
                gained += len({t for t in new - bp if t.decode() in planted[f]})
                tried += int(want_info[f, :counts[f]]["ntried"].sum())
            print(f"cap 120, params {params}: {gained} planted messages gained over BP, {tried} tries")
            assert gained >= 1
            # ft8gpu_ap_candidates with the tried hypotheses, one frame at a time on the same device arrays
            ins = [up(a) for a in (mag, cands, counts, status_in)]
            for f in range(B):
                groups = {}
                for i in range(int(counts[f])):
                    n = int(want_info[f, i]["ntried"])
                    if n:
                        groups.setdefault(tuple(int(j) for j in want_info[f, i]["index"][:n]), []).append(i)
                fr = [ins[0][f * ft8.MAG_ARRAY:(f + 1) * ft8.MAG_ARRAY], ins[1][f * cap * 8:(f + 1) * cap * 8], ins[2][4 * f:4 * f + 4],
                      ins[3][f * cap * 48:(f + 1) * cap * 48]]
                out_d = torch.empty(cap * 48, dtype=torch.uint8, device="cuda")
                info_d = torch.empty(cap * 8, dtype=torch.uint8, device="cuda")
                for idx, members in groups.items():
                    hyps = [sh.hypothesis(states[f]["entry"][j]) for j in idx]
                    dec.ap_candidates_dev(*fr, 1, hyps, params[2], out_d, info_d)
                    dec.synchronize()
                    ap = out_d.cpu().numpy().reshape(cap, 48)
                    for i in members:
                        assert ap[i].tobytes() == want_st[f, i].tobytes(), (f, i, idx)


# ---- the update rule -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def records():
    msgs, n = hc.records_of(hc.update_layout())
    msgs, n = msgs[0].copy(), n[0].copy()                              # receiver 0's twelve slots: every kind of record
    msgs[7, :45] = hc.records_of(hc.update_layout())[0][1, 7, :45]    # and a full slot of receiver 1's
    n[7] = 45
    msgs.setflags(write=False)
    n.setflags(write=False)
    return msgs, n


def entry_state(R):
    """states that are not reset: a few entries of every kind byte, cursors past 512, used above 1, slots about to wrap"""
    rng = np.random.default_rng(0x57A7E)
    st = sh.new_state(R)
    k1abc, w9xyz = hc.call_field("K1ABC"), hc.call_field("W9XYZ")
    for r in range(R):
        for j in rng.choice(sh.ENTRIES, 40, replace=False):
            hc.put(st[r:r + 1], int(j), int(rng.integers(0, 6)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)),
                   int(rng.integers(0, 256)), used=int(rng.integers(0, 256)), stamp=int(rng.integers(0, 1 << 32)))
        hc.put(st[r:r + 1], 3, 3, k1abc | 0xE0000000, w9xyz, 0xFE | (r & 1), used=9, stamp=5)
        hc.put(st[r:r + 1], 2, 3, k1abc, w9xyz | 0x20000000, r & 1, used=1, stamp=6)
        st[r]["cursor"] = int(rng.integers(0, 1 << 32))
        st[r]["slot"] = 0xFFFFFFFF - r
    return st


@pytest.mark.parametrize("shape", [(1, 12), (4, 3), (12, 1)])
def test_update_rule_over_cuts_of_the_same_records(records, shape):
    """host form through contexts of 2, 5, 8 and 16 frames (runs of slots, whole receivers, everything at once) and the device
    form between guard bands; the records are inputs"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    msgs, n_msgs = records
    R, S = shape
    m, n = msgs.reshape(R, S, 50), n_msgs.reshape(R, S)
    st0 = entry_state(R)
    want = sh.update(m, n, st0)
    assert want.tobytes() != st0.tobytes() and (want["slot"] == ((st0["slot"].astype(np.int64) + S) & 0xFFFFFFFF)).all()
    for mf in (2, 5, 8, 16):
        with ft8.Decoder(device=0, max_frames=mf) as dec:
            got = dec.hint_update(m, n, st0.view(ft8.HINT_STATE_DTYPE))
            assert got.tobytes() == want.tobytes(), (shape, mf)
            if mf == 16:
                md, nd, sd = up(m), up(n), guarded(st0)
                torch.cuda.synchronize()
                dec.hint_update_dev(md, nd, R, S, sd[GUARD:])
                dec.synchronize()
                assert unguard(sd, st0.nbytes).tobytes() == want.tobytes(), (shape, "device")
                assert md.cpu().numpy().tobytes() == m.tobytes() and nd.cpu().numpy().tobytes() == n.tobytes()


# ---- the whole path ----------------------------------------------------------------------------------------------------------------

def filled_msgs(shape):
    import rtlsdr_ft8d_amd as ft8
    return np.full(shape + (64,), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(shape)


@pytest.fixture(scope="module")
def stream(oracle):
    iq, texts = hc.scenario(oracle)
    want = sh.decode_hinted(oracle, iq, max_age=3, use_phase=True, msgs=filled_msgs((3, 4, 50)), **SCENARIO)
    iq.setflags(write=False)
    return iq, texts, want


@pytest.mark.parametrize("max_frames", [3, 5, 16])
def test_whole_path_on_the_stream_scenario(stream, max_frames):
    """msgs, n_msgs, n_by_stage and the exit state of 3 receivers x 4 slots against the restatement: one call, four calls of one
    slot, host and device form; through contexts of 3 frames (runs of slots), 5 (a receiver at a time) and 16 (all at once)"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, texts, (want_msgs, want_n, want_nbs, want_st) = stream
    p = (SCENARIO["tries"], SCENARIO["max_bad_per_64"], SCENARIO["max_hard_errors"])
    assert (want_nbs[:, 2:, 1] > want_nbs[:, 2:, 0]).any()
    with ft8.Decoder(device=0, max_frames=max_frames) as dec:
        msgs, n, nbs, st = dec.decode_messages_hinted(iq, *p, None, 3, True, filled_msgs((3, 4, 50)))
        assert np.array_equal(n, want_n) and np.array_equal(nbs, want_nbs), (n.tolist(), want_n.tolist(), nbs.tolist(), want_nbs.tolist())
        assert msgs.tobytes() == want_msgs.tobytes() and st.tobytes() == want_st.tobytes()
        st1, parts = None, []
        for s in range(4):
            m1, n1, b1, st1 = dec.decode_messages_hinted(np.ascontiguousarray(iq[:, s:s + 1]), *p, st1, 3, True, filled_msgs((3, 1, 50)))
            parts.append((m1, n1, b1))
        assert np.concatenate([q[0] for q in parts], axis=1).tobytes() == want_msgs.tobytes()
        assert np.array_equal(np.concatenate([q[1] for q in parts], axis=1), want_n)
        assert np.array_equal(np.concatenate([q[2] for q in parts], axis=1), want_nbs) and st1.tobytes() == want_st.tobytes()
        if max_frames != 16:
            return
        iq_d = torch.from_numpy(np.array(iq)).cuda()
        for with_nbs in (True, False):
            bufs = [guarded(filled_msgs((3, 4, 50))), guarded(np.full((3, 4), -0x5A5A5A5B, np.int32)),
                    guarded(np.full((3, 4, 2), -0x5A5A5A5B, np.int32)), guarded(sh.new_state(3))]
            torch.cuda.synchronize()
            dec.decode_messages_hinted_dev(iq_d, 3, 4, bufs[3][GUARD:], *p, 3, True, bufs[0][GUARD:], bufs[1][GUARD:],
                                           bufs[2][GUARD:] if with_nbs else None)
            dec.synchronize()
            assert unguard(bufs[0], want_msgs.nbytes).tobytes() == want_msgs.tobytes()
            assert unguard(bufs[1], want_n.nbytes).tobytes() == want_n.tobytes() and unguard(bufs[3], want_st.nbytes).tobytes() == want_st.tobytes()
            assert unguard(bufs[2], want_nbs.nbytes).tobytes() == (want_nbs.tobytes() if with_nbs else np.full((3, 4, 2), -0x5A5A5A5B, np.int32).tobytes())


def test_with_an_empty_table_the_records_are_those_of_decode_messages(stream):
    """slot 0 of every receiver meets a reset table: nothing is gained there, and its records are ft8gpu_decode_messages'; in
    every slot the records below the BP count are"""
    import rtlsdr_ft8d_amd as ft8
    iq, texts, (want_msgs, want_n, want_nbs, want_st) = stream
    p = (SCENARIO["tries"], SCENARIO["max_bad_per_64"], SCENARIO["max_hard_errors"])
    with ft8.Decoder(device=0, max_frames=16) as dec:
        plain, pn = dec.decode_messages(iq.reshape(12, 2, -1), filled_msgs((12, 50)))
        first, n1, nbs1, _st = dec.decode_messages_hinted(np.ascontiguousarray(iq[:, :1]), *p, None, 3, True, filled_msgs((3, 1, 50)))
        assert first.tobytes() == plain.reshape(3, 4, 50)[:, :1].tobytes() and np.array_equal(n1, pn.reshape(3, 4)[:, :1])
        assert np.array_equal(nbs1[:, :, 0], nbs1[:, :, 1])
        msgs, n, nbs, _st = dec.decode_messages_hinted(iq, *p, None, 3, True, filled_msgs((3, 4, 50)))
        assert np.array_equal(pn.reshape(3, 4), nbs[:, :, 0])
        for f in range(12):
            assert plain[f, :pn[f]].tobytes() == msgs.reshape(12, 50)[f, :pn[f]].tobytes()


def test_the_in_wave_form_of_the_ab_build_leaves_the_same_bytes(golden, stream):
    """FT8GPU_AB_HINT_IN_WAVE in the A/B build (no pre-kernel: the 16-byte entries are converted in the wave; tools/bench_hint.py
    times it beside the product's form): every configuration of the fixture in the host form chunked by 5 and in the device form, and
    the whole path on the stream scenario"""
    import rtlsdr_ft8d_amd as ft8
    d = golden
    B, cap = d["cands"].shape
    cands = d["cands"].view(ft8.CAND_DTYPE).reshape(B, cap)
    below = np.arange(cap)[None, :] < d["counts"][:, None]
    lib = ft8.load_ab_library()
    with ft8.Decoder(device=0, max_frames=5, max_candidates=cap, ldpc_iters=hc.ITERS, lib=lib) as dec:
        dec.set_debug_flags(ft8.AB_HINT_IN_WAVE)
        for k, name in enumerate(d["names"]):
            params = tuple(int(x) for x in d["params"][k])
            states = hc.states_for(d["states"][k], B).view(ft8.HINT_STATE_DTYPE)
            want_info = np.array(d["fill_info"], copy=True)
            want_info[below] = d[f"info_{k}"].view(sh.INFO_DTYPE).reshape(B, cap)[below]
            want_out = np.array(d["fill_st"], copy=True)
            want_out[below] = hc.golden_status(d, k)[below]
            st, info = dec.hint_candidates(d["mag"], cands, d["counts"], d["status_in"], states, *params, status_out=d["fill_st"], info=d["fill_info"])
            assert info.tobytes() == want_info.tobytes(), (name, first_difference(info.tobytes(), want_info.tobytes(), B, cap))
            assert st.tobytes() == want_out.tobytes(), name
            if k % 6 == 0:
                got = hint_dev(dec, d["mag"][:5], cands[:5], d["counts"][:5], d["status_in"][:5], states[:5], params, d["fill_st"][:5], d["fill_info"][:5])
                assert got == (want_out[:5].tobytes(), want_info[:5].tobytes()), (name, "device")
    iq, texts, (want_msgs, want_n, want_nbs, want_st) = stream
    p = (SCENARIO["tries"], SCENARIO["max_bad_per_64"], SCENARIO["max_hard_errors"])
    with ft8.Decoder(device=0, max_frames=5, lib=lib) as dec:
        dec.set_debug_flags(ft8.AB_HINT_IN_WAVE)
        msgs, n, nbs, st = dec.decode_messages_hinted(iq, *p, None, 3, True, filled_msgs((3, 4, 50)))
        assert np.array_equal(n, want_n) and np.array_equal(nbs, want_nbs)
        assert msgs.tobytes() == want_msgs.tobytes() and st.tobytes() == want_st.tobytes()


def test_refused_arguments(radio):
    import rtlsdr_ft8d_amd as ft8
    iq, _planted = radio
    with ft8.Decoder(device=0, max_frames=2) as dec:
        mag = dec.waterfall(iq[:1])
        cands, counts = dec.find_sync(mag)
        status = dec.decode_candidates(mag, cands, counts)
        states = ft8.hint_state(1)
        for params, word in (((0, 16, 40), "tries"), ((5, 16, 40), "tries"), ((1, -1, 40), "max_bad_per_64"), ((1, 65, 40), "max_bad_per_64"),
                             ((1, 16, -1), "max_hard_errors"), ((1, 16, 175), "max_hard_errors")):
            with pytest.raises(ft8.Ft8GpuError, match=word):
                dec.hint_candidates(mag, cands, counts, status, states, *params)
            with pytest.raises(ft8.Ft8GpuError, match=word):
                dec.decode_messages_hinted(iq[:1].reshape(1, 1, 2, -1), *params)
        dec.hint_candidates(mag, cands, counts, status, states, 4, 64, 174)
        dec.hint_candidates(mag, cands, counts, status, states, 1, 0, 0)
