"""GPU tests of the expected messages (ft8gpu_match_candidates, ft8gpu_expect_update, ft8gpu_decode_messages_expected)
against the numpy restatement tests/ft8_spec_match.py, byte for byte: the constructed frames frozen in
tests/golden/match_constructed.npz under every configuration, in the host form (chunked), the device form and the device
form in place; radio frames; max_candidates from 1 to 1024 with ragged counts and guard records behind the counts; the update
rule over 1 x 12, 4 x 3 and 12 x 1 cuts of the same records; the whole path on the 3 x 4 stream scenario as one call and as
four calls of one slot.  tests/test_match_cpu.py proves on the CPU that the cases are what they are named for."""
import numpy as np
import pytest

import ap_craft as ac
import callhash_craft as cc
import ft8_spec_match as smt
import match_craft as mc

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, mc.FILL


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


def match_dev(dec, mag, cands, counts, status_in, states, max_age, gate, status_out, info, in_place=False):
    """the device form between guard bands -> (status_out bytes, info bytes); the inputs stay as they are"""
    import torch
    B = len(counts)
    ins = [up(a) for a in (mag, cands, counts, status_in, states)]
    out_b, info_b = guarded(np.ascontiguousarray(status_out).view(np.uint8)), guarded(np.ascontiguousarray(info).view(np.uint8))
    torch.cuda.synchronize()
    dec.match_candidates_dev(ins[0], ins[1], ins[2], out_b[GUARD:] if in_place else ins[3], B, ins[4], max_age, gate, out_b[GUARD:], info_b[GUARD:])
    dec.synchronize()
    for a, b in zip((mag, cands, counts, states), (ins[0], ins[1], ins[2], ins[4])):
        assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()          # inputs are inputs, the states read-only
    return unguard(out_b, status_out.nbytes).tobytes(), unguard(info_b, info.nbytes).tobytes()


# ---- the constructed frames ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    d = mc.load_golden()
    B, cap = d["cands"].shape
    behind = np.arange(cap)[None, :] >= d["counts"][:, None]
    d["fill_st"] = np.full((B, cap, 48), FILL, np.uint8)
    d["fill_info"] = np.full((B, cap * 8), FILL, np.uint8).view(smt.INFO_DTYPE).reshape(B, cap)
    for name, _age, _gate in d["configs"]:
        st = np.array(d["status_" + name], copy=True)          # the fixture is in place on status_in: FILL behind the counts already
        assert (st[behind] == FILL).all()
        d["out_" + name] = st
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@pytest.mark.parametrize("form", ["host", "device", "in_place"])
def test_stage_entry_equals_the_frozen_restatement(golden, form):
    """every configuration (max_age, gate) of the fixture; the host form is chunked by max_frames 5 over 24 frames"""
    import rtlsdr_ft8d_amd as ft8
    d = golden
    B, cap = d["cands"].shape
    cands = d["cands"].view(ft8.CAND_DTYPE).reshape(B, cap)
    states = d["states"].view(ft8.EXPECT_STATE_DTYPE)
    with ft8.Decoder(device=0, max_frames=5 if form == "host" else B, max_candidates=cap) as dec:
        for name, max_age, gate in d["configs"]:
            want_st, want_info = d["out_" + name].tobytes(), d["info_" + name].tobytes()
            if form == "host":
                st, info = dec.match_candidates(d["mag"], cands, d["counts"], d["status_in"], states, max_age, gate,
                                                status_out=d["fill_st"], info=d["fill_info"])
                got_st, got_info = st.tobytes(), info.tobytes()
            elif form == "device":
                got_st, got_info = match_dev(dec, d["mag"], cands, d["counts"], d["status_in"], states, max_age, gate, d["fill_st"], d["fill_info"])
            else:
                got_st, got_info = match_dev(dec, d["mag"], cands, d["counts"], d["status_in"], states, max_age, gate, d["status_in"],
                                             d["fill_info"], in_place=True)
            if got_info != want_info:
                g = np.frombuffer(got_info, smt.INFO_DTYPE).reshape(B, cap)
                bad = np.argwhere(g.view(np.uint64) != d["info_" + name].view(np.uint64))
                names = {v: k for k, v in d["where"].items()}
                f, i = (int(x) for x in bad[0])
                raise AssertionError((name, form, len(bad), names.get((f, i)), g[f, i], d["info_" + name][f, i]))
            assert got_st == want_st, (name, form)


# ---- radio frames, any max_candidates ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def radio(oracle):
    iq, planted = ac.radio_frames(oracle)
    iq.setflags(write=False)
    return iq, planted


def radio_tables(planted, seed=0x7AB1E, unrelated=236):
    import rtlsdr_ft8d_amd as ft8
    rng = np.random.default_rng(seed)
    states = smt.new_state(len(planted))
    for f, texts in enumerate(planted):
        payloads = [ft8.pack77(t) for t in texts] + mc.unrelated_payloads(rng, unrelated, texts)
        for j, p in zip(rng.permutation(smt.ENTRIES)[:len(payloads)], payloads):
            mc.put(states[f], int(j), p)
    return states


@pytest.mark.parametrize("cap", [1, 2, 3, 4, 5, 45, 120, 1024])
def test_radio_frames_at_any_max_candidates(oracle, radio, cap):
    """the device's own stages on radio frames, counts made ragged (one frame 0, one full), guard records behind them: the
    host form, the device form and the device form in place against the restatement; at 120 it gains planted messages"""
    import rtlsdr_ft8d_amd as ft8
    iq, planted = radio
    B = 8 if cap <= 120 else 3
    gate = ft8.MATCH_MAX_HARD_ERRORS
    states = radio_tables(planted[:B])
    states["slot"] = 40
    states["entry"]["stamp"][:, ::7] = 10                             # every seventh entry is expired under max_age 20
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
        fill_st = np.full((B, cap, 48), FILL, np.uint8)
        fill_info = np.full((B, cap * 8), FILL, np.uint8).view(smt.INFO_DTYPE).reshape(B, cap)
        for max_age in (0, 20):
            want_st, want_info = smt.match_candidates(oracle, mag, cands, counts, status_in, states, max_age, gate, status_out=fill_st, info=fill_info)
            want_in = smt.match_candidates(oracle, mag, cands, counts, status_in, states, max_age, gate, status_out=status_in)[0]
            st, info = dec.match_candidates(mag, cands, counts, status_in, states.view(ft8.EXPECT_STATE_DTYPE), max_age, gate,
                                            status_out=fill_st, info=fill_info)
            assert info.tobytes() == want_info.tobytes() and st.tobytes() == want_st.tobytes(), (cap, max_age, "host")
            got = match_dev(dec, mag, cands, counts, status_in, states, max_age, gate, fill_st, fill_info)
            assert got == (want_st.tobytes(), want_info.tobytes()), (cap, max_age, "device")
            got = match_dev(dec, mag, cands, counts, status_in, states, max_age, gate, status_in, fill_info, in_place=True)
            assert got == (want_in.tobytes(), want_info.tobytes()), (cap, max_age, "in place")
            if cap == 120 and max_age == 0:
                sin, sout = status_in.view(ft8.STATUS_DTYPE).reshape(B, cap), want_st.view(ft8.STATUS_DTYPE).reshape(B, cap)
                gained = 0
                for f in range(B):
                    bp = {sin[f, i]["text"] for i in range(counts[f]) if sin[f, i]["ok"]}
                    new = {sout[f, i]["text"] for i in range(counts[f]) if want_info[f, i]["result"] == 1}
                    assert all(t.decode() in planted[f] for t in new)
                    gained += len(new - bp)
                assert gained >= 1


# ---- the update rule -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def records(oracle):
    msgs, n_msgs, _printed = cc.frames(oracle, mc.update_layout(), 0x0DD)
    msgs, n_msgs = msgs.reshape(-1, 50)[:12].copy(), n_msgs.reshape(-1)[:12].copy()
    msgs.setflags(write=False)
    n_msgs.setflags(write=False)
    return msgs, n_msgs


def entry_state(R):
    """states that are not reset: a few entries, cursors past 512, used above 1, slots about to wrap"""
    import rtlsdr_ft8d_amd as ft8
    rng = np.random.default_rng(0x57A7E)
    st = smt.new_state(R)
    for r in range(R):
        for j in rng.choice(smt.ENTRIES, 40, replace=False):
            mc.put(st[r], int(j), mc.random_payload(rng), used=int(rng.integers(1, 256)), kind=int(rng.integers(0, 2)), stamp=int(rng.integers(0, 1 << 32)))
        mc.put(st[r], 3, ft8.pack77("W9XYZ K1ABC RRR"), used=9, kind=1, stamp=5)
        st[r]["cursor"] = int(rng.integers(0, 1 << 32))
        st[r]["slot"] = 0xFFFFFFFF - r
    return st


@pytest.mark.parametrize("derive", [0, 1])
@pytest.mark.parametrize("shape", [(1, 12), (4, 3), (12, 1)])
def test_update_rule_over_cuts_of_the_same_records(records, shape, derive):
    """host form through contexts of 2, 5, 8 and 16 frames (runs of slots, whole receivers -- for shape (4, 3) one, then two per
    piece --, everything at once) and the device form between guard bands; the records are inputs"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    msgs, n_msgs = records
    R, S = shape
    m, n = msgs.reshape(R, S, 50), n_msgs.reshape(R, S)
    st0 = entry_state(R)
    want = smt.update(m, n, st0, bool(derive))
    assert want.tobytes() != st0.tobytes() and (want["slot"] == ((st0["slot"].astype(np.int64) + S) & 0xFFFFFFFF)).all()
    for mf in (2, 5, 8, 16):
        with ft8.Decoder(device=0, max_frames=mf) as dec:
            got = dec.expect_update(m, n, st0.view(ft8.EXPECT_STATE_DTYPE), derive)
            assert got.tobytes() == want.tobytes(), (shape, derive, mf)
            if mf == 16:
                md, nd, sd = up(m), up(n), guarded(st0)
                torch.cuda.synchronize()
                dec.expect_update_dev(md, nd, R, S, sd[GUARD:], derive)
                dec.synchronize()
                assert unguard(sd, st0.nbytes).tobytes() == want.tobytes(), (shape, derive, "device")
                assert md.cpu().numpy().tobytes() == m.tobytes() and nd.cpu().numpy().tobytes() == n.tobytes()


# ---- the whole path ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stream(oracle):
    import rtlsdr_ft8d_amd as ft8
    iq, texts = mc.scenario(oracle)
    want = {d: smt.decode_expected(oracle, iq, max_hard_errors=ft8.MATCH_MAX_HARD_ERRORS, max_age=3, derive=bool(d), msgs=filled_msgs((3, 4, 50)))
            for d in (0, 1)}
    iq.setflags(write=False)
    return iq, texts, want


def filled_msgs(shape):
    import rtlsdr_ft8d_amd as ft8
    return np.full(shape + (64,), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(shape)


@pytest.mark.parametrize("derive", [0, 1])
@pytest.mark.parametrize("max_frames", [3, 5, 8, 16])
def test_whole_path_on_the_stream_scenario(stream, derive, max_frames):
    """msgs, n_msgs, n_by_stage and the exit state of 3 receivers x 4 slots against the restatement: one call, four calls of one
    slot, host and device form; through contexts of 3 frames (runs of slots), 5 (a receiver at a time), 8 (two receivers, then
    one: in the device form a gathered piece, then the caller's arrays directly) and 16 (all at once).
    The records below the BP count are the bytes of ft8gpu_decode_messages."""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, texts, want = stream
    want_msgs, want_n, want_nbs, want_st = want[derive]
    gate = ft8.MATCH_MAX_HARD_ERRORS
    assert (want_nbs[:, 2, 1] > want_nbs[:, 2, 0]).any() and ((want_nbs[:, 3, 1] > want_nbs[:, 3, 0]).any() == bool(derive))
    with ft8.Decoder(device=0, max_frames=max_frames) as dec:
        msgs, n, nbs, st = dec.decode_messages_expected(iq, None, gate, 3, derive, filled_msgs((3, 4, 50)))
        assert np.array_equal(n, want_n) and np.array_equal(nbs, want_nbs)
        assert msgs.tobytes() == want_msgs.tobytes() and st.tobytes() == want_st.tobytes()
        # four calls of one slot
        st1, parts = None, []
        for s in range(4):
            m1, n1, b1, st1 = dec.decode_messages_expected(np.ascontiguousarray(iq[:, s:s + 1]), st1, gate, 3, derive, filled_msgs((3, 1, 50)))
            parts.append((m1, n1, b1))
        assert np.concatenate([p[0] for p in parts], axis=1).tobytes() == want_msgs.tobytes()
        assert np.array_equal(np.concatenate([p[1] for p in parts], axis=1), want_n)
        assert np.array_equal(np.concatenate([p[2] for p in parts], axis=1), want_nbs) and st1.tobytes() == want_st.tobytes()
        if max_frames not in (8, 16):
            return
        # device form between guard bands, n_by_stage present and absent
        iq_d = torch.from_numpy(np.array(iq)).cuda()
        for with_nbs in (True, False):
            bufs = [guarded(filled_msgs((3, 4, 50))), guarded(np.full((3, 4), -0x5A5A5A5B, np.int32)),
                    guarded(np.full((3, 4, 2), -0x5A5A5A5B, np.int32)), guarded(smt.new_state(3))]
            torch.cuda.synchronize()
            dec.decode_messages_expected_dev(iq_d, 3, 4, bufs[3][GUARD:], gate, 3, derive, bufs[0][GUARD:], bufs[1][GUARD:],
                                             bufs[2][GUARD:] if with_nbs else None)
            dec.synchronize()
            assert unguard(bufs[0], want_msgs.nbytes).tobytes() == want_msgs.tobytes()
            assert unguard(bufs[1], want_n.nbytes).tobytes() == want_n.tobytes() and unguard(bufs[3], want_st.nbytes).tobytes() == want_st.tobytes()
            assert unguard(bufs[2], want_nbs.nbytes).tobytes() == (want_nbs.tobytes() if with_nbs else np.full((3, 4, 2), -0x5A5A5A5B, np.int32).tobytes())
        if max_frames != 16:
            return
        # the records below the BP count are those of ft8gpu_decode_messages
        plain, pn = dec.decode_messages(iq.reshape(12, 2, -1), filled_msgs((12, 50)))
        assert np.array_equal(pn.reshape(3, 4), want_nbs[:, :, 0])
        for f in range(12):
            assert plain[f, :pn[f]].tobytes() == msgs.reshape(12, 50)[f, :pn[f]].tobytes()
        # four calls of one slot in the device form (one slot per receiver: no staging), the state carried on the device
        state_d = guarded(smt.new_state(3))
        for s in range(4):
            iq_s = torch.from_numpy(np.ascontiguousarray(iq[:, s])).cuda()
            bufs = [guarded(filled_msgs((3, 1, 50))), guarded(np.full((3, 1), -0x5A5A5A5B, np.int32)), guarded(np.full((3, 1, 2), -0x5A5A5A5B, np.int32))]
            torch.cuda.synchronize()
            dec.decode_messages_expected_dev(iq_s, 3, 1, state_d[GUARD:], gate, 3, derive, bufs[0][GUARD:], bufs[1][GUARD:], bufs[2][GUARD:])
            dec.synchronize()
            assert unguard(bufs[0], want_msgs[:, s].nbytes).tobytes() == want_msgs[:, s].tobytes(), s
            assert unguard(bufs[1], 12).tobytes() == want_n[:, s].tobytes() and unguard(bufs[2], 24).tobytes() == want_nbs[:, s].tobytes(), s
        assert unguard(state_d, want_st.nbytes).tobytes() == want_st.tobytes()
        # one receiver, four slots, in the device form
        bufs = [guarded(filled_msgs((1, 4, 50))), guarded(np.full((1, 4), -0x5A5A5A5B, np.int32)), guarded(smt.new_state(1))]
        torch.cuda.synchronize()
        dec.decode_messages_expected_dev(iq_d[1:2], 1, 4, bufs[2][GUARD:], gate, 3, derive, bufs[0][GUARD:], bufs[1][GUARD:], None)
        dec.synchronize()
        assert unguard(bufs[0], want_msgs[1].nbytes).tobytes() == want_msgs[1].tobytes() and unguard(bufs[1], 16).tobytes() == want_n[1].tobytes()
        assert unguard(bufs[2], want_st[1:2].nbytes).tobytes() == want_st[1:2].tobytes()
        assert iq_d.cpu().numpy().tobytes() == iq.tobytes()


def test_empty_calls_and_refused_arguments(gpu_decoder):
    import rtlsdr_ft8d_amd as ft8
    dec, lib = gpu_decoder, gpu_decoder.lib
    cap = dec.max_candidates
    mag, cands, counts = np.zeros((1, ft8.MAG_ARRAY), np.uint8), np.zeros((1, cap), ft8.CAND_DTYPE), np.zeros(1, np.int32)
    status, info, state = np.zeros((1, cap, 48), np.uint8), np.zeros((1, cap), ft8.MATCH_INFO_DTYPE), ft8.expect_state(1)
    p = lambda a: a.ctypes.data
    margs = lambda n, gate, st=state: (dec.h, p(mag), p(cands), p(counts), p(status), n, p(st) if st is not None else None, 0, gate, p(status), p(info), ft8.HOST_PTRS)
    assert lib.ft8gpu_match_candidates(*margs(0, 45)) == 0 and lib.ft8gpu_match_candidates(*margs(1, 45)) == 0
    for gate in (-1, 175):
        assert lib.ft8gpu_match_candidates(*margs(1, gate)) == -1 and b"max_hard_errors" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_match_candidates(*margs(1, 45, None)) == -1 and b"NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_match_candidates(*margs(-1, 45)) == -1
    msgs, n = np.zeros((1, 1, 50), ft8.MESSAGE_DTYPE), np.zeros((1, 1), np.int32)
    assert lib.ft8gpu_expect_update(dec.h, p(msgs), p(n), 0, 1, p(state), 1, ft8.HOST_PTRS) == 0
    assert lib.ft8gpu_expect_update(dec.h, p(msgs), p(n), 1, 0, p(state), 1, ft8.HOST_PTRS) == 0 and state.tobytes() == ft8.expect_state(1).tobytes()
    assert lib.ft8gpu_expect_update(dec.h, p(msgs), p(n), -1, 1, p(state), 1, ft8.HOST_PTRS) == -1 and b"negative" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_expect_update(dec.h, p(msgs), p(n), 1, 1, None, 1, ft8.HOST_PTRS) == -1 and b"NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_expect_update(dec.h, p(msgs), p(n), 1, 1, p(state), 1, ft8.HOST_PTRS) == 0 and state[0]["slot"] == 1
    d = dec.dev_alloc(16384)
    try:
        assert lib.ft8gpu_expect_update(dec.h, d, d, 1, 1, d + 4, 1, ft8.DEVICE_PTRS) == -1 and b"16-byte aligned" in lib.ft8gpu_last_error()
    finally:
        dec.dev_free(d)
    iq = np.zeros((1, 1, 2, ft8.NSAMPLES), np.float32)
    prm = ft8.ExpectParams(45, 0, 1)
    import ctypes as C
    eargs = lambda R, S, params: (dec.h, p(iq), R, S, p(state), params, p(msgs), p(n), None, ft8.HOST_PTRS)
    assert lib.ft8gpu_decode_messages_expected(*eargs(0, 1, C.byref(prm))) == 0
    assert lib.ft8gpu_decode_messages_expected(*eargs(1, 1, None)) == -1 and b"params" in lib.ft8gpu_last_error()
    bad = ft8.ExpectParams(175, 0, 1)
    assert lib.ft8gpu_decode_messages_expected(*eargs(1, 1, C.byref(bad))) == -1 and b"max_hard_errors" in lib.ft8gpu_last_error()
    assert state[0]["slot"] == 1
