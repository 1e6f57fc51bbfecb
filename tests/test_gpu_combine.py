"""GPU tests of the soft-bit memory (ft8gpu_combine_candidates, ft8gpu_softmem_update, ft8gpu_decode_messages_combined)
against the numpy restatement tests/ft8_spec_combine.py, byte for byte: the constructed frames frozen in
tests/golden/combine_constructed.npz under every configuration, in the host form (chunked), the device form and the device
form in place, with and without FT8GPU_DBG_FORCE_IEEE_DIV (the guard cases run both division forms); radio frames at
max_candidates 1, 2, 5, 120 and 1024 with ragged counts and guard records behind the counts, combining and the update rule;
the whole path on the 2 x 4 stream scenario as one call and as four calls of one slot, host and device form, through contexts
of 3, 5 and 16 frames.  tests/test_combine_cpu.py proves on the CPU that the cases are what they are named for."""
import numpy as np
import pytest

import combine_craft as cc
import ft8_spec_combine as sc

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, cc.FILL


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


def combine_dev(dec, mag, cands, counts, status_in, states, max_age, gate, status_out, info, in_place=False):
    """the device form between guard bands -> (status_out bytes, info bytes); the inputs stay as they are"""
    import torch
    B = len(counts)
    ins = [up(a) for a in (mag, cands, counts, status_in, states)]
    out_b, info_b = guarded(np.ascontiguousarray(status_out).view(np.uint8)), guarded(np.ascontiguousarray(info).view(np.uint8))
    torch.cuda.synchronize()
    dec.combine_candidates_dev(ins[0], ins[1], ins[2], out_b[GUARD:] if in_place else ins[3], B, ins[4], max_age, gate, out_b[GUARD:], info_b[GUARD:])
    dec.synchronize()
    for a, b in zip((mag, cands, counts, states), (ins[0], ins[1], ins[2], ins[4])):
        assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()          # inputs are inputs, the states read-only
    return unguard(out_b, status_out.nbytes).tobytes(), unguard(info_b, info.nbytes).tobytes()


def update_dev(dec, mag, cands, counts, status, info, states, store):
    """the device form of the update rule, the states between guard bands -> the exit states' bytes"""
    import torch
    ins = [up(a) for a in (mag, cands, counts, status, info)]
    st_b = guarded(states)
    torch.cuda.synchronize()
    dec.softmem_update_dev(ins[0], ins[1], ins[2], ins[3], ins[4], len(counts), st_b[GUARD:], store)
    dec.synchronize()
    for a, b in zip((mag, cands, counts, status, info), ins):
        assert b.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    return unguard(st_b, states.nbytes).tobytes()


def first_difference(got_info, want_info, where):
    g = np.frombuffer(got_info, sc.INFO_DTYPE).reshape(want_info.shape)
    bad = np.argwhere(g.view(np.uint64).reshape(want_info.shape) != want_info.view(np.uint64).reshape(want_info.shape))
    names = {v: k for k, v in where.items()}
    f, i = (int(x) for x in bad[0])
    return len(bad), names.get((f, i)), g[f, i], want_info[f, i]


# ---- the constructed frames ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    d = cc.load_golden()
    B, cap = d["cands"].shape
    behind = np.arange(cap)[None, :] >= d["counts"][:, None]
    d["fill_st"] = np.full((B, cap, 48), FILL, np.uint8)
    d["fill_info"] = np.full((B, cap * 8), FILL, np.uint8).view(sc.INFO_DTYPE).reshape(B, cap)
    for name, _age, _gate in cc.CONFIGS:
        assert (d["status_" + name][behind] == FILL).all()        # the fixture is in place on status_in: FILL behind the counts already
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@pytest.mark.parametrize("ieee", [0, 1])
@pytest.mark.parametrize("form", ["host", "device", "in_place"])
def test_stage_entry_equals_the_frozen_restatement(golden, form, ieee):
    """every configuration (max_age, min_agree) of the fixture, the guard cases among it, with the fast division forms behind
    their guards and with FT8GPU_DBG_FORCE_IEEE_DIV; the host form is chunked by max_frames 3 over 11 frames"""
    import rtlsdr_ft8d_amd as ft8
    d = golden
    B, cap = d["cands"].shape
    cands = d["cands"].view(ft8.CAND_DTYPE).reshape(B, cap)
    states = d["states"].view(ft8.SOFTMEM_STATE_DTYPE)
    with ft8.Decoder(device=0, max_frames=3 if form == "host" else B, max_candidates=cap) as dec:
        dec.set_debug_flags(ft8.DBG_FORCE_IEEE_DIV if ieee else 0)
        for name, max_age, gate in cc.CONFIGS:
            want_st, want_info = d["status_" + name].tobytes(), d["info_" + name].tobytes()
            if form == "host":
                st, info = dec.combine_candidates(d["mag"], cands, d["counts"], d["status_in"], states, max_age, gate,
                                                  status_out=d["fill_st"], info=d["fill_info"])
                got_st, got_info = st.tobytes(), info.tobytes()
            elif form == "device":
                got_st, got_info = combine_dev(dec, d["mag"], cands, d["counts"], d["status_in"], states, max_age, gate, d["fill_st"], d["fill_info"])
            else:
                got_st, got_info = combine_dev(dec, d["mag"], cands, d["counts"], d["status_in"], states, max_age, gate, d["status_in"],
                                               d["fill_info"], in_place=True)
            if got_info != want_info:
                raise AssertionError((name, form, ieee) + first_difference(got_info, d["info_" + name], d["where"]))
            assert got_st == want_st, (name, form, ieee)


@pytest.mark.parametrize("form", ["host", "device"])
def test_update_rule_equals_the_frozen_restatement(golden, form):
    """the exit states of every configuration at store_per_slot 0, 1, 3 and 128: ring wrap-around, a partner overwritten in
    the same slot, count saturating; the host form chunked by max_frames 4"""
    import rtlsdr_ft8d_amd as ft8
    d = golden
    B, cap = d["cands"].shape
    cands = d["cands"].view(ft8.CAND_DTYPE).reshape(B, cap)
    with ft8.Decoder(device=0, max_frames=4 if form == "host" else B, max_candidates=cap) as dec:
        for name, _age, _gate in cc.CONFIGS[:3]:
            status, info = d["status_" + name], d["info_" + name]
            for store in cc.STORES:
                want = d[f"after_{name}_{store}"]
                if form == "host":
                    got = dec.softmem_update(d["mag"], cands, d["counts"], status, info, d["states"], store).tobytes()
                else:
                    got = update_dev(dec, d["mag"], cands, d["counts"], status, info, d["states"], store)
                if got != want.tobytes():
                    g = np.frombuffer(got, sc.STATE_DTYPE)
                    f = int(np.flatnonzero([g[k].tobytes() != want[k].tobytes() for k in range(B)])[0])
                    e = [k for k in range(sc.ENTRIES) if g[f]["entry"][k].tobytes() != want[f]["entry"][k].tobytes()]
                    raise AssertionError((name, store, form, str(d["frame_names"][f]) if f < len(d["frame_names"]) else f, e[:8],
                                          int(g[f]["cursor"]), int(want[f]["cursor"]), int(g[f]["slot"]), int(want[f]["slot"])))


# ---- radio frames, any max_candidates ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stream_iq():
    iq, texts = cc.scenario()
    iq.setflags(write=False)
    return iq, texts


@pytest.mark.parametrize("cap", [1, 2, 5, 120, 1024])
def test_radio_frames_at_any_max_candidates(oracle, stream_iq, cap):
    """the device's own stages on the scenario's slots 0 and 2 (the same stations twice), counts made ragged (one frame 0),
    guard records behind them: the memory after slot 0 by the device's update rule, then combining in slot 2 in the host form,
    the device form and the device form in place, and the update rule again, all against the restatement"""
    import rtlsdr_ft8d_amd as ft8
    iq, _texts = stream_iq
    R = iq.shape[0]
    frames = np.ascontiguousarray(np.concatenate([iq[:, 0], iq[:, 2]]))               # [2 R]: slot 0 of every receiver, then slot 2
    store = 128 if cap != 120 else 40
    with ft8.Decoder(device=0, max_frames=2 * R, max_candidates=cap) as dec:
        mag = dec.waterfall(frames)
        cands, counts = dec.find_sync(mag)
        status = dec.decode_candidates(mag, cands, counts)
        counts = np.array(counts, copy=True)
        if cap > 2:
            counts[2 * R - 1] = max(1, int(counts[2 * R - 1]) * 2 // 3)
        status = np.array(status, copy=True).view(np.uint8).reshape(2 * R, cap, 48)
        status[np.arange(cap)[None, :] >= counts[:, None]] = FILL
        a, b = slice(0, R), slice(R, 2 * R)
        zero_info = np.zeros((R, cap), sc.INFO_DTYPE)
        st0 = sc.new_state(R)
        st0["slot"] = 7
        st0["cursor"] = [125 + 128 * (r % 3) for r in range(R)]            # the ring wraps within the slot
        want1 = sc.update(oracle, mag[a], cands[a], counts[a], status[a], zero_info, st0, store)
        got1 = dec.softmem_update(mag[a], cands[a], counts[a], status[a], zero_info, st0, store)
        assert got1.tobytes() == want1.tobytes(), (cap, "update after slot 0")
        assert update_dev(dec, mag[a], cands[a], counts[a], status[a], zero_info, st0, store) == want1.tobytes()
        fill_st = np.full((R, cap, 48), FILL, np.uint8)
        fill_info = np.full((R, cap * 8), FILL, np.uint8).view(sc.INFO_DTYPE).reshape(R, cap)
        cb = np.array(counts[b], copy=True)
        cb[0] = 0 if cap > 2 else cb[0]                                        # a frame without candidates
        for max_age, gate in ((0, 0), (0, 100), (1, 0)):
            states = np.array(want1, copy=True)
            states["slot"][0] += 1                                          # receiver 0 is one slot further: its entries are older
            kw = dict(iters=20, bp=oracle.bp_decode)
            want_st, want_info = sc.combine_candidates(oracle, mag[b], cands[b], cb, status[b], states, max_age, gate, status_out=fill_st,
                                                       info=fill_info, **kw)
            want_in = sc.combine_candidates(oracle, mag[b], cands[b], cb, status[b], states, max_age, gate, status_out=status[b], **kw)[0]
            st, info = dec.combine_candidates(mag[b], cands[b], cb, status[b], states, max_age, gate, status_out=fill_st, info=fill_info)
            assert info.tobytes() == want_info.tobytes() and st.tobytes() == want_st.tobytes(), (cap, max_age, gate, "host")
            got = combine_dev(dec, mag[b], cands[b], cb, status[b], states, max_age, gate, fill_st, fill_info)
            assert got == (want_st.tobytes(), want_info.tobytes()), (cap, max_age, gate, "device")
            got = combine_dev(dec, mag[b], cands[b], cb, status[b], states, max_age, gate, status[b], fill_info, in_place=True)
            assert got == (want_in.tobytes(), want_info.tobytes()), (cap, max_age, gate, "in place")
            want2 = sc.update(oracle, mag[b], cands[b], cb, want_in, want_info, states, store)
            assert dec.softmem_update(mag[b], cands[b], cb, want_in, want_info, states, store).tobytes() == want2.tobytes(), (cap, max_age, gate)
            assert update_dev(dec, mag[b], cands[b], cb, want_in, want_info, states, store) == want2.tobytes(), (cap, max_age, gate)
            if cap == 120 and (max_age, gate) == (0, 0):
                r = want_info["result"][np.arange(cap)[None, :] < cb[:, None]]
                assert (r == 1).sum() >= 1 and (r == 7).sum() >= 1             # BP ran, with and without success


# ---- the whole path ----------------------------------------------------------------------------------------------------------------

def filled_msgs(shape):
    import rtlsdr_ft8d_amd as ft8
    return np.full(shape + (64,), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(shape)


PATH_ARGS = dict(min_agree=96, max_age=3, store_per_slot=48)


@pytest.fixture(scope="module")
def stream(oracle, stream_iq):
    iq, texts = stream_iq
    R, S = iq.shape[:2]
    want = sc.decode_combined(oracle, iq, msgs=filled_msgs((R, S, 50)), bp=oracle.bp_decode, **PATH_ARGS)
    return iq, texts, want


@pytest.mark.parametrize("max_frames", [3, 5, 8, 16])
def test_whole_path_on_the_stream_scenario(stream, max_frames):
    """msgs, n_msgs, n_by_stage and the exit state of 2 receivers x 4 slots against the restatement: one call, four calls of one
    slot, host and device form; through contexts of 3 frames (runs of slots), 5 (a receiver at a time), 8 (both receivers in
    one piece that fills the context) and 16 (all at once).
    The records below the BP count are the bytes of ft8gpu_decode_messages.  Slot 2 gains messages only through combining."""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq, texts, want = stream
    R, S = iq.shape[:2]
    assert R * S >= 8
    want_msgs, want_n, want_nbs, want_st = want
    p = (PATH_ARGS["min_agree"], PATH_ARGS["max_age"], PATH_ARGS["store_per_slot"])
    assert (want_nbs[:, 2, 1] > want_nbs[:, 2, 0]).any() and (want_nbs[:, 0, 1] == want_nbs[:, 0, 0]).all()
    for r in range(R):
        for k in range(int(want_nbs[r, 2, 0]), int(want_nbs[r, 2, 1])):
            assert want_msgs[r, 2, k]["text"].decode() in texts[r][2] and want_msgs[r, 2, k]["pad"][2] == 2
    with ft8.Decoder(device=0, max_frames=max_frames) as dec:
        msgs, n, nbs, st = dec.decode_messages_combined(iq, None, *p, filled_msgs((R, S, 50)))
        assert np.array_equal(n, want_n) and np.array_equal(nbs, want_nbs)
        assert msgs.tobytes() == want_msgs.tobytes() and st.tobytes() == want_st.tobytes()
        # four calls of one slot
        st1, parts = None, []
        for s in range(S):
            m1, n1, b1, st1 = dec.decode_messages_combined(np.ascontiguousarray(iq[:, s:s + 1]), st1, *p, filled_msgs((R, 1, 50)))
            parts.append((m1, n1, b1))
        assert np.concatenate([q[0] for q in parts], axis=1).tobytes() == want_msgs.tobytes()
        assert np.array_equal(np.concatenate([q[1] for q in parts], axis=1), want_n)
        assert np.array_equal(np.concatenate([q[2] for q in parts], axis=1), want_nbs) and st1.tobytes() == want_st.tobytes()
        if max_frames not in (8, 16):
            # the device form through the same cuts: runs of slots of one receiver (3), a receiver at a time (5)
            iq_d = torch.from_numpy(np.array(iq)).cuda()
            junk = np.full((R, S, 2), -0x5A5A5A5B, np.int32)
            bufs = [guarded(filled_msgs((R, S, 50))), guarded(junk[:, :, 0]), guarded(junk), guarded(sc.new_state(R))]
            torch.cuda.synchronize()
            dec.decode_messages_combined_dev(iq_d, R, S, bufs[3][GUARD:], *p, bufs[0][GUARD:], bufs[1][GUARD:], bufs[2][GUARD:])
            dec.synchronize()
            assert unguard(bufs[0], want_msgs.nbytes).tobytes() == want_msgs.tobytes()
            assert unguard(bufs[1], want_n.nbytes).tobytes() == want_n.tobytes() and unguard(bufs[3], want_st.nbytes).tobytes() == want_st.tobytes()
            assert unguard(bufs[2], want_nbs.nbytes).tobytes() == want_nbs.tobytes() and iq_d.cpu().numpy().tobytes() == iq.tobytes()
            return
        # the records below the BP count are those of ft8gpu_decode_messages
        plain, pn = dec.decode_messages(iq.reshape(R * S, 2, -1), filled_msgs((R * S, 50)))
        assert np.array_equal(pn.reshape(R, S), want_nbs[:, :, 0])
        for f in range(R * S):
            assert plain[f, :pn[f]].tobytes() == msgs.reshape(R * S, 50)[f, :pn[f]].tobytes()
        # device form between guard bands, n_by_stage present and absent
        iq_d = torch.from_numpy(np.array(iq)).cuda()
        junk = np.full((R, S, 2), -0x5A5A5A5B, np.int32)
        for with_nbs in (True, False):
            bufs = [guarded(filled_msgs((R, S, 50))), guarded(junk[:, :, 0]), guarded(junk), guarded(sc.new_state(R))]
            torch.cuda.synchronize()
            dec.decode_messages_combined_dev(iq_d, R, S, bufs[3][GUARD:], *p, bufs[0][GUARD:], bufs[1][GUARD:],
                                             bufs[2][GUARD:] if with_nbs else None)
            dec.synchronize()
            assert unguard(bufs[0], want_msgs.nbytes).tobytes() == want_msgs.tobytes()
            assert unguard(bufs[1], want_n.nbytes).tobytes() == want_n.tobytes() and unguard(bufs[3], want_st.nbytes).tobytes() == want_st.tobytes()
            assert unguard(bufs[2], want_nbs.nbytes).tobytes() == (want_nbs.tobytes() if with_nbs else junk.tobytes())
        if max_frames != 16:
            return
        # four calls of one slot in the device form (one slot per receiver: no staging), the state carried on the device
        state_d = guarded(sc.new_state(R))
        for s in range(S):
            iq_s = torch.from_numpy(np.ascontiguousarray(iq[:, s])).cuda()
            bufs = [guarded(filled_msgs((R, 1, 50))), guarded(junk[:, :1, 0]), guarded(junk[:, :1])]
            torch.cuda.synchronize()
            dec.decode_messages_combined_dev(iq_s, R, 1, state_d[GUARD:], *p, bufs[0][GUARD:], bufs[1][GUARD:], bufs[2][GUARD:])
            dec.synchronize()
            assert unguard(bufs[0], want_msgs[:, s].nbytes).tobytes() == want_msgs[:, s].tobytes(), s
            assert unguard(bufs[1], 4 * R).tobytes() == want_n[:, s].tobytes() and unguard(bufs[2], 8 * R).tobytes() == want_nbs[:, s].tobytes(), s
        assert unguard(state_d, want_st.nbytes).tobytes() == want_st.tobytes()
        # one receiver, four slots, in the device form
        bufs = [guarded(filled_msgs((1, S, 50))), guarded(junk[:1, :, 0]), guarded(sc.new_state(1))]
        torch.cuda.synchronize()
        dec.decode_messages_combined_dev(iq_d[1:2], 1, S, bufs[2][GUARD:], *p, bufs[0][GUARD:], bufs[1][GUARD:], None)
        dec.synchronize()
        assert unguard(bufs[0], want_msgs[1].nbytes).tobytes() == want_msgs[1].tobytes() and unguard(bufs[1], 4 * S).tobytes() == want_n[1].tobytes()
        assert unguard(bufs[2], want_st[1:2].nbytes).tobytes() == want_st[1:2].tobytes()
        assert iq_d.cpu().numpy().tobytes() == iq.tobytes()


def test_empty_calls_and_refused_arguments(gpu_decoder):
    import ctypes as C
    import rtlsdr_ft8d_amd as ft8
    dec, lib = gpu_decoder, gpu_decoder.lib
    cap = dec.max_candidates
    mag, cands, counts = np.zeros((1, ft8.MAG_ARRAY), np.uint8), np.zeros((1, cap), ft8.CAND_DTYPE), np.zeros(1, np.int32)
    status, info, state = np.zeros((1, cap, 48), np.uint8), np.zeros((1, cap), ft8.COMBINE_INFO_DTYPE), ft8.softmem_state(1)
    p = lambda a: a.ctypes.data
    cargs = lambda n, gate, st=state: (dec.h, p(mag), p(cands), p(counts), p(status), n, p(st) if st is not None else None, 0, gate, p(status), p(info), ft8.HOST_PTRS)
    assert lib.ft8gpu_combine_candidates(*cargs(0, 100)) == 0 and lib.ft8gpu_combine_candidates(*cargs(1, 100)) == 0
    for gate in (-1, 175):
        assert lib.ft8gpu_combine_candidates(*cargs(1, gate)) == -1 and b"min_agree" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_combine_candidates(*cargs(1, 100, None)) == -1 and b"NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_combine_candidates(*cargs(-1, 100)) == -1
    uargs = lambda n, store, st=state: (dec.h, p(mag), p(cands), p(counts), p(status), p(info), n, p(st) if st is not None else None, store, ft8.HOST_PTRS)
    assert lib.ft8gpu_softmem_update(*uargs(0, 16)) == 0 and state.tobytes() == ft8.softmem_state(1).tobytes()
    for store in (-1, 129):
        assert lib.ft8gpu_softmem_update(*uargs(1, store)) == -1 and b"store_per_slot" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_softmem_update(*uargs(1, 16, None)) == -1 and b"NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_softmem_update(*uargs(1, 16)) == 0 and state[0]["slot"] == 1 and state[0]["cursor"] == 0
    d = dec.dev_alloc(2 * sc.STATE_DTYPE.itemsize)
    try:
        assert lib.ft8gpu_softmem_update(dec.h, d, d, d, d, d, 1, d + 4, 16, ft8.DEVICE_PTRS) == -1 and b"16-byte aligned" in lib.ft8gpu_last_error()
        assert lib.ft8gpu_combine_candidates(dec.h, d, d, d, d, 1, d + 8, 0, 100, d, d, ft8.DEVICE_PTRS) == -1 and b"16-byte aligned" in lib.ft8gpu_last_error()
    finally:
        dec.dev_free(d)
    iq = np.zeros((1, 1, 2, ft8.NSAMPLES), np.float32)
    msgs, n = np.zeros((1, 1, 50), ft8.MESSAGE_DTYPE), np.zeros((1, 1), np.int32)
    prm = ft8.CombineParams(100, 0, 16)
    eargs = lambda R, S, params, st=state: (dec.h, p(iq), R, S, p(st) if st is not None else None, params, p(msgs), p(n), None, ft8.HOST_PTRS)
    assert lib.ft8gpu_decode_messages_combined(*eargs(0, 1, C.byref(prm))) == 0
    assert lib.ft8gpu_decode_messages_combined(*eargs(1, 0, C.byref(prm))) == 0
    assert lib.ft8gpu_decode_messages_combined(*eargs(1, 1, None)) == -1 and b"params" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_decode_messages_combined(*eargs(1, 1, C.byref(prm), None)) == -1 and b"NULL" in lib.ft8gpu_last_error()
    for bad in (ft8.CombineParams(175, 0, 16), ft8.CombineParams(-1, 0, 16)):
        assert lib.ft8gpu_decode_messages_combined(*eargs(1, 1, C.byref(bad))) == -1 and b"min_agree" in lib.ft8gpu_last_error()
    for bad in (ft8.CombineParams(100, 0, 129), ft8.CombineParams(100, 0, -1)):
        assert lib.ft8gpu_decode_messages_combined(*eargs(1, 1, C.byref(bad))) == -1 and b"store_per_slot" in lib.ft8gpu_last_error()
    assert state[0]["slot"] == 1
    assert lib.ft8gpu_decode_messages_combined(*eargs(1, 1, C.byref(prm))) == 0 and state[0]["slot"] == 2
