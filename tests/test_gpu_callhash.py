"""GPU tests of the call hash table (ft8gpu_resolve_calls / ft8gpu_decode_messages_resolved): the stage entry on the constructed
records of tests/callhash_craft.py, frozen in tests/golden/callhash_cases.npz with what the restatement
(tests/ft8_spec_callhash.py) makes of them.  Every comparison is byte for byte on the resolved records (prefilled, so that the
records at and above a frame's count show a stray write), on the exit state, and -- in the device form -- on guard bands of
0xA5 around both device outputs.  Host form and device form.  tests/test_callhash_cpu.py proves on the CPU that the cases are
what they are named for."""
import numpy as np
import pytest

import callhash_craft as cc
import ft8_spec_callhash as sc
import synth_util as S

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xA5

_golden = {}


def golden():
    if not _golden:
        for c in cc.load_golden():
            for k in ("msgs", "n_msgs", "state", "resolved", "state_out"):
                c[k].setflags(write=False)
            _golden[c["name"]] = c
    return _golden


CASES = ["basic", "type4", "collide_12_record_order", "collide_12_field_order", "collide_12_across_slots", "collide_22",
         "age_0", "age_0_wrap", "age_1", "age_1_wrap", "age_2", "age_2_wrap", "chain", "counts", "long", "plain"]


def prefilled(shape):
    return np.frombuffer(np.full(int(np.prod(shape)) * 48, cc.JUNK, np.uint8).tobytes(), sc.RESOLVED_DTYPE).reshape(shape).copy()


def resolve_on_gpu(dec, form, msgs, n_msgs, state, max_age):
    """(resolved, exit state) as numpy arrays of the restatement's dtypes; resolved starts from cc.JUNK bytes"""
    import rtlsdr_ft8d_amd as ft8
    R, Sl = n_msgs.shape
    pre = prefilled((R, Sl, 50))
    if form == "host":
        res, st = dec.resolve_calls(msgs, n_msgs, state.view(ft8.CALLHASH_STATE_DTYPE), max_age, pre.view(ft8.RESOLVED_DTYPE))
        return res.view(sc.RESOLVED_DTYPE), st.view(sc.STATE_DTYPE)
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    msgs_d, n_d = up(msgs), up(n_msgs)
    bufs = []
    for a in (state, pre):
        b = torch.full((GUARD + a.nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        b[GUARD:GUARD + a.nbytes] = up(a)
        bufs.append(b)
    torch.cuda.synchronize()
    dec.resolve_calls_dev(msgs_d, n_d, R, Sl, bufs[0][GUARD:], max_age, bufs[1][GUARD:])
    dec.synchronize()
    out = []
    for a, b in zip((state, pre), bufs):
        h = b.cpu().numpy()
        assert (h[:GUARD] == FILL).all() and (h[GUARD + a.nbytes:] == FILL).all(), "a guard band was written"
        out.append(h[GUARD:GUARD + a.nbytes].copy())
    assert msgs_d.cpu().numpy().tobytes() == msgs.tobytes() and n_d.cpu().numpy().tobytes() == n_msgs.tobytes()    # inputs are inputs
    return out[1].view(sc.RESOLVED_DTYPE).reshape(R, Sl, 50), out[0].view(sc.STATE_DTYPE).reshape(R)


def first_difference(got, want):
    bad = np.argwhere((got.view(np.uint8).reshape(want.shape + (48,)) != want.view(np.uint8).reshape(want.shape + (48,))).any(axis=-1))
    if not len(bad):
        return None
    at = tuple(int(x) for x in bad[0])
    return len(bad), at, got[at], want[at]


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", CASES)
def test_stage_entry_equals_the_frozen_restatement(gpu_decoder, name, form):
    """tests 1 - 4 and 6 - 8 of the list: basic resolution, type 4, collisions, ageing with a wrapping counter, clamped counts,
    long texts, plain messages; and the mixed traffic of test 5 in one call"""
    g = golden()[name]
    res, st = resolve_on_gpu(gpu_decoder, form, g["msgs"], g["n_msgs"], g["state"], g["max_age"])
    assert res.tobytes() == g["resolved"].tobytes(), (name, first_difference(res, g["resolved"]))
    assert st.tobytes() == g["state_out"].tobytes(), name


def test_the_cases_list_is_the_golden_files():
    assert CASES == list(golden())


@pytest.mark.parametrize("form", ["host", "device"])
def test_chaining_and_independent_receivers(gpu_decoder, form):
    """one call of 4 slots = 4 calls of 1 slot = 2 + 2, states included; permuting receivers permutes the outputs; one
    receiver alone gives its rows"""
    g = golden()["chain"]
    msgs, n_msgs = g["msgs"], g["n_msgs"]
    want, want_st = sc.resolve(msgs, n_msgs, max_age=2, resolved=prefilled(msgs.shape))
    assert int(want["n_resolved"].sum()) >= 10
    for cuts in ((4,), (1, 1, 1, 1), (2, 2), (3, 1)):
        state, at, parts = sc.new_state(3), 0, []
        for k in cuts:
            r, state = resolve_on_gpu(gpu_decoder, form, np.ascontiguousarray(msgs[:, at:at + k]), np.ascontiguousarray(n_msgs[:, at:at + k]), state, 2)
            parts.append(r)
            at += k
        got = np.concatenate(parts, axis=1)
        assert got.tobytes() == want.tobytes(), (cuts, first_difference(got, want))
        assert state.tobytes() == want_st.tobytes(), cuts
    perm = [2, 0, 1]
    r, s = resolve_on_gpu(gpu_decoder, form, np.ascontiguousarray(msgs[perm]), np.ascontiguousarray(n_msgs[perm]), sc.new_state(3), 2)
    assert r.tobytes() == want[perm].tobytes() and s.tobytes() == want_st[perm].tobytes()
    r, s = resolve_on_gpu(gpu_decoder, form, np.ascontiguousarray(msgs[1:2]), np.ascontiguousarray(n_msgs[1:2]), sc.new_state(1), 2)
    assert r.tobytes() == want[1:2].tobytes() and s.tobytes() == want_st[1:2].tobytes()


@pytest.mark.parametrize("max_frames", [1, 2, 3, 5, 8])
def test_host_form_staging_cuts_along_slots_or_whole_receivers(max_frames):
    """3 receivers x 4 slots through contexts of 1, 2, 3 frames (runs of slots of one receiver), 5 (one whole receiver at a
    time) and 8 (two, then one): the bytes of one launch"""
    import rtlsdr_ft8d_amd as ft8
    g = golden()["chain"]
    want, want_st = sc.resolve(g["msgs"], g["n_msgs"], max_age=1, resolved=prefilled(g["msgs"].shape))
    with ft8.Decoder(device=0, max_frames=max_frames) as dec:
        res, st = resolve_on_gpu(dec, "host", g["msgs"], g["n_msgs"], sc.new_state(3), 1)
    assert res.tobytes() == want.tobytes(), first_difference(res, want)
    assert st.tobytes() == want_st.tobytes()


def test_an_empty_call_and_refused_arguments(gpu_decoder):
    import rtlsdr_ft8d_amd as ft8
    dec = gpu_decoder
    g = golden()["basic"]
    state = np.array(g["state"].view(ft8.CALLHASH_STATE_DTYPE), copy=True)
    res = prefilled((2, 2, 50))
    args = lambda R, Sl: (dec.h, g["msgs"].ctypes.data, g["n_msgs"].ctypes.data, R, Sl, state.ctypes.data, 0, res.ctypes.data, ft8.HOST_PTRS)
    assert dec.lib.ft8gpu_resolve_calls(*args(0, 2)) == 0 and dec.lib.ft8gpu_resolve_calls(*args(2, 0)) == 0
    assert state.tobytes() == g["state"].tobytes() and res.tobytes() == prefilled((2, 2, 50)).tobytes()
    for R, Sl, word in ((-1, 2, "negative"), (2, -1, "negative"), (1, (1 << 24) + 1, "exceeds")):
        assert dec.lib.ft8gpu_resolve_calls(*args(R, Sl)) == -1 and word.encode() in dec.lib.ft8gpu_last_error()
    assert dec.lib.ft8gpu_resolve_calls(dec.h, g["msgs"].ctypes.data, g["n_msgs"].ctypes.data, 2, 2, None, 0, res.ctypes.data, ft8.HOST_PTRS) == -1
    assert b"NULL" in dec.lib.ft8gpu_last_error()
    p = dec.dev_alloc(4096)
    try:
        assert dec.lib.ft8gpu_resolve_calls(dec.h, p, p, 1, 1, p + 4, 0, p, ft8.DEVICE_PTRS) == -1
        assert b"16-byte aligned" in dec.lib.ft8gpu_last_error()
    finally:
        dec.dev_free(p)
    assert state.tobytes() == g["state"].tobytes() and res.tobytes() == prefilled((2, 2, 50)).tobytes()


# ---- the whole path --------------------------------------------------------------------------------------------------------------

WHOLE = [[["CQ PJ4/K1ABC", "CQ K1ABC FN42", "W9XYZ K9AN -07"], ["<PJ4/K1ABC> W9XYZ -11", "<K1ABC> PJ4/W1AW RR73", "<KH1/KH7Z> K9AN R-03"]],
         [["CQ KH1/KH7Z", "CQ W1AW FN31"], ["KH7Z <KH1/KH7Z> RRR", "KH1/KH7Z <W1AW> 73", "<PJ4/K1ABC> W9XYZ -11"]]]
_whole = {}


def whole_frames():
    """2 receivers x 2 slots: strong signals (+3 dB in 2500 Hz) 350 Hz apart, the full calls one slot before their hashes"""
    if "iq" not in _whole:
        import rtlsdr_ft8d_amd as ft8
        iq = np.zeros((2, 2, 2, S.NSAMPLES), np.float32)
        for r in range(2):
            for s in range(2):
                rng = np.random.default_rng(900 + 2 * r + s)
                fi, fq = rng.normal(0.0, 1.0, S.NSAMPLES), rng.normal(0.0, 1.0, S.NSAMPLES)
                for k, text in enumerate(WHOLE[r][s]):
                    si, sq = S.cpfsk(ft8.encode(ft8.pack77(text)), 300.0 + 350.0 * k, int(round((0.3 + 0.2 * k) * 3200)), S.amplitude_for_snr(3.0, 1.0))
                    fi += si
                    fq += sq
                i32, q32 = fi.astype(np.float32), fq.astype(np.float32)
                scale = np.float32(0.5) / max(np.abs(i32).max(), np.abs(q32).max())
                iq[r, s, 0], iq[r, s, 1] = i32 * scale, q32 * scale
        iq.setflags(write=False)
        _whole["iq"] = iq
    return _whole["iq"]


def filled_msgs(shape):
    import rtlsdr_ft8d_amd as ft8
    return np.full(shape + (64,), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(shape)


@pytest.mark.parametrize("ap", [None, dict(passes=1, hyps=("CQ ? ?",))], ids=["plain", "ap"])
def test_whole_path(gpu_decoder, ap):
    """msgs and n_msgs are the bytes of the entry it wraps; resolved is the restatement applied to those records; host and
    device form"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    dec = gpu_decoder
    iq = whole_frames()
    flat = iq.reshape(4, 2, S.NSAMPLES)
    if ap is None:
        want_msgs, want_n = dec.decode_messages(flat, filled_msgs((4, 50)))
    else:
        want_msgs, want_n, _ = dec.decode_messages_ap(flat, ap["passes"], ap["hyps"], msgs=filled_msgs((4, 50)))
    texts = [[m["text"].decode().rstrip(" ") for m in want_msgs[f, :want_n[f]]] for f in range(4)]
    printed = [[t.replace("<PJ4/K1ABC>", "<...>").replace("<K1ABC>", "<...>").replace("<KH1/KH7Z>", "<...>").replace("<W1AW>", "<...>")
                for t in WHOLE[r][s]] for r in range(2) for s in range(2)]
    for f in range(4):
        assert set(printed[f]) <= set(texts[f]), (f, texts[f])                 # every planted message was decoded
    want_msgs, want_n = want_msgs.reshape(2, 2, 50), want_n.reshape(2, 2)
    want_res, want_st = sc.resolve(want_msgs, want_n, max_age=3, resolved=prefilled((2, 2, 50)))
    got_msgs, got_n, got_res, got_st = dec.decode_messages_resolved(iq, None, 3, ap, filled_msgs((2, 2, 50)), prefilled((2, 2, 50)).view(ft8.RESOLVED_DTYPE))
    assert got_msgs.tobytes() == want_msgs.tobytes() and np.array_equal(got_n, want_n)
    assert got_res.tobytes() == want_res.tobytes(), first_difference(got_res.view(sc.RESOLVED_DTYPE), want_res)
    assert got_st.tobytes() == want_st.tobytes()
    resolved_texts = {r["text"].decode().rstrip(" ") for f in ((0, 1), (1, 1)) for r in got_res[f][:got_n[f]]}
    assert {"<PJ4/K1ABC> W9XYZ -11", "<K1ABC> PJ4/W1AW RR73", "<...> K9AN R-03", "KH7Z <KH1/KH7Z> RRR", "KH1/KH7Z <W1AW> 73",
            "<...> W9XYZ -11"} <= resolved_texts, resolved_texts
    # device form, guard bands around the state and the resolved records
    iq_d = torch.from_numpy(np.array(iq)).cuda()
    msgs_d = torch.full((4 * 50 * 64,), FILL, dtype=torch.uint8, device="cuda")
    n_d = torch.full((4,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    sizes = (2 * 81936, 4 * 50 * 48)
    bufs = [torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device="cuda") for n in sizes]
    bufs[0][GUARD:GUARD + sizes[0]] = 0
    bufs[1][GUARD:GUARD + sizes[1]] = cc.JUNK
    torch.cuda.synchronize()
    dec.decode_messages_resolved_dev(iq_d, 2, 2, bufs[0][GUARD:], 3, msgs_d, n_d, bufs[1][GUARD:], ap)
    dec.synchronize()
    assert msgs_d.cpu().numpy().tobytes() == want_msgs.tobytes() and np.array_equal(n_d.cpu().numpy().reshape(2, 2), want_n)
    for b, n, want in zip(bufs, sizes, (want_st, want_res)):
        h = b.cpu().numpy()
        assert (h[:GUARD] == FILL).all() and (h[GUARD + n:] == FILL).all(), "a guard band was written"
        assert h[GUARD:GUARD + n].tobytes() == want.tobytes()
