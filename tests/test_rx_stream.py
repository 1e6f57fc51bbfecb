"""ft8gpu_rx_stream: the RX front end with the filter state carried from one 15 s slot into the next, as the reference's
daemon runs rtlsdr_callback() (rtlsdr_ft8d.c:76-202: the integrators, comb delays, decimationIndex and FIR history
are function statics that are never reset).  Every comparison is on float bit patterns, counts and state bytes: exact.
Ground truth is tests/rx_stream_util.py (the oracle's callback with a carried state), which is itself held to one pass
over the concatenated bytes and to the reference's own rtlsdr_callback (oracle/_ref/ref_oracle)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib
import rx_stream_util as U
from test_reference_exec import _binary, ref_rx
from test_rx import make_capture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = 48000
KINDS = ("signal", "random", "extremes")
FULL = 36_000_000                                   # pairs of a 15 s slot at 2.4 Msps; 36 000 000 = 751 * 47936 + 64


def stream_raw(seed, nslots, npairs, kind):
    """one receiver's consecutive slots: a single capture of nslots * npairs pairs, cut"""
    return make_capture(seed, nslots * npairs, kind).reshape(nslots, 2 * npairs)


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_chain_equals_one_pass_over_the_concatenated_bytes(oracle, kind):
    npairs, S = 751 * 200 + 8 * 37, 5
    raw = stream_raw(3, S, npairs, kind)
    frames, counts, st = U.oracle_chain(raw)
    whole, nwhole, stw = U.oracle_chain(raw.reshape(1, -1))
    d = 0
    for s in range(S):
        assert counts[s] == (d + npairs) // 751
        d = (d + npairs) % 751
        assert not frames[s][:, counts[s]:].any()
    assert int(st["decimationIndex"][0]) == d != 0
    assert int(counts.sum()) == int(nwhole[0]) == S * npairs // 751 < NS
    cat = np.concatenate([frames[s][:, :counts[s]] for s in range(S)], axis=1)
    assert np.array_equal(U.bits(cat), U.bits(whole[0][:, :nwhole[0]]))
    assert same_bytes(st, stw)
    # a carried slot is not a slot from reset: every sample differs (the decimation grid is shifted)
    fresh, nfresh, _ = U.oracle_chain(raw[1:2])
    n = min(int(nfresh[0]), int(counts[1]))
    assert n >= 200 and np.all(U.bits(fresh[0][:, :n]) != U.bits(frames[1][:, :n]))


def test_rx_state_abi_layout_and_reset():
    import rtlsdr_ft8d_amd as ft8
    names = list(ft8.RX_STATE_DTYPE.names)
    assert names == list(U.ORACLE_STATE_DTYPE.names) and ft8.RX_STATE_DTYPE.itemsize == 516
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "ft8gpu.h"
#include "ft8_oracle.h"
#define F(f) printf("%zu %zu %zu %zu\n", offsetof(ft8gpu_rx_state, f), offsetof(ft8o_rx_state_t, f), sizeof(((ft8gpu_rx_state *)0)->f), sizeof(((ft8o_rx_state_t *)0)->f));
int main(void){ printf("%zu %zu 0 0\n", sizeof(ft8gpu_rx_state), sizeof(ft8o_rx_state_t));
 F(Ix1) F(Ix2) F(Qx1) F(Qx2) F(Iy1) F(It1y) F(It1z) F(Qy1) F(Qt1y) F(Qt1z) F(Iy2) F(It2y) F(It2z) F(Qy2) F(Qt2y) F(Qt2z)
 F(decimationIndex) F(firI) F(firQ) return 0; }'''
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        with open(src, "w") as f:
            f.write(prog)
        subprocess.check_call(["gcc", "-std=gnu17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"), src, "-o", exe])
        rows = [tuple(map(int, l.split())) for l in subprocess.check_output([exe]).decode().splitlines()]
    assert rows[0][:2] == (516, 516)
    for name, (og, oo, sg, so) in zip(names, rows[1:]):
        assert og == oo == ft8.RX_STATE_DTYPE.fields[name][1] and sg == so == ft8.RX_STATE_DTYPE.fields[name][0].itemsize, name
    lib = ft8.load_library()
    st = U.pattern(3, ft8.RX_STATE_DTYPE)
    lib.ft8gpu_rx_state_reset(st[1:].ctypes.data)
    assert not st[1:2].view(np.uint8).any() and np.all(st[0:1].view(np.uint8) == U.FILL) and np.all(st[2:3].view(np.uint8) == U.FILL)
    assert same_bytes(st[1:2], U.reset_state())
    lib.ft8gpu_rx_state_reset(None)


def _a_then_b(kind, npairs_b):
    """A short, B behind it; decimationIndex after A is not 0"""
    npairs_a = 751 * 104 + 8 * 37
    raw = make_capture(21, npairs_a + npairs_b, kind)
    return raw, raw[:2 * npairs_a], raw[2 * npairs_a:]


@pytest.mark.parametrize("kind", KINDS)
def test_reference_callback_carries_its_state_like_the_oracle_chain(oracle, kind):
    """the reference's own rtlsdr_callback over A || B from reset: its outputs [nA:48000] are what the chain stores for B
    when B starts from the state A left"""
    ref_oracle = _binary("ref_oracle")
    raw, a, b = _a_then_b(kind, 751 * 3000 + 8 * 11)
    ri, rq, rn = ref_rx(ref_oracle, raw, 65536)
    st = U.reset_state()
    fa, na = U.oracle_slot(st, a)
    assert na == 104 and int(st["decimationIndex"][0]) == 8 * 37
    fb, nb = U.oracle_slot(st, b)
    assert rn == na + nb < NS
    ref = np.stack([ri, rq])
    assert np.array_equal(U.bits(fa[:, :na]), U.bits(ref[:, :na]))
    assert np.array_equal(U.bits(fb[:, :nb]), U.bits(ref[:, na:na + nb]))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def gpu_host(dec, raw, states, normalise):
    """host-pointer form into 0xA5-patterned outputs"""
    import rtlsdr_ft8d_amd as ft8
    nstreams, nslots = raw.shape[:2]
    iq, n_out, st = dec.rx_stream(raw, None if states is None else states.view(ft8.RX_STATE_DTYPE), normalise,
                                  iq=U.pattern((nstreams, nslots, 2, NS), np.float32), n_out=U.pattern((nstreams, nslots), np.uint32))
    return iq, n_out, st


def gpu_dev(dec, raw, states, normalise, guard=0):
    """device-pointer form; with guard > 0 every output sits between two guard bands of `guard` bytes that must stay 0xA5"""
    import torch
    nstreams, nslots = raw.shape[:2]
    npairs = raw.shape[2] // 2
    st0 = U.reset_state().repeat(nstreams) if states is None else states
    d_raw = torch.from_numpy(np.ascontiguousarray(raw)).cuda()

    def banded(nbytes, init=None):
        t = torch.full((guard + nbytes + guard,), U.FILL, dtype=torch.uint8, device="cuda")
        if init is not None:
            t[guard:guard + nbytes] = torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).reshape(-1)).cuda()
        return t
    b_iq, b_n, b_st = banded(nstreams * nslots * 2 * NS * 4), banded(nstreams * nslots * 4), banded(nstreams * 516, st0)
    torch.cuda.synchronize()
    dec.rx_stream_dev(d_raw, nstreams, nslots, npairs, b_st.data_ptr() + guard, b_iq.data_ptr() + guard, b_n.data_ptr() + guard, normalise)
    dec.synchronize()
    out = []
    for t, dt, shape in ((b_iq, np.float32, (nstreams, nslots, 2, NS)), (b_n, np.uint32, (nstreams, nslots)), (b_st, U.ORACLE_STATE_DTYPE, (nstreams,))):
        h = t.cpu().numpy()
        if guard:
            assert np.all(h[:guard] == U.FILL) and np.all(h[-guard:] == U.FILL), f"a guard band around {np.dtype(dt)} was written"
        out.append(h[guard:h.size - guard].copy().view(dt).reshape(shape))
    return out


def check(got, want, what):
    (iq, n_out, st), (wiq, wn, wst) = got, want
    assert np.array_equal(np.asarray(n_out, np.uint32), wn), (what, n_out, wn)
    assert same_bytes(st, wst), f"{what}: exit state differs"
    for k in range(wiq.shape[0]):
        for s in range(wiq.shape[1]):
            for ch in range(2):
                d = np.flatnonzero(U.bits(iq[k, s, ch]) != U.bits(wiq[k, s, ch]))
                assert d.size == 0, f"{what}: stream {k} slot {s} {'IQ'[ch]}: {d.size} samples differ, first at {d[0]} (stored {wn[k, s]})"


RX_CASES = [("signal", 751 * 3000 + 8 * 37), ("random", 751 * 2000), ("extremes", 751 * 1500 + 744), ("zeros", 751 * 100),
            ("signal", 8 * 50), ("random", 751 * 48000 + 8 * 1000), ("random", 752), ("extremes", 751 * 17 + 1), ("random", 751 * 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,npairs", RX_CASES)
def test_gpu_rx_stream_from_reset_equals_rx_decimate(gpu_decoder, kind, npairs):
    """the cases of tests/test_rx.py::test_gpu_rx_bit_exact"""
    npairs -= npairs % 8
    raws = np.stack([make_capture(10 + k, npairs, kind) for k in range(2)])
    for normalise in (False, True):
        want = gpu_decoder.rx_decimate(raws, normalise=normalise)
        iq, n_out, st = gpu_host(gpu_decoder, raws[:, None, :], None, normalise)
        assert np.all(n_out == min(NS, npairs // 751))
        assert np.all(st["decimationIndex"] == npairs % 751)
        assert iq[:, 0].tobytes() == want.tobytes(), f"{kind}/{npairs} normalise={normalise}"


def entry_states(nstreams):
    """reset for stream 0; the others from the oracle after a prefix that ends in the middle of a block"""
    sts = [U.reset_state()]
    for k in range(1, nstreams):
        sts.append(U.state_after(make_capture(70 + k, 751 * 8 * (7 + k) + 8 * (11 + 30 * k), "signal")))
    st = np.concatenate(sts)
    assert all(int(d) % 751 != 0 for d in st["decimationIndex"][1:])
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("host", "device"))
@pytest.mark.parametrize("kind", KINDS + ("zeros",))
def test_gpu_rx_stream_chained_slots_equal_the_oracle(oracle, gpu_decoder, kind, form):
    nstreams, nslots, npairs = 3, 4, 751 * 304 + 8 * 37                   # the phase drifts by 296 per slot
    raw = np.stack([stream_raw(30 + k, nslots, npairs, kind) for k in range(nstreams)])
    st0 = entry_states(nstreams)
    for normalise in (False, True):
        want = U.oracle_streams(raw, st0, normalise)
        assert len(set(want[1].reshape(-1).tolist())) > 1                 # the drift shows in the counts
        got = gpu_host(gpu_decoder, raw, st0, normalise) if form == "host" else gpu_dev(gpu_decoder, raw, st0, normalise)
        check(got, want, f"{kind} {form} normalise={normalise}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("host", "device"))
def test_gpu_rx_stream_short_slots_and_single_events(oracle, gpu_decoder, form):
    run = (lambda raw, st, nm: gpu_host(gpu_decoder, raw, st, nm)) if form == "host" else (lambda raw, st, nm: gpu_dev(gpu_decoder, raw, st, nm))
    mid = U.state_after(make_capture(41, 751 * 72 + 8 * 45, "signal"))    # the middle of a block: decimationIndex 360
    assert int(mid["decimationIndex"][0]) == 360
    late = U.state_after(make_capture(42, 751 * 56 + 744, "random"))      # 7 pairs before an event
    assert int(late["decimationIndex"][0]) == 744
    for normalise in (False, True):
        # slots shorter than one block: no output, the state still advances
        for st0, nslots in ((mid, 4), (U.reset_state(), 1), (mid, 1)):
            raw = stream_raw(43, nslots, 8, "random")[None]
            want = U.oracle_streams(raw, st0, normalise)
            assert not want[1].any()
            check(run(raw, st0, normalise), want, f"npairs 8 x {nslots} from {int(st0['decimationIndex'][0])}")
        # 8-pair slots one of which holds the event
        raw = stream_raw(44, 4, 8, "extremes")[None]
        want = U.oracle_streams(raw, late, normalise)
        assert want[1].tolist() == [[1, 0, 0, 0]]
        check(run(raw, late, normalise), want, "npairs 8 x 4 across an event")
        # a call whose only slot holds exactly one decimation event: fewer than 2 outputs shift the comb delays, fewer
        # than 56 shift the FIR history
        for st0, npairs in ((U.reset_state(), 752), (mid, 752), (mid, 392), (late, 8), (mid, 751 * 32 + 8)):
            raw = stream_raw(45, 1, npairs, "signal")[None]
            want = U.oracle_streams(raw, st0, normalise)
            assert want[1][0, 0] == (int(st0["decimationIndex"][0]) + npairs) // 751
            check(run(raw, st0, normalise), want, f"one slot of {npairs} pairs from {int(st0['decimationIndex'][0])}")
        assert U.oracle_streams(stream_raw(45, 1, 752, "signal")[None], mid)[1][0, 0] == 1


@pytest.mark.gpu
def test_gpu_rx_stream_slot_with_more_than_48000_events(oracle, gpu_decoder):
    """the filters keep running past the 48000th output of a slot (:195-200): the next slot starts from that state"""
    npairs = 751 * 48000 + 8 * 1000
    raw = stream_raw(46, 2, npairs, "random")[None]
    mid = U.state_after(make_capture(41, 751 * 72 + 8 * 45, "signal"))
    for normalise in (False, True):
        want = U.oracle_streams(raw, mid, normalise)
        assert want[1].tolist() == [[NS, NS]]
        check(gpu_host(gpu_decoder, raw, mid, normalise), want, f"over-long slots normalise={normalise}")


@pytest.mark.gpu
def test_gpu_rx_stream_split_invariance(oracle, gpu_decoder):
    npairs, N = 751 * 504 + 8 * 53, 6
    raw = np.stack([stream_raw(50 + k, N, npairs, kind) for k, kind in enumerate(("signal", "random"))])
    st0 = entry_states(2)
    # nslots = N in one call equals N calls of one slot
    for normalise in (False, True):
        iq, n_out, st = gpu_host(gpu_decoder, raw, st0, normalise)
        cur = st0.copy()
        for s in range(N):
            iq1, n1, cur = gpu_host(gpu_decoder, raw[:, s:s + 1], cur, normalise)
            assert iq1.tobytes() == iq[:, s:s + 1].tobytes() and np.array_equal(n1, n_out[:, s:s + 1]), (s, normalise)
        assert same_bytes(cur, st)
    # one stream cut into calls at multiple-of-8 split points: the same concatenated outputs and end state as one call
    total = N * npairs
    assert (int(st0["decimationIndex"][1]) + total) // 751 < NS
    one = raw[1].reshape(1, 1, -1)
    iq, n_out, st = gpu_host(gpu_decoder, one, st0[1:2], False)
    whole = iq[0, 0][:, :n_out[0, 0]]
    rng = np.random.default_rng(6)
    for cuts in ([8], [752], [total - 8], sorted((8 * rng.choice(np.arange(1, total // 8), 7, replace=False)).tolist()),
                 [8 * k for k in range(1, 200)]):
        cur, parts = st0[1:2].copy(), []
        for a, b in zip([0] + cuts, cuts + [total]):
            iq1, n1, cur = gpu_host(gpu_decoder, one[:, :, 2 * a:2 * b], cur, False)
            parts.append(iq1[0, 0][:, :n1[0, 0]])
        assert np.array_equal(U.bits(np.concatenate(parts, axis=1)), U.bits(whole)), cuts[:8]
        assert same_bytes(cur, st), cuts[:8]


@pytest.mark.gpu
def test_gpu_rx_stream_full_size_slots(oracle, gpu_decoder):
    """2 streams x 2 slots of 36 000 000 pairs.  From reset the second slot enters at decimationIndex 64 and both slots store
    47936 samples; from decimationIndex 704 the first slot stores 47937."""
    raw = np.stack([stream_raw(60 + k, 2, FULL, kind) for k, kind in enumerate(("random", "signal"))])
    st0 = np.concatenate([U.reset_state(), U.state_after(make_capture(62, 751 * 80 + 704, "signal"))])
    assert st0["decimationIndex"].tolist() == [0, 704]
    want = U.oracle_streams(raw, st0, True)
    assert want[1].tolist() == [[47936, 47936], [47937, 47936]] and want[2]["decimationIndex"].tolist() == [128, 81]
    check(gpu_host(gpu_decoder, raw, st0, True), want, "full size, host form")
    check(gpu_dev(gpu_decoder, raw, st0, True), want, "full size, device form")


@pytest.mark.gpu
def test_gpu_rx_stream_against_the_reference_callback(oracle, gpu_decoder):
    """the reference's own rtlsdr_callback over A || B from reset (oracle/_ref/ref_oracle), B a full 15 s slot: the library,
    called for A and then for B with the carried state, stores for B what the reference computes behind A's outputs"""
    ref_oracle = _binary("ref_oracle")
    raw, a, b = _a_then_b("signal", FULL)
    ri, rq, rn = ref_rx(ref_oracle, raw, 65536)
    ref = np.stack([ri, rq])
    assert rn == NS
    fa, na, st = gpu_host(gpu_decoder, a[None, None, :], None, False)
    assert na[0, 0] == 104 and st["decimationIndex"][0] == 8 * 37
    fb, nb, st = gpu_host(gpu_decoder, b[None, None, :], st, False)
    assert nb[0, 0] == (8 * 37 + FULL) // 751 >= NS - 104
    assert np.array_equal(U.bits(fa[0, 0][:, :104]), U.bits(ref[:, :104]))
    assert np.array_equal(U.bits(fb[0, 0][:, :NS - 104]), U.bits(ref[:, 104:]))


@pytest.mark.gpu
def test_gpu_rx_stream_feeds_decoder(oracle, gpu_decoder):
    """a carried frame -> decode, all on the GPU, equals the oracle doing the same on the oracle's carried frame"""
    npairs = 751 * 6000 + 64
    raw = stream_raw(5, 2, npairs, "signal")[None]
    iq, n_out, _ = gpu_decoder.rx_stream(raw, normalise=True)
    want, wn, _ = U.oracle_chain(raw[0], None, True)
    assert np.array_equal(n_out[0], wn) and np.array_equal(U.bits(iq[0]), U.bits(want))
    dec, n = gpu_decoder.decode_batch(iq[0])
    for s in range(2):
        rdec, rn = oracle.subsystem(want[s, 0], want[s, 1])
        assert n[s] == rn and dec[s].tobytes() == rdec.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("nstreams,nslots,npairs", [(1, 1, 8), (3, 1, 751 * 16 + 8), (2, 3, 751 * 257 + 8 * 3), (1, 5, 760), (5, 3, 8 * 31)])
def test_gpu_rx_stream_guard_bands(oracle, gpu_decoder, nstreams, nslots, npairs):
    npairs -= npairs % 8
    raw = np.stack([stream_raw(80 + k, nslots, npairs, "random") for k in range(nstreams)])
    st0 = np.concatenate([U.state_after(make_capture(90 + k, 751 * 56 + 8 * (5 + 17 * k), "extremes")) for k in range(nstreams)])
    for normalise in (False, True):
        check(gpu_dev(gpu_decoder, raw, st0, normalise, guard=4096), U.oracle_streams(raw, st0, normalise), f"guarded {nstreams}x{nslots}x{npairs}")


@pytest.mark.gpu
def test_gpu_rx_stream_argument_errors(gpu_decoder):
    import torch
    import rtlsdr_ft8d_amd as ft8
    lib, h = gpu_decoder.lib, gpu_decoder.h
    raw = make_capture(1, 2 * 800, "random").reshape(1, 2, -1)
    st = U.state_after(make_capture(2, 751 * 64 + 8 * 9, "signal")).view(ft8.RX_STATE_DTYPE)
    iq, n_out = U.pattern((1, 2, 2, NS), np.float32), U.pattern((1, 2), np.uint32)

    def call(raw_p, nstreams, nslots, npairs, st_p, iq_p, flags=ft8.HOST_PTRS):
        before = st.tobytes()
        rc = lib.ft8gpu_rx_stream(h, raw_p, nstreams, nslots, npairs, st_p, iq_p, n_out.ctypes.data, 1, flags)
        msg = lib.ft8gpu_last_error()
        msg = msg.decode() if isinstance(msg, bytes) else C.cast(msg, C.c_char_p).value.decode()
        assert rc != 0 and msg, (rc, msg)
        assert st.tobytes() == before and np.all(iq.view(np.uint8) == U.FILL) and np.all(n_out.view(np.uint8) == U.FILL)
        return msg
    p = (raw.ctypes.data, st.ctypes.data, iq.ctypes.data)
    assert "multiple of 8" in call(p[0], 1, 2, 796, p[1], p[2])
    assert "multiple of 8" in call(p[0], 1, 2, 0, p[1], p[2])
    assert "max_frames" in call(p[0], 1, gpu_decoder.max_frames + 1, 800, p[1], p[2])
    assert "NULL" in call(None, 1, 2, 800, p[1], p[2])
    assert "NULL" in call(p[0], 1, 2, 800, None, p[2])
    assert "NULL" in call(p[0], 1, 2, 800, p[1], None)
    assert call(p[0], -1, 2, 800, p[1], p[2])
    good = st.copy()
    st["decimationIndex"][0] = 751
    assert "decimationIndex" in call(p[0], 1, 2, 800, p[1], p[2])
    # the device form reads the entry decimationIndex back and refuses it likewise; the device state stays as it was
    d_raw = torch.from_numpy(raw).cuda()
    d_st = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    d_iq = torch.full((iq.size * 4,), U.FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert "decimationIndex" in call(d_raw.data_ptr(), 1, 2, 800, d_st.data_ptr(), d_iq.data_ptr(), ft8.DEVICE_PTRS)
    assert "aligned" in call(d_raw.data_ptr() + 8, 1, 1, 792, d_st.data_ptr(), d_iq.data_ptr(), ft8.DEVICE_PTRS)
    gpu_decoder.synchronize()
    assert d_st.cpu().numpy().tobytes() == st.tobytes() and bool((d_iq == U.FILL).all())
    st[:] = good
    with pytest.raises(ft8.Ft8GpuError):
        gpu_decoder.rx_stream(raw[:, :, :2 * 796])
