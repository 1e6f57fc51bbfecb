"""The dB quantiser of the waterfall kernel (csrc/quant_math.h) against the reference expression on EVERY float, and all
256 byte values through the real kernel.

The kernel does not evaluate (int)(2*(10.0f*log10f(1e-12f + mag2*4.0f/(NFFT*NFFT)))+240) (rtlsdr_ft8d.c:1415-1427): it takes a
v_log_f32 guess, one compare against a host-built threshold table and a single scaling.  The parity tests reach it only through
FFT outputs of radio-like frames, where a cell on a threshold is a 1e-7 event and most bytes below 44 never occur.  Here:
  * ft8gpu_selftest_quantiser walks every |X|^2 bit pattern (0 .. +inf, every NaN) through the kernel's own functions and
    the context's uploaded table and returns the step function; the oracle's ft8o_quantise_steps returns the step function of
    the reference expression with this machine's libm.  Equal step lists and equal q(0) are equality on every float.
  * the uploaded table itself is held against the oracle's steps;
  * a gain sweep over 9 decades puts every byte 0..255 through the waterfall kernel in its three forms.
Measured on one MI355X box: the device walk (2^31 + 2^24 patterns, three pair evaluations each) takes 6.0 ms (host clock
around the call), the oracle's scan of 2^31 patterns 0.79 s on 16 threads there (7.4 s on 8 threads of a CPU box); the six tests
together 3.2 s.  The result was the guess for 2 152 073 232 patterns and the guess + 1 for 3 799 023."""
import ctypes as C
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POS_INF, N_ORDERED, N_NAN = 0x7F800000, 0x7F800001, 2 * 0x7FFFFF
NTHREADS = min(16, len(os.sched_getaffinity(0)))


def as_float(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def oracle_steps(oracle):
    """the reference expression's step function over 0 .. +inf (2^31 log10f calls: computed once), q(0), and its NaN behaviour"""
    t0 = time.time()
    bits, val, n, down = oracle.quantise_steps(0, POS_INF, NTHREADS)
    seconds = time.time() - t0
    q = oracle.lib().ft8o_quantise
    nan_steps = [oracle.quantise_steps(lo, lo + 0x7FFFFE, NTHREADS)[2] for lo in (0x7F800001, 0xFF800001)]
    nan_first = [q(float(as_float([lo])[0])) for lo in (0x7F800001, 0xFF800001)]
    print(f"oracle scan of 0 .. +inf: {seconds:.2f} s on {NTHREADS} threads, {n} steps, {down} of them down")
    # what the CPU test of the oracle asserts; here it is the premise of every comparison below
    assert n == 255 and down == 0 and np.array_equal(val, np.arange(1, 256)) and q(0.0) == 0
    assert nan_steps == [0, 0] and nan_first == [0, 0]                    # every NaN -> 0
    for a in (bits, val):
        a.setflags(write=False)
    return dict(bits=bits, val=val, n=n, q0=q(0.0), seconds=seconds)


@pytest.fixture(scope="module")
def device_walk(gpu_decoder):
    gpu_decoder.selftest_quantiser()                                      # first launch: code object load
    gpu_decoder.synchronize()
    t0 = time.time()
    r = gpu_decoder.selftest_quantiser()
    print(f"device walk: {1e3 * (time.time() - t0):.1f} ms (host clock around the call, which ends in a stream synchronise)")
    return r


def test_device_step_function_equals_the_reference_expression_on_every_float(oracle_steps, device_walk):
    """Every float 0 .. +inf and every NaN through the kernel's quantiser, in both slots of the pair and beside hashed partners:
    the device's ordered step list must be the oracle's -- same bit patterns, same values -- with the same q(0) and every NaN
    quantised to 0; no evaluation of a pattern may disagree with another, and both branches of the compare (result = guess,
    result = guess + 1) must have been taken."""
    r = device_walk
    print({k: v for k, v in r.items() if not isinstance(v, np.ndarray)})
    assert r["n_steps"] == oracle_steps["n"] == len(r["steps_bits"]), (r["n_steps"], hex(r["first_bad"]))     # no overflow of the list
    differ = np.flatnonzero((r["steps_bits"] != oracle_steps["bits"]) | (r["steps_val"] != oracle_steps["val"]))
    assert differ.size == 0, [(int(k), hex(r["steps_bits"][k]), hex(oracle_steps["bits"][k])) for k in differ[:5]]
    assert r["q0"] == oracle_steps["q0"] == 0
    assert r["nan_nonzero"] == 0, hex(r["first_bad"])
    assert r["disagree"] == 0, hex(r["first_bad"])
    assert r["first_bad"] == 0
    assert r["from_guess"] > 0 and r["from_guess_plus_1"] > 0
    assert r["from_guess"] + r["from_guess_plus_1"] == N_ORDERED + N_NAN                       # every pattern of the domain, once


def test_uploaded_threshold_table_sits_on_the_reference_steps(oracle_steps, device_walk):
    """qthr[k] as it lies on the device against the oracle's k-th step b_k in |X|^2: with y(m) = m * 2^-18 + 1e-12 in float32,
    qthr[k] <= y(b_k) and qthr[k] > y(b_k - 1) -- the table (bisection, +-64 neighbours and 200 000 samples at create time) on
    exactly the floats where it decides."""
    thr = device_walk["qthr"]
    assert thr.dtype == np.float32 and thr.shape == (256,) and thr[0] == 0
    b = oracle_steps["bits"]
    assert np.array_equal(oracle_steps["val"], np.arange(1, 256))         # b[k - 1] is the step to k

    def y(bits):
        return as_float(bits) * np.float32(2.0 ** -18) + np.float32(1e-12)
    y_at, y_below = y(b), y(b - np.uint32(1))
    assert y_at.dtype == np.float32
    bad = np.flatnonzero(~((thr[1:] <= y_at) & (thr[1:] > y_below)))
    assert bad.size == 0, [(int(k) + 1, float(thr[k + 1]), float(y_below[k]), float(y_at[k])) for k in bad[:5]]


@pytest.fixture(scope="module")
def sweep(oracle):
    """one noise frame at 16 gains, 0.6 decades apart from 1e-6 to 1e3: the oracle's waterfalls contain every byte value"""
    base = np.random.default_rng(2026).normal(0, 1, (2, 48000)).astype(np.float32)
    iq = np.stack([base * np.float32(10 ** (-6 + 0.6 * k)) for k in range(16)])
    assert iq.dtype == np.float32
    mags = oracle.waterfall_batch(iq, nthreads=NTHREADS)
    dec, n = oracle.subsystem_batch(iq, nthreads=NTHREADS)
    for a in (iq, mags, dec, n):
        a.setflags(write=False)
    return iq, mags, dec, n


@pytest.mark.parametrize("form", ["rows", "ab-rows", "ab-lds"])
def test_gain_sweep_puts_every_byte_through_the_kernel(sweep, form):
    """all 256 byte values through the real waterfall kernel -- the product library, the A/B build's product form and its LDS
    form -- bit-identical to the oracle, and the spots decoded from them as well"""
    import rtlsdr_ft8d_amd as ft8
    iq, mags, rdec, rn = sweep
    hist = np.bincount(mags.ravel(), minlength=256)
    print(f"rarest byte {int(hist.argmin())} occurs {int(hist.min())} times; {int(hist[0])} zeros, {int(hist[255])} of 255")
    assert (hist > 0).all(), np.flatnonzero(hist == 0)                   # a narrow input cannot pass
    lib = None if form == "rows" else ft8.load_ab_library()
    with ft8.Decoder(device=0, max_frames=16, lib=lib) as d:
        if form == "ab-lds":
            d.set_debug_flags(ft8.AB_WATERFALL_LDS)
        mag = d.waterfall(iq)
        dec, n = d.decode_batch(iq)
    for k in range(16):
        diff = np.flatnonzero(mag[k] != mags[k])
        assert diff.size == 0, f"{form} frame {k}: {diff.size} cells differ, first {diff[:5]}: {mag[k][diff[:5]]} vs {mags[k][diff[:5]]}"
    for k in range(16):
        assert n[k] == rn[k] and dec[k].tobytes() == rdec[k].tobytes(), (form, k)


def test_selftest_quantiser_refuses_null_outputs_and_leaves_the_others_alone(gpu_decoder):
    d = gpu_decoder
    f = d.lib.ft8gpu_selftest_quantiser

    def fresh():
        return [np.full(7, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(64, 0xDEADBEEF, np.uint32), np.full(64, 0x5A, np.uint8),
                np.full(256, -7.5, np.float32)]
    for missing in range(4):
        bufs = fresh()
        ptrs = [None if k == missing else a.ctypes.data for k, a in enumerate(bufs)]
        assert f(d.h, ptrs[0], ptrs[1], ptrs[2], 64, ptrs[3]) == -1
        assert b"NULL argument" in d.lib.ft8gpu_last_error()
        for a, b in zip(bufs, fresh()):
            assert np.array_equal(a, b)
    for cap in (0, -1):
        bufs = fresh()
        assert f(d.h, bufs[0].ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data, cap, bufs[3].ctypes.data) == -1
        assert b"cap" in d.lib.ft8gpu_last_error()
        for a, b in zip(bufs, fresh()):
            assert np.array_equal(a, b)
    bufs = fresh()
    assert f(None, bufs[0].ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data, 64, bufs[3].ctypes.data) == -1
    assert b"ctx is NULL" in d.lib.ft8gpu_last_error()
    # a list that does not fit shows: the true count comes back, only cap entries are written
    bufs = fresh()
    assert f(d.h, bufs[0].ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data, 10, bufs[3].ctypes.data) == 0
    assert bufs[0][0] == 255 and np.array_equal(bufs[2][:10], np.arange(1, 11)) and (bufs[1][10:] == 0xDEADBEEF).all() and (bufs[2][10:] == 0x5A).all()
