"""The BP loop of the LDPC kernel after the instructions that were not the reference's arithmetic left it (csrc/decode.hip:
no zeroing of the third variable's states on lanes that have none, no select in front of the guard, no guard after
iteration 0, row-product broadcasts as operand modifiers): every 48-byte status record of both kernel forms -- the counting
form <true, 1> of the stage entry and the pipeline form <false, 3> -- against ft8_decode of the oracle, byte for byte, with the
fast divisions and with FT8GPU_DBG_FORCE_IEEE_DIV.

Shape 1: 65 frames, so that there are several groups of blocks and a remainder for the XCD renumbering (cap 120: 1950 blocks,
cap 5: 130 blocks of which one wave in four is idle), at 1, 2 and 20 iterations (the loop leaves after the first hard decision,
after one guard-less iteration, and runs the guard for real).
Shape 2: 8 frames whose LLRs are exactly zero in large numbers -- low-level noise that the waterfall quantises to a few distinct
bytes, and constant input -- so that zero messages and zero row products occur in iterations 0 and 1: what the skipped guard
of iteration 0 and the exact key test of iteration 1 are about."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOST_THREADS = 8


def _pipeline_view(want):
    """what the pipeline form reports: ldpc_errors 0 for a codeword and 83 otherwise, every other byte the same"""
    w = want.copy()
    e = w[:, :, 0:2].view(np.int16)
    e[e != 0] = 83
    return w


def _records(dec, ft8, mag, cands, counts, flags):
    dec.set_debug_flags(flags)
    try:
        st = dec.decode_candidates(mag, cands, counts)
    finally:
        dec.set_debug_flags(0)
    return st.view(np.uint8).reshape(st.shape[0], st.shape[1], 48)


def _check_all_forms(oracle, ft8, dec, mag, cands, counts, iters, what):
    want = oracle.decode_candidates_batch(mag, cands, counts, iters, HOST_THREADS)
    pipe = _pipeline_view(want)
    total = int(counts.sum())
    for ieee in (0, ft8.DBG_FORCE_IEEE_DIV):
        for form, ref in ((0, want), (ft8.DBG_PIPELINE_FORM, pipe)):
            got = _records(dec, ft8, mag, cands, counts, ieee | form)
            bad = np.argwhere((got != ref).any(axis=2))
            print(f"{what} iters {iters} ieee {int(bool(ieee))} form {'pipeline' if form else 'counting'}: "
                  f"{len(bad)} of {total} records differ")
            assert len(bad) == 0, f"{what}, {iters} iterations, flags {ieee | form}: {len(bad)} of {total} records differ, first (frame, candidate) {tuple(bad[0])}"
    return want


@pytest.fixture(scope="module")
def traffic65():
    """65 synthesised frames of 20 signals and their waterfalls (the candidate lists depend on the cap)"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B, S = 65, 20
    _, tones = workload.message_pool()
    with ft8.Decoder(device=0, max_frames=B) as dec:
        sig, _ = workload.frame_signals(770000, B, S, tones, snr_range=(-18.0, 0.0))
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, S, 1.0, workload.SEED_BASE + 21, iq, first_frame=770000)
        dec.synchronize()
        mag = dec.waterfall(iq.cpu().numpy())
    return mag


@pytest.mark.parametrize("cap", [5, 120])
def test_every_record_of_65_frames_in_both_forms_and_both_divisions(oracle, traffic65, cap):
    import rtlsdr_ft8d_amd as ft8
    mag = traffic65
    B = mag.shape[0]
    with ft8.Decoder(device=0, max_frames=B, max_candidates=cap) as dec:
        cands, counts = dec.find_sync(mag)
        assert int(counts.sum()) > 0.9 * B * cap                     # the lists are (nearly) full: every block has work
        for iters in (1, 2, 20):
            dec.set_params(ldpc_iters=iters)
            want = _check_all_forms(oracle, ft8, dec, mag, cands, counts, iters, f"65 frames cap {cap}")
            st = want.reshape(-1, 48).view(ft8.STATUS_DTYPE).reshape(-1)
            if iters == 20:
                assert int((st["ok"] == 1).sum()) > (2 if cap == 5 else 8) * B          # real decodes were compared
                if cap == 120:                                                        # (the five strongest decode at once)
                    assert len(set(st["iters"].tolist())) > 5                         # ... and left the loop at many different iterations


def test_every_record_of_frames_with_exactly_zero_llrs(oracle):
    import rtlsdr_ft8d_amd as ft8
    rng = np.random.default_rng(2024)
    levels = [2e-6, 3e-6, 5e-6, 7e-6, 1e-5, 1.5e-5, 3e-5]              # the quantiser's floor: 2 .. about 30 distinct bytes
    iq = np.stack([rng.normal(0, s, (2, ft8.NSAMPLES)).astype(np.float32) for s in levels]
                  + [np.full((2, ft8.NSAMPLES), 0.25, np.float32)])
    B, cap = iq.shape[0], 120
    assert B == 8
    with ft8.Decoder(device=0, max_frames=B, max_candidates=cap, min_score=-32768) as dec:
        mag = dec.waterfall(iq)
        cands, counts = dec.find_sync(mag)
        assert (counts == cap).all()
        # the inputs are what the test is about: exactly-zero LLRs in large numbers, beside candidates that have none or only zeros
        zeros = np.array([[int((oracle.llr(mag[k], cands[k, c:c + 1], normalise=False) == 0).sum()) for c in range(cap)] for k in range(B)])
        assert zeros.sum() > 0.2 * B * cap * 174, zeros.sum()
        assert ((zeros > 0) & (zeros < 174)).sum() > 0.5 * B * cap and (zeros == 174).any()
        for iters in (20, 2, 1):
            dec.set_params(ldpc_iters=iters)
            want = _check_all_forms(oracle, ft8, dec, mag, cands, counts, iters, "zero-LLR frames")
            if iters == 20:
                st = want.reshape(-1, 48).view(ft8.STATUS_DTYPE).reshape(-1)
                assert (st["iters"] >= 2).sum() > 0.5 * B * cap                        # the guard after iteration 1 saw these products
