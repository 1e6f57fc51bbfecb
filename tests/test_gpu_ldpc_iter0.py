"""Iteration 0 of the LDPC kernel stands in front of the BP loop (csrc/decode.hip): no check has sent a message yet, so the
three edges of a variable carry one value and fast_tanh runs on three values per lane, not nine; the loop starts at
iteration 1.  Every 48-byte status record of both kernel forms -- the counting form <true, 1> of the stage entry and the
pipeline form <false, 3> -- against ft8_decode of the oracle, byte for byte, with the fast divisions and with
FT8GPU_DBG_FORCE_IEEE_DIV (iteration 0 in the reference's own domain).

  * 3 synthesised frames at caps 1, 4, 5 and 9 (one block per frame, a full block, partial blocks) and 1, 2, 3 and 20
    iterations: at 1 the loop body never runs, at 2 it runs once.
  * One constructed frame (tests/osd_craft.py writes the cells that give a chosen vector of raw soft bits): soft bits that are
    all zero (variance 0: NaN LLRs), zeros among codeword bits (cwh = -0 where the loop's sums give +0; zero row products
    for the guard's exact test after iteration 1), candidates whose symbols lie before the first or behind the last block,
    codewords that are valid at iteration 0, and codewords with weak wrong bits that converge at iteration 1.
  * The launch order of the blocks: 65 and 130 frames at cap 120, and cap 1 (one block per frame), through the whole
    pipeline against the oracle's spot records."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOST_THREADS = 8
ITERS = (1, 2, 3, 20)


def _pipeline_view(want):
    """what the pipeline form reports: ldpc_errors 0 for a codeword and 83 otherwise, every other byte the same"""
    w = want.copy()
    e = w[:, :, 0:2].view(np.int16)
    e[e != 0] = 83
    return w


def _check_all_forms(oracle, ft8, dec, mag, cands, counts, iters, what):
    want = oracle.decode_candidates_batch(mag, cands, counts, iters, HOST_THREADS)
    pipe = _pipeline_view(want)
    total = int(counts.sum())
    for ieee in (0, ft8.DBG_FORCE_IEEE_DIV):
        for form, ref in ((0, want), (ft8.DBG_PIPELINE_FORM, pipe)):
            dec.set_debug_flags(ieee | form)
            try:
                st = dec.decode_candidates(mag, cands, counts)
            finally:
                dec.set_debug_flags(0)
            got = st.view(np.uint8).reshape(st.shape[0], st.shape[1], 48)
            bad = np.argwhere((got != ref).any(axis=2))
            print(f"{what} iters {iters} ieee {int(bool(ieee))} form {'pipeline' if form else 'counting'}: {len(bad)} of {total} records differ")
            assert len(bad) == 0, f"{what}, {iters} iterations, flags {ieee | form}: {len(bad)} of {total} records differ, first (frame, candidate) {tuple(bad[0])}"
    return want.reshape(want.shape[0], want.shape[1], 48).view(ft8.STATUS_DTYPE).reshape(want.shape[0], want.shape[1])


@pytest.fixture(scope="module")
def frames130():
    """130 synthesised frames of 20 signals, on the host"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B, S = 130, 20
    _, tones = workload.message_pool()
    with ft8.Decoder(device=0, max_frames=B) as dec:
        sig, _ = workload.frame_signals(810000, B, S, tones, snr_range=(-18.0, 0.0))
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, S, 1.0, workload.SEED_BASE + 43, iq, first_frame=810000)
        dec.synchronize()
        return iq.cpu().numpy()


@pytest.mark.parametrize("cap", [1, 4, 5, 9])
def test_three_frames_at_small_caps_and_iteration_caps(oracle, frames130, cap):
    import rtlsdr_ft8d_amd as ft8
    iq = frames130[:3]
    with ft8.Decoder(device=0, max_frames=3, max_candidates=cap) as dec:
        mag = dec.waterfall(iq)
        cands, counts = dec.find_sync(mag)
        assert (counts == cap).all()                                     # 20 signals a frame: every list is full
        for iters in ITERS:
            dec.set_params(ldpc_iters=iters)
            st = _check_all_forms(oracle, ft8, dec, mag, cands, counts, iters, f"3 frames cap {cap}")
            assert int(st["iters"].max()) <= iters
            if iters == 1:
                # the loop body never ran: a record is a codeword found by iteration 0, the all-zero exit, or the cap
                assert set(st["iters"].reshape(-1).tolist()) <= {0, 1}


# ---- constructed soft bits ---------------------------------------------------------------------------------------------------

def _constructed(oracle):
    """one frame: mag uint8 [94208], cands [CAP], and what each candidate is for"""
    import osd_craft as oc
    rng = np.random.default_rng(0x17E0)
    mag = np.zeros(oc.MAG_ARRAY, np.uint8)
    cands, names = [], []

    def add(v, name, time_offset=0):
        c = np.zeros((), oc.CAND_DTYPE)
        c["score"], c["time_offset"], c["freq_offset"] = 100 - len(cands), time_offset, 8 * len(cands)
        if v is not None:
            oc.write_candidate(mag, v, c)
        cands.append(c)
        names.append(name)

    strong = lambda: rng.integers(60, 256, 174)
    add(None, "all_zero")                                                # cells all 0: every raw soft bit 0, variance 0, NaN LLRs
    v = oc._signed(oc._codeword(rng), strong())
    v[rng.permutation(174)[:40]] = 0
    add(v, "zeros_among_codeword_bits")                                  # cwh = -0 on 40 variables; zero row products after iteration 0
    v = oc._signed(oc._codeword(rng), strong())
    v[0:174:3] = 0
    add(v, "every_third_zero")
    v = np.zeros(174, np.int16)
    v[5], v[70], v[140] = 9, -200, 1
    add(v, "three_nonzero")                                              # rows whose products are zero whichever member is left out
    for k in range(3):
        add(oc._signed(oc._codeword(rng), strong()), f"valid_at_0_{k}")
    rc, a77 = oracle.pack77("CQ K1ABC FN42")
    assert rc == 0
    add(oc._signed(oc._payload_codeword(np.unpackbits(a77)[:77]), strong()), "valid_at_0_crc")       # a real message: CRC and unpack77 run
    for k, nweak in enumerate((1, 2, 3)):
        cw = oc._codeword(rng)
        v = oc._signed(cw, rng.integers(150, 256, 174))
        at = rng.permutation(174)[:nweak]
        v[at] = np.where(cw[at] == 1, -(k + 1), k + 1)                    # wrong sign, magnitude 1 .. 3
        add(v, f"weak_wrong_bits_{nweak}")
    # symbols before block 0 / behind block 91 read as zeros (ft8_extract_likelihood)
    add(oc._signed(oc._codeword(rng), strong()), "blocks_before_the_waterfall", time_offset=-12)
    add(oc._signed(oc._codeword(rng), strong()), "blocks_behind_the_waterfall", time_offset=30)
    return mag, np.array(cands, oc.CAND_DTYPE), names


def test_constructed_soft_bits(oracle):
    import osd_craft as oc
    import rtlsdr_ft8d_amd as ft8
    mag, cands, names = _constructed(oracle)
    cap = len(cands)
    assert cap == 13 and cands.dtype == ft8.CAND_DTYPE                 # three full blocks and one wave of a fourth
    idx = {n: k for k, n in enumerate(names)}
    # the inputs are what they are named for
    raw = np.array([oracle.llr(mag, cands[k:k + 1], normalise=False) for k in range(cap)])
    assert not raw[idx["all_zero"]].any()
    assert (raw[idx["zeros_among_codeword_bits"]] == 0).sum() == 40 and (raw[idx["every_third_zero"]] == 0).sum() >= 58
    assert np.isnan(oracle.llr(mag, cands[0:1])).all()
    for n, to in (("blocks_before_the_waterfall", -12), ("blocks_behind_the_waterfall", 30)):
        outside = [k for k in range(58) if not 0 <= to + oc.sym_of(k) < oc.NBLOCKS]
        assert len(outside) >= 5 and all(not raw[idx[n], 3 * k:3 * k + 3].any() for k in outside) and raw[idx[n]].any()
    mag, cands, counts = mag[None, :], cands[None, :], np.array([cap], np.int32)
    with ft8.Decoder(device=0, max_frames=1, max_candidates=cap) as dec:
        for iters in ITERS:
            dec.set_params(ldpc_iters=iters)
            st = _check_all_forms(oracle, ft8, dec, mag, cands, counts, iters, "constructed frame")[0]
            for n in names:
                if n.startswith("valid_at_0"):                           # found by iteration 0 itself
                    assert st[idx[n]]["ldpc_errors"] == 0 and st[idx[n]]["iters"] == 0, (n, st[idx[n]])
                if n.startswith("weak_wrong_bits") and iters >= 2:     # iteration 0 fails the check, iteration 1 finds the codeword
                    assert st[idx[n]]["ldpc_errors"] == 0 and st[idx[n]]["iters"] == 1, (n, st[idx[n]])
                if n.startswith("weak_wrong_bits") and iters == 1:
                    assert st[idx[n]]["ldpc_errors"] > 0 and st[idx[n]]["iters"] == 1, (n, st[idx[n]])
            assert st[idx["valid_at_0_crc"]]["ok"] == 1 and st[idx["valid_at_0_crc"]]["text"] == b"CQ K1ABC FN42"
            assert st[idx["all_zero"]]["iters"] == 0 and st[idx["all_zero"]]["ldpc_errors"] == 83      # the all-zero word ends it
            if iters == 20:
                assert st[idx["zeros_among_codeword_bits"]]["iters"] >= 1 and st[idx["every_third_zero"]]["iters"] >= 1


# ---- launch order ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nframes,cap", [(65, 120), (130, 120), (130, 1)])
def test_every_frame_keeps_its_records_whatever_the_block_order(oracle, frames130, nframes, cap):
    """the mapping block -> (frame, group of four candidates) only places work: 65 frames x 30 blocks and 130 x 30 have a
    remainder for the XCD renumbering and several groups per XCD; cap 1 is one block per frame"""
    import rtlsdr_ft8d_amd as ft8
    iq = frames130[:nframes]
    with ft8.Decoder(device=0, max_frames=nframes, max_candidates=cap) as dec:
        gdec, gn = dec.decode_batch(iq)
    rdec, rn = oracle.subsystem_batch(iq, oracle.default_params(10, cap, 20), HOST_THREADS)
    bad = [k for k in range(nframes) if gn[k] != rn[k] or gdec[k].tobytes() != rdec[k].tobytes()]
    print(f"{nframes} frames cap {cap}: {int(gn.sum())} messages, {len(bad)} frames differ")
    assert not bad, f"{len(bad)} of {nframes} frames differ from the oracle, first {bad[0]}"
    assert int(gn.sum()) > (2 * nframes if cap == 120 else 0)          # real decodes were compared
