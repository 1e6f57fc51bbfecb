"""GPU parity tests: the HIP path (through the C ABI of libft8gpu.so) against the CPU oracle on the
same inputs.  Bit-exact at every stage boundary:
  waterfall uint8 (float path: FFT order + quantiser thresholds are shared by construction),
  sync scores / candidate list (integer), LLR+BP status incl. the packed 91 bits (float BP with
  identical operation order, -ffp-contract=off on both sides), CRC, text, spot records.
north_star's float tolerance for sync scores (1e-4) is moot: scores are integers and compared exactly.
"""
import os

import numpy as np
import pytest

import synth_util as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAG = 94208


@pytest.fixture(scope="module")
def frames(oracle):
    """a small zoo of frames: reference self-test, seeded multi-signal frames, degenerate inputs"""
    enc = S.oracle_encode_fn(oracle)
    out = []
    i, q = oracle.selftest_signal()
    out.append(("selftest", np.stack([i, q])))
    for seed, nsig, snr in [(11, 1, (-5, 0)), (12, 5, (-15, 0)), (13, 20, (-18, 0)), (14, 40, (-18, 0)),
                            (15, 60, (-24, -14)), (16, 12, (-10, 5))]:
        iq, _ = S.make_frame(seed, nsig, enc, snr_range=snr, cq_fraction=0.7)
        out.append((f"synth{seed}", iq))
    rng = np.random.default_rng(99)
    out.append(("zeros", np.zeros((2, 48000), np.float32)))
    out.append(("noise_only", (rng.normal(0, 0.15, (2, 48000))).astype(np.float32)))
    imp = np.zeros((2, 48000), np.float32)
    imp[0, 1234] = 0.5
    imp[1, 40000] = -0.5
    out.append(("impulses", imp))
    t = np.arange(48000) / 3200.0
    tone = np.stack([0.5 * np.cos(2 * np.pi * 700.0 * t), 0.5 * np.sin(2 * np.pi * 700.0 * t)]).astype(np.float32)
    out.append(("carrier", tone))
    out.append(("fullscale", rng.uniform(-0.5, 0.5, (2, 48000)).astype(np.float32)))
    out.append(("tiny", (rng.normal(0, 1e-9, (2, 48000))).astype(np.float32)))
    out.append(("huge", (rng.normal(0, 50.0, (2, 48000))).astype(np.float32)))
    # two frames of on-air style traffic (workload.mixed_message_pool: reports, RR73 / RRR / 73, bare calls, R grid, /R /P,
    # hashed calls, type 4, free text, telemetry, payloads unpack77 refuses), one message heard twice in each: every stage
    # test below -- waterfall, scores, candidate lists, per-candidate status AND TEXT at 1 / 7 / 20 / 50 iterations, spot
    # records -- also runs on messages that are not CQ calls and come out of noise
    from rtlsdr_ft8d_amd import workload
    texts, tones = workload.message_pool(traffic="mixed")
    for seed, nsig, snr in [(17, 20, (-16, 0)), (18, 45, (-20, -4))]:
        out.append((f"mixed{seed}", S.make_mixed_frame(seed, nsig, snr, texts, tones)[0]))
    assert len(out) == 16                              # the gpu_decoder fixture holds 16 frames
    return out


@pytest.fixture(scope="module")
def oracle_mags(oracle, frames):
    return np.stack([oracle.waterfall(iq[0], iq[1]) for _, iq in frames])


def test_waterfall_bit_exact(oracle, gpu_decoder, frames, oracle_mags):
    iq = np.stack([f for _, f in frames])
    mag = gpu_decoder.waterfall(iq)
    for k, (name, _) in enumerate(frames):
        diff = np.flatnonzero(mag[k] != oracle_mags[k])
        assert diff.size == 0, f"{name}: {diff.size} cells differ, first {diff[:5]}"


def test_waterfall_nonfinite_and_overflowing_samples(oracle, gpu_decoder):
    """inf, NaN and FLT_MAX samples: |X|^2 overflows or is NaN.  The reference's (int) conversion is
    undefined there; the fence (oracle ft8o_quantise) is 255 for +inf and 0 for NaN, and a
    saturated cell must not leak into its neighbour (the packed 16-bit store of the kernel).
    NOT a parity claim: the reference as built on x86 yields 0 for +inf (ft8o_quantise_x86); this test pins the
    product to the fenced definition, and tests/test_oracle.py pins how the two definitions differ."""
    rng = np.random.default_rng(7)
    fmax = np.finfo(np.float32).max
    frames = []
    for special in ([np.inf], [np.nan], [fmax, -fmax], [np.inf, -np.inf, np.nan, fmax, 1e30, -1e25]):
        iq = rng.normal(0, 0.1, (2, 48000)).astype(np.float32)
        pos = rng.integers(0, 48000, 12)
        for j, p_ in enumerate(pos):
            iq[j & 1, p_] = special[j % len(special)]
        frames.append(iq)
    big = rng.normal(0, 1e18, (2, 48000)).astype(np.float32)      # every |X|^2 overflows to +inf, nothing is NaN
    frames.append(big)
    iq = np.stack(frames)
    mag = gpu_decoder.waterfall(iq)
    for k in range(iq.shape[0]):
        ref = oracle.waterfall(iq[k, 0], iq[k, 1])
        diff = np.flatnonzero(mag[k] != ref)
        assert diff.size == 0, f"frame {k}: {diff.size} cells differ, first {diff[:5]}"
    assert (mag[4] == 255).all()
    dec, n = gpu_decoder.decode_batch(iq)                          # the rest of the path takes any bytes
    for k in range(iq.shape[0]):
        rdec, rn = oracle.subsystem(iq[k, 0], iq[k, 1])
        assert n[k] == rn and dec[k].tobytes() == rdec.tobytes()


def test_waterfall_close_to_float64_truth(oracle, gpu_decoder, frames):
    """the float32 R4DIF FFT vs a float64 FFT: at most a handful of +-1 quantiser flips"""
    iq = np.stack([f for _, f in frames[:5]])
    mag = gpu_decoder.waterfall(iq)
    for k in range(iq.shape[0]):
        truth = oracle.waterfall(iq[k, 0], iq[k, 1], f64=True)
        d = mag[k].astype(int) - truth.astype(int)
        assert np.abs(d).max() <= 1
        assert np.count_nonzero(d) <= 1e-4 * MAG + 2       # flip-rate tolerance 1e-4


def test_score_map_exact(oracle, gpu_decoder, oracle_mags):
    s = gpu_decoder.score_map(oracle_mags)
    for k in range(oracle_mags.shape[0]):
        ref = oracle.score_map(oracle_mags[k])
        assert np.array_equal(s[k], ref), f"frame {k}: {np.count_nonzero(s[k] != ref)} scores differ"


@pytest.mark.parametrize("max_candidates,min_score", [(120, 10), (8, 10), (33, 5), (480, 10), (120, 0), (1000, -5), (120, 1), (60, 40),
                                                      (120, 300), (120, 32767), (64, -32768)])   # incl. thresholds beyond any numerator
def test_find_sync_exact(oracle, gpu_decoder, oracle_mags, max_candidates, min_score):
    gpu_decoder.set_params(min_score=min_score, max_candidates=max_candidates, ldpc_iters=20)
    try:
        cands, counts = gpu_decoder.find_sync(oracle_mags)
        for k in range(oracle_mags.shape[0]):
            ref = oracle.find_sync(oracle_mags[k], max_candidates, min_score)
            assert counts[k] == len(ref), f"frame {k}: count {counts[k]} vs {len(ref)}"
            assert np.array_equal(cands[k, :counts[k]], ref), f"frame {k}: candidate list differs"
            assert not cands[k, counts[k]:].view(np.uint64).any()
    finally:
        gpu_decoder.set_params(min_score=10, max_candidates=120, ldpc_iters=20)


def _oracle_status(oracle, mag, cands, iters):
    return [oracle.decode(mag, cands[c:c + 1], iters) for c in range(len(cands))]


def _compare_status(name, st, ref):
    for c, r in enumerate(ref):
        g = st[c]
        where = f"{name} cand {c}"
        assert g["ldpc_errors"] == r["ldpc_errors"], where
        assert g["iters"] == r["iters"], where
        assert bytes(g["a91"]) == r["a91"], where
        assert bool(g["ok"]) == r["ok"], where
        if r["ldpc_errors"] == 0:
            assert g["crc_extracted"] == r["crc_extracted"] and g["crc_calculated"] == r["crc_calculated"], where
            if r["crc_extracted"] == r["crc_calculated"]:
                assert g["unpack_status"] == r["unpack_status"], where
        if r["ok"]:
            assert g["text"].decode() == r["text"], where


@pytest.mark.parametrize("iters", [20, 1, 7, 50])
def test_decode_candidates_exact(oracle, gpu_decoder, frames, oracle_mags, iters):
    gpu_decoder.set_params(ldpc_iters=iters)
    try:
        B = oracle_mags.shape[0]
        cands = np.zeros((B, 120), gpu_decoder.find_sync(oracle_mags[:1])[0].dtype)
        counts = np.zeros(B, np.int32)
        for k in range(B):
            ref = oracle.find_sync(oracle_mags[k], 120, 10)
            cands[k, :len(ref)] = ref
            counts[k] = len(ref)
        st = gpu_decoder.decode_candidates(oracle_mags, cands, counts)
        nconv = 0
        texts = set()
        for k in range(B):
            ref = _oracle_status(oracle, oracle_mags[k], cands[k, :counts[k]], iters)
            _compare_status(frames[k][0], st[k], ref)
            nconv += sum(r["ok"] for r in ref)
            texts |= {r["text"] for r in ref if r["ok"]}
        if iters >= 20:
            assert nconv > 20          # the comparison exercised real decodes
            # ... of messages that are not CQ calls, out of noise (the mixed-traffic frames): reports, acknowledgements, hashed calls
            other = {t for t in texts if not t.startswith("CQ")}
            assert len(other) >= 15 and any(" R-" in t or " R+" in t for t in other) and any(t.rstrip().endswith("73") for t in other), sorted(other)[:40]
    finally:
        gpu_decoder.set_params(ldpc_iters=20)


def test_decode_degenerate_waterfalls(oracle, gpu_decoder):
    """constant waterfall (LLR variance 0 -> NaN path), random bytes, saturated bytes, edge offsets"""
    rng = np.random.default_rng(5)
    mags = np.stack([
        np.full(MAG, 100, np.uint8),
        rng.integers(0, 256, MAG, dtype=np.uint8),
        np.full(MAG, 255, np.uint8),
        rng.integers(0, 2, MAG, dtype=np.uint8) * 255,
    ])
    cd = gpu_decoder.find_sync(mags[:1])[0].dtype
    cands = np.zeros((4, 120), cd)
    counts = np.full(4, 120, np.int32)
    for k in range(4):
        for c in range(120):
            cands[k, c] = (rng.integers(-50, 200), rng.integers(-12, 24), rng.integers(0, 249),
                           rng.integers(0, 2), rng.integers(0, 2))
    cands[:, 0] = (30, -12, 0, 0, 0)
    cands[:, 1] = (30, 23, 248, 1, 1)
    st = gpu_decoder.decode_candidates(mags, cands, counts)
    for k in range(4):
        ref = _oracle_status(oracle, mags[k], cands[k], 20)
        _compare_status(f"degenerate{k}", st[k], ref)


def test_unpack_all_message_types(oracle, gpu_decoder):
    """feed hand-built codewords of every message type through decode_candidates by painting them
    into a waterfall: exercises device unpack77 branches (free text, telemetry, /R /P, hashed,
    CQ nnn, CQ aaaa, non-standard, reports, failures) against the oracle's."""
    rng = np.random.default_rng(77)
    payloads = []
    # standard type 1 KAT + random type 1/2 payloads with assorted fields
    rc, kat = oracle.pack77("CQ K1JT FN20QI")
    payloads.append(bytes(kat[:10]))
    for _ in range(150):
        p = bytearray(rng.integers(0, 256, 10, dtype=np.uint8).tobytes())
        p[9] &= 0xF8
        i3 = int(rng.choice([0, 1, 2, 3, 4, 5, 1, 1, 2, 4, 0]))
        p[9] = (p[9] & 0xC0) | (i3 << 3)
        if i3 == 0:                      # force n3 in {0, 5, other}
            n3 = int(rng.choice([0, 5, 1, 0, 5]))
            p[8] = (p[8] & 0xFE) | ((n3 >> 2) & 1)
            p[9] = (p[9] & 0x3F) | ((n3 & 3) << 6)
        if i3 in (1, 2) and rng.random() < 0.6:
            # special tokens / small n28 so that DE QRZ CQ, CQ nnn, CQ aaaa and hashed calls appear
            n28 = int(rng.choice([0, 1, 2, 3, 500, 1002, 1003, 20000, 532443, 532444, 2063591, 2063592, 3000000,
                                  6257895, 6257896, 10222009]))
            n29 = (n28 << 1) | int(rng.integers(0, 2))
            p[0] = (n29 >> 21) & 0xFF
            p[1] = (n29 >> 13) & 0xFF
            p[2] = (n29 >> 5) & 0xFF
            p[3] = (p[3] & 0x07) | ((n29 << 3) & 0xF8)
        if i3 in (1, 2) and rng.random() < 0.5:
            ig = int(rng.choice([0, 10320, 32400, 32401, 32402, 32403, 32404, 32405, 32430, 32435, 32470, 32767]))
            p[7] = (p[7] & 0xE0) | ((ig >> 10) & 0x1F)
            p[8] = (ig >> 2) & 0xFF
            p[9] = (p[9] & 0x3F) | ((ig & 3) << 6)
        payloads.append(bytes(p))
    # messages of every kind from the independent encoder (tests/ft8_spec_pack.py, written from the published protocol)
    import ft8_spec_pack as P
    payloads += [P.pack_standard("K1ABC", "W9XYZ", x) for x in ("EN37", "R EN37", "-11", "R+07", "RRR", "RR73", "73", "")]
    payloads += [P.pack_standard("K1ABC/R", "W9XYZ", "EN37", i3=1), P.pack_standard("G4ABC", "PA9XYZ/P", "JO22", i3=2),
                 P.pack_standard("CQ 123", "DL1ABC", "JO62"), P.pack_standard("CQ DX", "VK3ABC", "QF22"),
                 P.pack_standard("CQ TEST", "9A1A", "JN75"), P.pack_standard("QRZ", "JA1XYZ", "PM95"), P.pack_standard("DE", "3D2AG", "RH91")]
    payloads += [P.pack_free_text(t) for t in ("TNX BOB 73 GL", "A", "+-./?0123 ZY", "HELLO WORLD")]
    payloads += [P.pack_telemetry("0123456789ABCDEF01"), P.pack_telemetry("7FFFFFFFFFFFFFFFFF")]
    payloads += [P.pack_nonstandard("PJ4/K1ABC", 1234, icq=1), P.pack_nonstandard("YW18FIFA", 77, flip=0, nrpt=2),
                 P.pack_nonstandard("KH1/KH7Z", 4095, flip=1, nrpt=3), P.pack_nonstandard("W9XYZ/QRP", 0, flip=1, nrpt=0)]
    n = len(payloads)
    # paint each codeword as a clean signal into its own waterfall at time_offset 0 / freq_offset 10
    mags = np.full((n, 92, 2, 2, 256), 60, np.uint8)
    for k, p in enumerate(payloads):
        tones = oracle.encode(np.frombuffer(p + b"\0\0", np.uint8))
        for s, tnum in enumerate(tones):
            mags[k, s, 0, 0, 10 + int(tnum)] = 160
    mags = mags.reshape(n, MAG)
    cd = gpu_decoder.find_sync(mags[:1])[0].dtype
    cands = np.zeros((n, 120), cd)
    cands[:, 0] = (40, 0, 10, 0, 0)
    counts = np.ones(n, np.int32)
    # process in chunks that fit the fixture's max_frames
    texts = set()
    for a in range(0, n, 16):
        st = gpu_decoder.decode_candidates(mags[a:a + 16], cands[a:a + 16], counts[a:a + 16])
        for k in range(st.shape[0]):
            ref = oracle.decode(mags[a + k], cands[a + k, :1], 20)
            _compare_status(f"payload{a + k}", st[k], [ref])
            assert ref["ldpc_errors"] == 0
            if ref["ok"]:
                texts.add(ref["text"].split(" ")[0][:3])
    assert len(texts) >= 6            # several distinct message shapes were produced


def test_unpack_randomised_payload_sweep(oracle):
    """6000 random 77-bit payloads -- uniformly random bits, and random bits with every i3 / n3 type, the special n28
    tokens and the grid / report codes forced in -- painted 24 to a frame and decoded through the pipeline form's
    neighbour (ft8gpu_decode_candidates): status, CRC, unpack return code and text of every one against the oracle.
    (Round 4 rewrote the device unpack77 on two 64-bit words and an LDS work area: no byte array, no scratch.)"""
    import rtlsdr_ft8d_amd as ft8
    rng = np.random.default_rng(2026)
    per_frame, nframes = 24, 250
    n = per_frame * nframes
    payloads = rng.integers(0, 256, (n, 10), dtype=np.uint8)
    payloads[:, 9] &= 0xF8
    forced = rng.random(n) < 0.7
    i3 = rng.choice([0, 0, 1, 1, 1, 2, 2, 3, 4, 4, 5, 6, 7], n)
    payloads[forced, 9] = (payloads[forced, 9] & 0xC0) | (i3[forced] << 3).astype(np.uint8)
    tokens = np.array([0, 1, 2, 3, 4, 500, 1002, 1003, 1004, 20000, 532443, 532444, 2063591, 2063592, 2063593, 3000000,
                       6257895, 6257896, 6257897, 10222009, 268435455], np.int64)
    grids = np.array([0, 1, 17, 10320, 32399, 32400, 32401, 32402, 32403, 32404, 32405, 32406, 32430, 32435, 32436, 32470, 32767], np.int64)
    for k in np.nonzero(forced)[0]:
        p = payloads[k]
        t = int(i3[k])
        if t == 0:
            n3 = int(rng.choice([0, 5, 0, 5, 1, 2, 3, 4, 6, 7]))
            p[8] = (p[8] & 0xFE) | ((n3 >> 2) & 1)
            p[9] = (p[9] & 0x3F) | ((n3 & 3) << 6)
        if t in (1, 2):
            if rng.random() < 0.5:
                n29 = (int(rng.choice(tokens)) << 1) | int(rng.integers(0, 2))
                p[0], p[1], p[2] = (n29 >> 21) & 0xFF, (n29 >> 13) & 0xFF, (n29 >> 5) & 0xFF
                p[3] = (p[3] & 0x07) | ((n29 << 3) & 0xF8)
            if rng.random() < 0.5:
                n29 = (int(rng.choice(tokens)) << 1) | int(rng.integers(0, 2))
                p[3] = (p[3] & 0xF8) | ((n29 >> 26) & 0x07)
                p[4], p[5], p[6] = (n29 >> 18) & 0xFF, (n29 >> 10) & 0xFF, (n29 >> 2) & 0xFF
                p[7] = (p[7] & 0x3F) | ((n29 & 3) << 6)
            if rng.random() < 0.6:
                ig = int(rng.choice(grids))
                p[7] = (p[7] & 0xE0) | ((ig >> 10) & 0x1F)
                p[8] = (ig >> 2) & 0xFF
                p[9] = (p[9] & 0x3F) | ((ig & 3) << 6)
    mags = np.full((nframes, 92, 2, 2, 256), 60, np.uint8)
    cd = np.dtype([("score", "<i2"), ("time_offset", "<i2"), ("freq_offset", "<i2"), ("time_sub", "u1"), ("freq_sub", "u1")])
    cands = np.zeros((nframes, 120), cd)
    counts = np.full(nframes, per_frame, np.int32)
    sym = np.arange(79)
    for k in range(n):
        f, c = divmod(k, per_frame)
        f0 = 4 + 10 * c
        tones = oracle.encode(np.ascontiguousarray(np.concatenate([payloads[k], np.zeros(2, np.uint8)])))
        mags[f, sym, 0, 0, f0 + np.asarray(tones, np.int64)] = 170
        cands[f, c] = (40, 0, f0, 0, 0)
    mags = mags.reshape(nframes, MAG)
    with ft8.Decoder(device=0, max_frames=nframes) as dec:
        assert cands.dtype.itemsize == dec.find_sync(mags[:1])[0].dtype.itemsize
        st = dec.decode_candidates(mags, cands.view(dec.find_sync(mags[:1])[0].dtype), counts)
    kinds, oks = set(), 0
    for f in range(nframes):
        ref = _oracle_status(oracle, mags[f], cands[f, :per_frame], 20)
        _compare_status(f"sweep frame {f}", st[f], ref)
        for c, r in enumerate(ref):
            assert r["ldpc_errors"] == 0
            oks += int(r["ok"])
            if r["ok"]:
                kinds.add(r["text"].split(" ")[0][:2])
            else:
                assert bytes(st[f][c]["text"]).strip(b"\0") == b"", (f, c)       # no characters of a failed unpack leak into the record
    assert oks > 0.4 * n and len(kinds) >= 12, (oks, sorted(kinds))


def test_end_to_end_spots_exact(oracle, gpu_decoder, frames):
    iq = np.stack([f for _, f in frames])
    dec, n = gpu_decoder.decode_batch(iq)
    total = 0
    for k, (name, f) in enumerate(frames):
        rdec, rn = oracle.subsystem(f[0], f[1])
        assert n[k] == rn, f"{name}: n_results {n[k]} vs {rn}"
        assert dec[k].tobytes() == rdec.tobytes(), f"{name}: spot records differ"
        total += rn
    assert total >= 30


def test_selftest_through_dropin_symbol(oracle):
    """config 1: the reference's own -t check (rtlsdr_ft8d.c:966-971) through ft8_subsystem()"""
    import rtlsdr_ft8d_amd as ft8
    i, q = oracle.selftest_signal()
    lib = ft8.load_library()
    lib.initFFTW()
    dec, n = ft8.ft8_subsystem(i, q)
    assert n == 1
    assert dec[0]["call"] == b"K1JT" and dec[0]["loc"] == b"FN20"
    assert dec[0]["freq"] == 28 and dec[0]["snr"] == 34
    # stale-slot semantics (:1509-1520): a non-CQ frame leaves caller bytes untouched
    pre = np.zeros(50, ft8.RESULT_DTYPE)
    pre["call"] = b"STALE"
    dec2, n2 = ft8.ft8_subsystem(np.zeros(48000, np.float32), np.zeros(48000, np.float32), pre)
    assert n2 == 0 and (dec2["call"] == b"STALE").all()
    lib.freeFFTW()


def test_collect_spots_dedup_and_table_full(oracle, gpu_decoder):
    """>50 unique messages (the reference's non-terminating case), duplicates, non-CQ, 2-token CQ, and caller-made
    records with bytes behind the text's terminator (strcmp never looks at them; the kernel compares canonical dwords)"""
    import rtlsdr_ft8d_amd as ft8
    rng = np.random.default_rng(3)
    C = 120
    cands = np.zeros((3, C), ft8.CAND_DTYPE)
    st = np.zeros((3, C), ft8.STATUS_DTYPE)
    counts = np.array([C, 12, 8], np.int32)
    for c in range(C):
        cands[0, c] = (100 - c // 2, 0, c, 0, c & 1)
        st[0, c]["ok"] = 1
        st[0, c]["crc_extracted"] = (c // 2) * 50 % 16384 if c % 3 else rng.integers(0, 16384)   # clashes on purpose
        st[0, c]["text"] = (f"CQ K{c % 10}AB{chr(65 + (c // 2) % 26)} FN{c // 2 % 100:02d}" if c % 4 else f"W1AW K{c % 10}XYZ -{c % 30:02d}").encode()
    texts = [b"CQ K1ABC FN42", b"CQ K1ABC FN42", b"CQ K1ABC ", b"CQ DX K1JT FN20", b"K1ABC W9XYZ RR73", b"TNX BOB 73 GL",
             b"CQ PJ4/K1ABC", b"", b"CQ", b"CQ1 ABCDEFGHIJKLMNO PQRS", b"CQ K1ABC FN42", b"QRZ K1ABC FN42"]
    for c, t in enumerate(texts):
        cands[1, c] = (50 - c, 1, 20 + c, 0, c & 1)
        st[1, c]["ok"] = 1
        st[1, c]["crc_extracted"] = 77 if c < 3 else 100 + c
        st[1, c]["text"] = t
    cands[1, 10]["score"] = 5          # below min_score -> skipped at :1467
    dirty = [b"CQ K1ABC FN42\0XYZ", b"CQ K1ABC FN42\0QQQQQQQQQQQ", b"CQ K1ABC FN42", b"CQ K1ABC FN4\0" + b"2", b"CQ K1ABC FN4\0Z",
             b"\0CQ K9ZZZ EM10", b"\0\0\0\0junk", b"CQ W1AW FN31\0\0\0\0\0\0\0\0\0\0\0\0x"]
    for c, t in enumerate(dirty):
        cands[2, c] = (40 - c, 0, 30 + c, 0, c & 1)
        st[2, c]["ok"] = 1
        st[2, c]["crc_extracted"] = 4242 if c < 7 else 4243
        raw = np.frombuffer(t.ljust(25, b"\0"), np.uint8)
        st.view(np.uint8).reshape(3, C, 48)[2, c, 22:47] = raw      # the text field, byte for byte (embedded NULs kept)
    dec, n = gpu_decoder.collect_spots(cands, counts, st)
    # reference semantics restated directly in Python for this synthetic table
    for f in range(3):
        table = [None] * 50
        out = np.zeros(50, ft8.RESULT_DTYPE)
        nd = 0
        for c in range(counts[f]):
            if cands[f, c]["score"] < 10 or not st[f, c]["ok"]:
                continue
            h = int(st[f, c]["crc_extracted"])
            text = st.view(np.uint8).reshape(3, C, 48)[f, c, 22:47].tobytes().split(b"\0")[0]
            idx, probes, empty, dup = h % 50, 0, False, False
            while True:
                if table[idx] is None:
                    empty = True
                elif table[idx] == (h, text):
                    dup = True
                else:
                    idx = (idx + 1) % 50
                    probes += 1
                    if probes >= 50:
                        break
                if empty or dup:
                    break
            if empty:
                table[idx] = (h, text)
                toks = text.decode().split()
                if toks and toks[0].startswith("CQ"):
                    out[nd]["call"] = (toks[1] if len(toks) > 1 else "(null)")[:12].encode()
                    out[nd]["loc"] = (toks[2] if len(toks) > 2 else "(null)")[:6].encode()
                    fo, fs = int(cands[f, c]["freq_offset"]), int(cands[f, c]["freq_sub"])
                    out[nd]["freq"] = int((fo + fs / 2) * 6.25)
                    out[nd]["snr"] = int(cands[f, c]["score"])
                nd += 1
        assert n[f] == nd
        assert dec[f].tobytes() == out.tobytes()
    assert n[0] == 50


def test_batch_larger_than_context_and_device_pointers(oracle, frames):
    """chunking over max_frames and the FT8GPU_DEVICE_PTRS path with torch-owned HBM buffers"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    iq = np.stack([f for _, f in frames[:7]])
    with ft8.Decoder(device=0, max_frames=3) as d:
        dec, n = d.decode_batch(iq)
        t_iq = torch.from_numpy(iq).cuda()
        t_dec = torch.zeros(iq.shape[0] * 50 * 28, dtype=torch.uint8, device="cuda")
        t_n = torch.zeros(iq.shape[0], dtype=torch.int32, device="cuda")
        d.set_stream(torch.cuda.current_stream().cuda_stream)
        d.decode_batch_dev(t_iq, iq.shape[0], t_dec, t_n)
        torch.cuda.synchronize()
        assert np.array_equal(t_n.cpu().numpy(), n)
        assert t_dec.cpu().numpy().tobytes() == dec.tobytes()
        d.set_stream(None)
    for k in range(iq.shape[0]):
        rdec, rn = oracle.subsystem(iq[k, 0], iq[k, 1])
        assert n[k] == rn and dec[k].tobytes() == rdec.tobytes()


def test_stage_entries_chunked_host_and_device_forms_agree(oracle, frames):
    """every stage entry over 8 frames, three ways: the host form on a 3-frame context (chunks 3, 3, 2), the device form
    on the same context, and the device form on a context that holds all 8 frames.  Every output starts as the byte
    pattern 0xA5 (the Python wrappers would zero it), so a slot that an entry leaves alone, or fills from the wrong chunk,
    shows.  The three results are byte-identical, with one exception: the host form of decode_candidates returns zeros
    in the status slots past counts[f] (its staging buffer is cleared), where the device form leaves the caller's bytes."""
    import ctypes as C
    import torch
    import rtlsdr_ft8d_amd as ft8
    lib = ft8.load_library()
    B, FILL = 8, 0xA5
    iq = np.stack([f for _, f in frames[:6] + frames[14:16]])       # CQ-heavy synthetic frames and on-air style traffic
    info = ft8.ReportInfo(rcall=b"N0CALL", rloc=b"FN20", app_version=b"rtlsdr-ft8d_v0.3.6", dial_freq=14074000,
                          unixtime=1700000000, sequence=1, random_id=7)

    class Out:
        def __init__(self, shape, dtype):
            self.shape, self.dtype = shape, np.dtype(dtype)

    def call(d, dev, entry, *args):
        """numpy arrays are inputs (uploaded for the device form), Out slots are outputs that start as FILL (and are
        in-out where the entry reads them); anything else is passed as it is"""
        outs, cargs, keep = [], [], []
        for a in args:
            if isinstance(a, Out):
                nbytes = int(np.prod(a.shape)) * a.dtype.itemsize
                if dev:
                    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
                    outs.append((t, a))
                    cargs.append(t.data_ptr())
                else:
                    h = np.full(nbytes, FILL, np.uint8).view(a.dtype).reshape(a.shape)
                    outs.append((h, a))
                    cargs.append(h.ctypes.data)
            elif isinstance(a, np.ndarray):
                h = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
                t = torch.from_numpy(h.copy()).cuda() if dev else h
                keep.append(t)
                cargs.append(t.data_ptr() if dev else t.ctypes.data)
            else:
                cargs.append(a)
        rc = getattr(lib, "ft8gpu_" + entry)(d.h, *cargs, ft8.DEVICE_PTRS if dev else ft8.HOST_PTRS)
        assert rc == 0, lib.ft8gpu_last_error()
        torch.cuda.synchronize()
        return [(o.cpu().numpy() if dev else o).view(a.dtype).reshape(a.shape) for o, a in outs]

    for cap, unixtimes in ((120, None), (7, np.arange(B, dtype=np.uint32) + 1700000000)):
        with ft8.Decoder(device=0, max_frames=3, max_candidates=cap) as d3, ft8.Decoder(device=0, max_frames=B, max_candidates=cap) as d8:
            for d in (d3, d8):
                d.set_stream(torch.cuda.current_stream().cuda_stream)

            def three(entry, *args):
                return call(d3, False, entry, *args), call(d3, True, entry, *args), call(d8, True, entry, *args)

            def same(entry, *args):
                host, dev3, dev8 = three(entry, *args)
                for form, r in (("device form, chunked", dev3), ("device form, one chunk", dev8)):
                    for k, (a, b) in enumerate(zip(host, r)):
                        assert a.tobytes() == b.tobytes(), f"{entry} cap {cap}: output {k} of the {form} differs from the host form"
                return host

            (mag,) = same("waterfall", iq, B, Out((B, MAG), np.uint8))
            cands, counts = same("find_sync", mag, B, Out((B, cap), ft8.CAND_DTYPE), Out((B,), np.int32))
            same("score_map", mag, B, Out((B, 2, 2, 36, 249), np.int16))
            live = np.arange(cap)[None, :] < counts[:, None]
            status = {}
            for dbg in (0, ft8.DBG_PIPELINE_FORM):
                d3.set_debug_flags(dbg)
                d8.set_debug_flags(dbg)
                (host,), (dev3,), (dev8,) = three("decode_candidates", mag, cands, counts, B, Out((B, cap), ft8.STATUS_DTYPE))
                assert dev3.tobytes() == dev8.tobytes(), f"decode_candidates cap {cap} flags {dbg}"
                assert host[live].tobytes() == dev3[live].tobytes(), f"decode_candidates cap {cap} flags {dbg}"
                # the stated exception: past counts[f] the host form returns its cleared staging, the device form the caller's bytes
                assert host[~live].tobytes() == bytes(host[~live].nbytes)
                assert dev3[~live].tobytes() == bytes([FILL]) * dev3[~live].nbytes
                status[dbg] = host
            d3.set_debug_flags(0)
            d8.set_debug_flags(0)
            decodes, nres = same("collect_spots", cands, counts, status[0], B, Out((B, 50), ft8.RESULT_DTYPE), Out((B,), np.int32))
            same("noise_baseline", mag, B, Out((B, 2, 256), np.uint8))
            same("collect_messages", mag, cands, counts, status[0], B, Out((B, 50), ft8.MESSAGE_DTYPE), Out((B,), np.int32))
            same("pskreporter_datagrams", decodes, nres, B, C.byref(info), unixtimes, Out((B, ft8.DATAGRAM_STRIDE), np.uint8),
                 Out((B,), np.int32))

        # ... and agree with the oracle: waterfall, candidate lists, status records (both forms of the kernel), spots
        params = oracle.default_params(max_candidates=cap)
        for k in range(B):
            assert np.array_equal(mag[k], oracle.waterfall(iq[k, 0], iq[k, 1])), f"frame {k}"
            ref = oracle.find_sync(mag[k], cap, 10)
            assert counts[k] == len(ref) and np.array_equal(cands[k, :counts[k]], ref), f"frame {k}"
            _compare_status(f"frame {k}", status[0][k], _oracle_status(oracle, mag[k], cands[k, :counts[k]], 20))
            a, b = status[0][k, :counts[k]], status[ft8.DBG_PIPELINE_FORM][k, :counts[k]]
            for name in ("iters", "crc_extracted", "crc_calculated", "unpack_status", "ok", "a91", "text"):
                assert np.array_equal(a[name], b[name]), f"frame {k}: {name}"
            assert np.array_equal(a["ldpc_errors"] == 0, b["ldpc_errors"] == 0)
            rdec = np.full(50 * ft8.RESULT_DTYPE.itemsize, FILL, np.uint8).view(ft8.RESULT_DTYPE)
            rn = C.c_int32(0)
            oracle.lib().ft8o_subsystem_from_waterfall(oracle._u8(np.ascontiguousarray(mag[k])), C.byref(params),
                                                       rdec.ctypes.data, C.byref(rn))
            assert nres[k] == rn.value and decodes[k].tobytes() == rdec.tobytes(), f"frame {k}: spots"
        if cap == 120:
            assert nres.sum() >= 5 and counts.min() < cap      # real spots, and frames with slots past their count


def test_device_synth_frames_decode_and_match_oracle(oracle):
    """the on-device generator used by bench.py: frames come back to the host and the oracle must
    agree with the GPU decode of the very same samples (full-size batches are checked the same way
    on a sample of frames in bench.py)."""
    import torch
    import rtlsdr_ft8d_amd as ft8
    rng = np.random.default_rng(21)
    B, NS = 6, 8
    sig = np.zeros((B, NS), ft8.SIGNAL_DTYPE)
    sent = []
    for b in range(B):
        for s in range(NS):
            msg = S.random_message(rng)
            sig[b, s]["tones"] = ft8.encode(ft8.pack77_std(msg))
            sig[b, s]["f0_hz"] = rng.uniform(100, 1500)
            sig[b, s]["t0_s"] = rng.uniform(0, 1.8)
            sig[b, s]["amplitude"] = S.amplitude_for_snr(rng.uniform(-12, 0), 1.0)
            sent.append((b, msg))
    with ft8.Decoder(device=0, max_frames=B) as d:
        t_iq = torch.empty((B, 2, 48000), dtype=torch.float32, device="cuda")
        d.synth_frames(sig, B, NS, 1.0, 1234, t_iq)
        iq = t_iq.cpu().numpy()
        assert np.isfinite(iq).all()
        assert np.allclose(np.abs(iq).reshape(B, -1).max(axis=1), 0.5, rtol=1e-6)
        dec, n = d.decode_batch(iq)
    found = 0
    for b in range(B):
        rdec, rn = oracle.subsystem(iq[b, 0], iq[b, 1])
        assert n[b] == rn and dec[b].tobytes() == rdec.tobytes()
        calls = {x["call"].decode() for x in dec[b][:n[b]]}
        found += sum(1 for bb, m in sent if bb == b and m.split()[1] in calls)
    assert found >= 0.6 * len(sent)        # most of the planted CQ calls are recovered


def test_device_synth_waveform_matches_the_cpfsk_oracle(oracle):
    """f-3: the on-device generator's signal part against the double-precision restatement of the
    reference's modulation loop (rtlsdr_ft8d.c:946-955).  Noise off, so the frame is the sum of the CPFSK
    signals, peak-normalised to 0.5 (:248-263).  Tolerance 1e-5 absolute on samples of magnitude <= 0.5:
    the kernel evaluates sincospi of a double cycle count in float."""
    import torch
    import rtlsdr_ft8d_amd as ft8
    rng = np.random.default_rng(33)
    cases = [1, 1, 4, 20]
    B, NS = len(cases), max(cases)
    sig = np.zeros((B, NS), ft8.SIGNAL_DTYPE)
    for b, ns in enumerate(cases):
        for s in range(ns):
            sig[b, s]["tones"] = ft8.encode(ft8.pack77_std(S.random_message(rng)))
            sig[b, s]["f0_hz"] = rng.uniform(100, 1500)
            sig[b, s]["t0_s"] = rng.uniform(0, 2.4) if b else 0.0      # late starts run off the end of the frame
            sig[b, s]["amplitude"] = rng.uniform(0.1, 2.0)
    with ft8.Decoder(device=0, max_frames=B) as d:
        t_iq = torch.empty((B, 2, 48000), dtype=torch.float32, device="cuda")
        d.synth_frames(sig, B, NS, 0.0, 99, t_iq)
        iq = t_iq.cpu().numpy()
    for b, ns in enumerate(cases):
        start = [int(np.rint(np.float32(sig[b, s]["t0_s"]) * np.float32(3200.0))) for s in range(NS)]
        oi, oq = oracle.synth_cpfsk(sig[b]["tones"], sig[b]["f0_hz"].astype(np.float64), start,
                                    sig[b]["amplitude"].astype(np.float64))
        oi, oq = oracle.normalise(oi, oq)
        assert np.abs(iq[b, 0] - oi).max() <= 1e-5 and np.abs(iq[b, 1] - oq).max() <= 1e-5, b
        assert abs(np.abs(iq[b]).max() - 0.5) < 1e-6


def test_device_synth_noise_statistics():
    """f-3: the counter-based AWGN of the generator (no CPU counterpart): mean, variance ratio, whiteness,
    I/Q independence, Gaussian tails and frame-to-frame independence on about 10^6 samples"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    B = 11
    sig = np.zeros((B, 0), ft8.SIGNAL_DTYPE)                          # no signals: noise only
    with ft8.Decoder(device=0, max_frames=B) as d:
        t_iq = torch.empty((B, 2, 48000), dtype=torch.float32, device="cuda")
        d.synth_frames(sig, B, 0, 1.0, 4242, t_iq)
        iq = t_iq.cpu().numpy().astype(np.float64)
    x = iq / iq.reshape(B, -1).std(axis=1)[:, None, None]            # undo the per-frame peak normalisation
    flat = x.reshape(-1)                                             # 1 056 000 samples
    n = flat.size
    assert abs(flat.mean()) < 4 / np.sqrt(n)
    assert abs((flat ** 4).mean() - 3.0) < 0.03                      # Gaussian kurtosis
    assert abs((np.abs(flat) > 3).mean() - 0.0026998) < 3e-4         # 3-sigma tail mass
    for b in range(B):
        i_, q_ = x[b, 0], x[b, 1]
        assert abs(np.mean(i_[:-1] * i_[1:])) < 5 / np.sqrt(48000)   # lag-1 autocorrelation
        assert abs(np.mean(i_ * q_)) < 5 / np.sqrt(48000)            # I/Q cross-correlation
        assert 3.6 < 0.5 / iq[b].std() < 5.6                         # peak of 96 000 Gaussian samples is 4-5 sigma
    assert abs(np.mean(x[0, 0] * x[1, 0])) < 5 / np.sqrt(48000)      # different frames are independent
    assert abs(x[:, 0].var() / x[:, 1].var() - 1.0) < 0.01


def test_decode_with_forced_ieee_division(oracle):
    """the BP kernel's guarded fast division falls back to the compiler's IEEE division when a
    numerator is tiny; FT8GPU_DBG_FORCE_IEEE_DIV (a per-context flag) takes that path for every
    division.  Compared against the oracle again, stage boundary and whole path."""
    import rtlsdr_ft8d_amd as ft8
    enc = S.oracle_encode_fn(oracle)
    frames = [np.stack(oracle.selftest_signal())] + [S.make_frame(s, n, enc, snr_range=(-18, 0), cq_fraction=0.7)[0]
                                                     for s, n in [(13, 20), (14, 40), (16, 12)]]
    iq = np.stack(frames)
    with ft8.Decoder(device=0, max_frames=4) as d:
        d.set_debug_flags(ft8.DBG_FORCE_IEEE_DIV)
        mag = d.waterfall(iq)
        cands, counts = d.find_sync(mag)
        st = d.decode_candidates(mag, cands, counts)
        dec, n = d.decode_batch(iq)
        d.set_debug_flags(0)
        st_fast = d.decode_candidates(mag, cands, counts)
    assert st.tobytes() == st_fast.tobytes()               # both division forms give the same records
    assert int(counts.sum()) > 100
    for k in range(iq.shape[0]):
        for c in range(counts[k]):
            r = oracle.decode(mag[k], cands[k, c:c + 1], 20)
            g = st[k, c]
            assert g["ldpc_errors"] == r["ldpc_errors"] and g["iters"] == r["iters"]
            assert bytes(g["a91"]) == r["a91"] and bool(g["ok"]) == r["ok"]
        rdec, rn = oracle.subsystem(iq[k, 0], iq[k, 1])
        assert n[k] == rn and dec[k].tobytes() == rdec.tobytes()


def test_bp_division_chains_by_exhaustion():
    """fast_tanh / fast_atanh (ft8_lib ldpc.c) are functions of ONE float, so the BP kernel's short rcp/fma division
    chains (csrc/bp_math.h: three operations after v_rcp_f32 for atanh, five for tanh) are checked against the
    compiler's IEEE-754 division on EVERY input of the fast path's domain -- all 2^32 bit patterns, scalar and
    packed forms.  Zero mismatches is the proof the parity claim of the LDPC kernel rests on.  Also bounds
    max|fast_tanh|, which bounds fast_atanh's inputs (six factors per check row at most)."""
    import rtlsdr_ft8d_amd as ft8
    with ft8.Decoder(device=0, max_frames=1) as d:
        r = d.selftest_bp_math()
    assert r["tanh_inputs"] > 2_000_000_000 and r["atanh_inputs"] > 900_000_000, r
    assert r["tanh_mismatch"] == 0 and r["atanh_mismatch"] == 0 and r["pair_mismatch"] == 0, r
    assert r["first_bad"] == 0
    assert 1.0 < r["tanh_max"] < 1.0075 and r["tanh_max"] ** 6 < 1.05, r          # 1.05 = bpm::kAtanhMaxAbs
    with ft8.Decoder(device=0, max_frames=1) as d:
        with pytest.raises(ft8.Ft8GpuError, match="unknown bits"):
            d.set_debug_flags(64)
        with pytest.raises(ft8.Ft8GpuError, match="unknown bits"):
            d.set_debug_flags(16)            # kernel-form selectors exist in the A/B build only


def test_llr_scale_factor_is_correctly_rounded_on_every_float():
    """ftx_normalize_logl scales the soft bits by sqrtf(24.0f / variance): two correctly rounded operations in the reference.
    Rounds 1-4 computed the root with HIP's __fsqrt_rn, which (without OCML_BASIC_ROUNDED_OPERATIONS) is the raw 1-ulp
    v_sqrt_f32: about one candidate in a hundred got LLRs one ulp low, visible only where a hard decision sat within an ulp
    of zero -- 93 candidates in 20 million, found by comparing every candidate's status record (tools/soak_parity.py
    --records).  ft8gpu_selftest_norm_math holds the quotient and the root the kernel computes against EXACT arithmetic
    (products and squares that are exact in double) for every float in [2^-60, 2^60]."""
    import rtlsdr_ft8d_amd as ft8
    with ft8.Decoder(device=0, max_frames=1) as d:
        r = d.selftest_norm_math()
    assert r["inputs"] == 120 * (1 << 23) + 1, r                 # every float of 120 binades and 2^60 itself
    assert r["div_bad"] == 0 and r["sqrt_bad"] == 0 and r["compose_bad"] == 0 and r["first_bad"] == 0, r
    # ... and the divisions inside fast_tanh / fast_atanh, which the chains of ft8gpu_selftest_bp_math are compared with, are
    # themselves the correctly rounded quotients on every input of their domains
    assert r["rational_inputs"] > 1_100_000_000 and r["rational_div_bad"] == 0, r


def test_decode_pipeline_form_of_the_kernel(oracle):
    """the batch pipeline runs the BP kernel without the exact error count: a scalar group-parity test
    screens every hard decision and only survivors get the exact per-row check.  With
    FT8GPU_DBG_PIPELINE_FORM the stage entry runs that form; every field except ldpc_errors must be
    what the oracle (and the counting form) reports, and ldpc_errors must be 0 exactly for codewords."""
    import rtlsdr_ft8d_amd as ft8
    enc = S.oracle_encode_fn(oracle)
    frames = [np.stack(oracle.selftest_signal()), np.zeros((2, 48000), np.float32)]
    frames += [S.make_frame(s, n, enc, snr_range=(-20, 0), cq_fraction=0.7)[0] for s, n in [(21, 20), (22, 40), (23, 12), (24, 60), (25, 0)]]
    iq = np.stack(frames)
    ncand = nok = 0
    for iters in (20, 3):
        with ft8.Decoder(device=0, max_frames=iq.shape[0], ldpc_iters=iters) as d:
            d.set_debug_flags(ft8.DBG_PIPELINE_FORM)
            mag = d.waterfall(iq)
            cands, counts = d.find_sync(mag)
            st = d.decode_candidates(mag, cands, counts)
        for k in range(iq.shape[0]):
            for c in range(counts[k]):
                r = oracle.decode(mag[k], cands[k, c:c + 1], iters)
                g = st[k, c]
                ncand += 1
                nok += bool(g["ok"])
                assert (g["ldpc_errors"] == 0) == (r["ldpc_errors"] == 0) and g["ldpc_errors"] in (0, 83)
                assert g["iters"] == r["iters"] and bytes(g["a91"]) == r["a91"] and bool(g["ok"]) == r["ok"]
                if r["ok"]:
                    assert g["text"].decode() == r["text"] and g["crc_extracted"] == r["crc_extracted"]
    assert ncand > 200 and nok > 20


def test_c_caller_self_test_and_file_replay(oracle, tmp_path):
    """examples/ft8_replay.c: a plain C program that links libft8gpu.so and uses only the reference's
    own three symbols (initFFTW / ft8_subsystem / freeFFTW) the way rtlsdr_ft8d.c does for -t and -r"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "ft8_replay")
    subprocess.check_call(["gcc", "-O2", "-std=gnu17", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "ft8_replay.c"),
                           "-L", os.path.join(root, "rtlsdr_ft8d_amd"), "-lft8gpu",
                           "-Wl,-rpath," + os.path.join(root, "rtlsdr_ft8d_amd"), "-lm", "-o", exe])
    out = subprocess.run([exe, "-t"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Self-test SUCCESS!" in out.stdout and "K1JT" in out.stdout and "FN20" in out.stdout
    # the self-test wrote selftest.iq (Q negated, :784-806); replaying it decodes again (-r path, :859-887)
    out = subprocess.run([exe, "selftest.iq"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "Number of samples: 48000" in out.stdout and "K1JT" in out.stdout
    # same file through the oracle's reader + decoder gives the same single spot
    import ctypes as C
    i2, q2 = np.zeros(48000, np.float32), np.zeros(48000, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert oracle.lib().ft8o_read_raw_iq(fp(i2), fp(q2), str(tmp_path / "selftest.iq").encode()) == 48000
    dec, n = oracle.subsystem(i2, q2)
    assert n == 1 and f"     {int(dec[0]['snr']):2d} {int(dec[0]['freq']):8d} {dec[0]['call'].decode():>10s} {dec[0]['loc'].decode():>6s}" in out.stdout


def test_ft8_lib_level_c_caller(tmp_path):
    """examples/ft8_lib_level.c: the reference's own candidate loop (rtlsdr_ft8d.c:1438-1523) written against
    the ft8_lib-level headers under include/ft8_lib/ft8/ and the symbols ft8_find_sync / ft8_decode / pack77 /
    ft8_encode of libft8gpu.so -- must give the records ft8_subsystem gives"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "ft8_lib_level")
    subprocess.check_call(["gcc", "-O2", "-std=gnu17", "-Wall", "-Wextra", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "ft8_lib_level.c"),
                           "-L", os.path.join(root, "rtlsdr_ft8d_amd"), "-lft8gpu",
                           "-Wl,-rpath," + os.path.join(root, "rtlsdr_ft8d_amd"), "-lm", "-o", exe])
    out = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ft8_lib-level path == ft8_subsystem" in out.stdout and "K1JT" in out.stdout and "DL1ABC" in out.stdout
    # the frame carries QSO traffic too: 13 unique messages, five of them CQ-first (two without a locator), one heard twice
    assert "ft8_lib level: 13 messages, ft8_subsystem: 13 messages" in out.stdout and "PJ4/K1ABC" in out.stdout and "(null)" in out.stdout


def test_ft8_lib_level_symbols_match_the_oracle(oracle, frames, oracle_mags):
    """ft8_find_sync / ft8_decode (rtlsdr_ft8d.c:1450, :1476) through ctypes: candidate lists and every
    candidate's message / status against the oracle, including the paths that bypass the remembered list
    (a candidate that was not returned by ft8_find_sync, a waterfall changed in place, another iteration count)"""
    import ctypes as C
    import rtlsdr_ft8d_amd as ft8

    class Waterfall(C.Structure):
        _fields_ = [("max_blocks", C.c_int), ("num_blocks", C.c_int), ("num_bins", C.c_int), ("time_osr", C.c_int),
                    ("freq_osr", C.c_int), ("mag", C.c_void_p), ("block_stride", C.c_int), ("protocol", C.c_int)]

    class Message(C.Structure):
        _fields_ = [("text", C.c_char * 25), ("hash", C.c_uint16)]

    class Status(C.Structure):
        _fields_ = [("ldpc_errors", C.c_int), ("crc_extracted", C.c_uint16), ("crc_calculated", C.c_uint16), ("unpack_status", C.c_int)]

    L = ft8.load_library()
    L.ft8_find_sync.argtypes = [C.POINTER(Waterfall), C.c_int, C.c_void_p, C.c_int]
    L.ft8_decode.argtypes = [C.POINTER(Waterfall), C.c_void_p, C.POINTER(Message), C.c_int, C.POINTER(Status)]
    L.ft8_decode.restype = C.c_bool

    def check(mag, cand, iters):
        m, st = Message(), Status()
        ok = L.ft8_decode(C.byref(wf), cand.ctypes.data, C.byref(m), iters, C.byref(st))
        r = oracle.decode(mag, cand, iters)
        assert bool(ok) == r["ok"] and st.ldpc_errors == r["ldpc_errors"]
        if r["ldpc_errors"] == 0:
            assert (st.crc_extracted, st.crc_calculated) == (r["crc_extracted"], r["crc_calculated"])
        if r["ok"]:
            assert m.text.decode() == r["text"] and m.hash == r["hash"] and st.unpack_status == r["unpack_status"]
        return bool(ok)

    nok = 0
    for k in (0, 3, 4, 5):                                   # self-test, 20 / 40 / 60 signals
        mag = oracle_mags[k].copy()
        wf = Waterfall(0, 92, 256, 2, 2, mag.ctypes.data, 1024, 1)      # PROTO_FT8 = 1
        heap = np.zeros(120, ft8.CAND_DTYPE)
        n = L.ft8_find_sync(C.byref(wf), 120, heap.ctypes.data, 10)
        ref = oracle.find_sync(mag)
        assert n == len(ref) and np.array_equal(heap[:n], ref)
        for c in range(n):                                   # the remembered list: one launch, then lookups
            nok += check(mag, heap[c:c + 1], 20)
        for c in (0, n // 2):                                # another iteration count re-decodes the list
            check(mag, heap[c:c + 1], 3)
        other = heap[:1].copy()                              # a candidate ft8_find_sync never returned
        other["freq_offset"] += 1
        check(mag, other, 20)
        for c in range(n):                                   # back to 20: the list is decoded again and fully cached ...
            check(mag, heap[c:c + 1], 20)
        mag[1000:60000] = np.random.default_rng(k).integers(0, 255, 59000, dtype=np.uint8)   # ... same buffer, new bytes:
        for c in (0, 1, n - 1):                              # a cached answer would be stale now, also at the cached iteration count
            check(mag, heap[c:c + 1], 20)
            check(mag, heap[c:c + 1], 7)
    assert nok > 30
    # geometry the kernels are not built for is refused
    bad = Waterfall(0, 93, 256, 2, 2, oracle_mags[0].ctypes.data, 1024, 1)
    assert L.ft8_find_sync(C.byref(bad), 120, np.zeros(120, ft8.CAND_DTYPE).ctypes.data, 10) == 0
    # and the drop-in ft8_subsystem still uses the reference's constants afterwards
    i, q = frames[3][1]
    dec, n = ft8.ft8_subsystem(i, q)
    rdec, rn = oracle.subsystem(i, q)
    assert n == rn and dec.tobytes() == rdec.tobytes()


@pytest.mark.parametrize("cap,min_score,iters", [(33, 10, 20), (7, 12, 5), (250, 8, 20)])
def test_end_to_end_other_parameters(oracle, gpu_decoder, frames, cap, min_score, iters):
    """run-time forms of K_MAX_CANDIDATES / K_MIN_SCORE / K_LDPC_ITERS (rtlsdr_ft8d.h:43-45), including
    caps that are not a multiple of the 4 candidate waves of a decode workgroup"""
    gpu_decoder.set_params(min_score=min_score, max_candidates=cap, ldpc_iters=iters)
    try:
        iq = np.stack([f for _, f in frames[:7]])
        dec, n = gpu_decoder.decode_batch(iq)
        p = oracle.default_params(min_score, cap, iters)
        for k in range(iq.shape[0]):
            rdec, rn = oracle.subsystem(iq[k, 0], iq[k, 1], p)
            assert n[k] == rn and dec[k].tobytes() == rdec.tobytes(), frames[k][0]
    finally:
        gpu_decoder.set_params(min_score=10, max_candidates=120, ldpc_iters=20)


def test_api_edge_cases_and_errors(gpu_decoder):
    """empty batches, parameter validation and NULL arguments report through the int return code /
    ft8gpu_last_error (the reference's void ft8_subsystem has no error channel)"""
    import ctypes as C
    import rtlsdr_ft8d_amd as ft8
    lib = ft8.load_library()
    h = gpu_decoder.h
    # empty batch: nothing to do, success, outputs untouched
    dec = np.full((1, 50), 7, np.uint8).view(np.uint8)
    n = np.array([-5], np.int32)
    assert lib.ft8gpu_decode_batch(h, 0, 0, 0, 0, ft8.HOST_PTRS) == 0
    iq = np.zeros((0, 2, 48000), np.float32)
    d, nn = gpu_decoder.decode_batch(iq)
    assert d.shape == (0, 50) and nn.shape == (0,)
    # NULL arrays / negative counts
    assert lib.ft8gpu_decode_batch(h, 0, 1, 0, 0, ft8.HOST_PTRS) != 0 and b"NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_decode_batch(h, 0, -1, 0, 0, ft8.HOST_PTRS) != 0
    assert lib.ft8gpu_waterfall(h, 0, 1, 0, ft8.HOST_PTRS) != 0
    # parameter validation (rtlsdr_ft8d.h:43-45 made run-time)
    for bad in [dict(max_candidates=0), dict(max_candidates=ft8.load_library() and 1025), dict(ldpc_iters=0), dict(min_score=40000)]:
        with pytest.raises(ft8.Ft8GpuError):
            gpu_decoder.set_params(**bad)
    assert (gpu_decoder.params.min_score, gpu_decoder.params.max_candidates, gpu_decoder.params.ldpc_iters) == (10, 120, 20)
    # a context on a GPU that does not exist
    with pytest.raises(ft8.Ft8GpuError):
        ft8.Decoder(device=99, max_frames=1)
    with pytest.raises(ft8.Ft8GpuError):
        ft8.Decoder(device=0, max_frames=0)
    # RX front end argument checks
    assert lib.ft8gpu_rx_decimate(h, 0, 1, 800, 0, 0, ft8.HOST_PTRS) != 0
    raw = np.zeros(2 * 804, np.uint8)
    out = np.zeros((1, 2, 48000), np.float32)
    assert lib.ft8gpu_rx_decimate(h, raw.ctypes.data, 1, 804, out.ctypes.data, 0, ft8.HOST_PTRS) != 0      # 804 % 8 != 0
    assert b"multiple of 8" in lib.ft8gpu_last_error()
    # timing is off unless enabled
    with pytest.raises(ft8.Ft8GpuError):
        gpu_decoder.timings()


def test_decode_randomised_waterfall_sweep(oracle, gpu_decoder):
    """3 840 candidates over waterfalls built to stress the float paths of the BP kernel: saturated random
    bytes, two-level maps (huge normalisation factors), nearly constant maps with sparse spikes (many zero
    LLRs = erasures, exact zeros inside BP), smooth gradients, and real-looking noise with planted tones.
    Every candidate's ldpc_errors / iterations / packed bits / CRC / text must equal the oracle's."""
    rng = np.random.default_rng(2024)
    mags = []
    for k in range(32):
        kind = k % 8
        if kind == 0:
            m = rng.integers(0, 256, MAG, dtype=np.uint8)
        elif kind == 1:
            m = (100 + rng.integers(0, 2, MAG)).astype(np.uint8)                      # two adjacent levels
        elif kind == 2:
            m = np.full(MAG, 90, np.uint8)
            idx = rng.integers(0, MAG, 3000)
            m[idx] = rng.integers(91, 140, idx.size)                                  # sparse spikes on a flat floor
        elif kind == 3:
            m = (np.arange(MAG) % 251).astype(np.uint8)                               # sawtooth
        elif kind == 4:
            m = np.clip(rng.normal(120, 6, MAG), 0, 255).astype(np.uint8)             # noise floor
        elif kind == 5:
            m = np.clip(rng.normal(120, 6, MAG), 0, 255).astype(np.uint8).reshape(92, 2, 2, 256)
            for _ in range(30):                                                       # planted tone ladders
                f, t0 = rng.integers(0, 248), rng.integers(0, 12)
                for s in range(79):
                    m[min(t0 + s, 91), :, :, f + rng.integers(0, 8)] += 40
            m = m.reshape(MAG)
        elif kind == 6:
            m = (rng.integers(0, 4, MAG) * 85).astype(np.uint8)                       # four levels, full range
        else:
            m = np.clip(rng.normal(20, 30, MAG), 0, 255).astype(np.uint8)             # clipped at zero
        mags.append(m)
    mags = np.stack(mags)
    cd = gpu_decoder.find_sync(mags[:1])[0].dtype
    cands = np.zeros((32, 120), cd)
    counts = np.full(32, 120, np.int32)
    for k in range(32):
        for c in range(120):
            cands[k, c] = (rng.integers(10, 60), rng.integers(-12, 24), rng.integers(0, 249), rng.integers(0, 2), rng.integers(0, 2))
    total = conv = 0
    for a in range(0, 32, 16):
        st = gpu_decoder.decode_candidates(mags[a:a + 16], cands[a:a + 16], counts[a:a + 16])
        for k in range(16):
            ref = _oracle_status(oracle, mags[a + k], cands[a + k], 20)
            _compare_status(f"sweep{a + k}", st[k], ref)
            total += len(ref)
            conv += sum(r["ldpc_errors"] == 0 for r in ref)
    assert total == 3840


@pytest.mark.parametrize("form", ["rows", "ab-rows", "ab-lds"])
def test_waterfall_forms_are_bit_identical(oracle, form):
    """Both forms of the last FFT stage -- 4 x 4 register transposes across the wave's rows with v_permlane16/32_swap
    (the product) and the exchange through LDS -- must produce the oracle's bytes.  The LDS form is not in the shipped
    library any more: it is compiled into the A/B build (libft8gpu_ab.so, -DFT8GPU_AB_FORMS) and selected there by a
    per-context flag; the same test runs the product library, the A/B build's product form and its LDS form."""
    import rtlsdr_ft8d_amd as ft8
    import synth_util as S
    enc = S.oracle_encode_fn(oracle)
    fr = [np.stack(oracle.selftest_signal())] + [S.make_frame(s, n, enc)[0] for s, n in ((3, 5), (4, 30), (5, 0))]
    fr.append(np.zeros((2, 48000), np.float32))
    rng = np.random.default_rng(2)
    big = rng.normal(0, 0.2, (300, 2, 48000)).astype(np.float32)      # enough frames for the XCD-aware work order
    iq = np.concatenate([np.stack(fr), big])
    lib = None if form == "rows" else ft8.load_ab_library()
    with ft8.Decoder(device=0, max_frames=iq.shape[0], lib=lib) as d:
        if form == "ab-lds":
            d.set_debug_flags(ft8.AB_WATERFALL_LDS)
        if form == "rows":
            with pytest.raises(ft8.Ft8GpuError, match="unknown bits"):      # the shipped library has no such form
                d.set_debug_flags(ft8.AB_WATERFALL_LDS)
        mag = d.waterfall(iq)
        dec, n = d.decode_batch(iq[:5])
    for k in list(range(5)) + [5, 100, 304]:
        assert np.array_equal(mag[k], oracle.waterfall(iq[k, 0], iq[k, 1])), (form, k)
    for k in range(5):
        rdec, rn = oracle.subsystem(iq[k, 0], iq[k, 1])
        assert n[k] == rn and dec[k].tobytes() == rdec.tobytes(), (form, k)


def test_gpu_against_the_independent_numpy_restatement(gpu_decoder, frames, oracle_mags):
    """closes the triangle: the HIP kernels against tests/ft8_spec_decode.py (numpy float32 written from SURVEY Appendix A,
    not from the oracle) directly -- all 35 856 sync scores, the ordered candidate list, and per candidate the
    parity-error count, the BP iterations entered and the 91 packed bits"""
    import ft8_spec_decode as spec
    bp = spec.BP()
    checked = 0
    for k in (0, 3):                                          # the reference's self-test frame and a 20-signal frame
        mag = oracle_mags[k]
        sc = spec.score_map(mag)
        assert np.array_equal(gpu_decoder.score_map(mag[None])[0].reshape(sc.shape), sc.astype(np.int16))
        cands, counts = gpu_decoder.find_sync(mag[None])
        mine = spec.find_sync(mag, 120, 10, scores=sc)
        assert int(counts[0]) == len(mine)
        got = [[int(c["score"]), int(c["time_offset"]), int(c["freq_offset"]), int(c["time_sub"]), int(c["freq_sub"])] for c in cands[0, :counts[0]]]
        assert got == [list(c) for c in mine]
        st = gpu_decoder.decode_candidates(mag[None], cands, counts)[0]
        for c in range(min(len(mine), 40)):
            errors, entered, a91 = spec.decode_candidate(bp, mag, mine[c], 20)
            assert (int(st[c]["ldpc_errors"]), int(st[c]["iters"]), bytes(st[c]["a91"])) == (errors, entered, a91), (k, c)
            checked += 1
    assert checked > 40


@pytest.mark.parametrize("form", ["lane", "wave"])
def test_heap_forms_are_exact(oracle, form):
    """ft8_heap_simt_kernel (one lane per frame; the batch pipeline uses it from 3072 frames on) and the wave-per-frame
    kernel must both return the reference's candidate lists -- order included: each is forced for every launch with its
    per-context flag of the A/B build (the shipped library picks the form by launch size and has no such flags) and
    compared with the oracle at several caps, thresholds and ragged frame counts"""
    import rtlsdr_ft8d_amd as ft8
    import synth_util as S
    enc = S.oracle_encode_fn(oracle)
    fr = [np.stack(oracle.selftest_signal())] + [S.make_frame(s, n, enc, snr_range=(-20, 0))[0] for s, n in ((3, 5), (4, 30), (5, 60), (6, 0), (7, 45))]
    fr.append(np.zeros((2, 48000), np.float32))
    rng = np.random.default_rng(9)
    mags = [oracle.waterfall(f[0], f[1]) for f in fr] + [rng.integers(0, 256, 94208, dtype=np.uint8) for _ in range(70)]   # 77 frames: two waves, ragged
    mag = np.stack(mags)
    bad = []
    with ft8.Decoder(device=0, max_frames=len(mags), lib=ft8.load_ab_library()) as d:
        d.set_debug_flags(ft8.AB_HEAP_LANE_PER_FRAME if form == "lane" else ft8.AB_HEAP_WAVE_PER_FRAME)
        for cap, ms in ((120, 10), (128, 10), (7, 10), (1, 10), (33, 0), (120, -5), (64, 30)):
            d.set_params(min_score=ms, max_candidates=cap)
            cands, counts = d.find_sync(mag)
            for k in range(len(mags)):
                ref = oracle.find_sync(mags[k], cap, ms)
                if counts[k] != len(ref) or not np.array_equal(cands[k, :counts[k]], ref) or cands[k, counts[k]:].tobytes().strip(b"\0"):
                    bad.append((cap, ms, k))
        with pytest.raises(ft8.Ft8GpuError, match="exclude each other"):
            d.set_debug_flags(ft8.AB_HEAP_LANE_PER_FRAME | ft8.AB_HEAP_WAVE_PER_FRAME)
    assert not bad, bad[:5]


def test_candidates_that_showed_the_one_ulp_square_root(oracle, gpu_decoder):
    """tests/golden/sqrt_ulp_cases.*: four candidates (waterfall + candidate) out of the 93 in 20 million whose status record
    differed from the oracle while the LLR scale factor was computed with HIP's __fsqrt_rn (the native 1-ulp root; the
    fixture keeps what the GPU said then).  A hard decision sits within an ulp of zero at one BP iteration of each: with the
    correctly rounded root the GPU must agree with the oracle at every max_iterations 1 ... 20 -- and it must NOT reproduce the
    recorded outputs of the old library (the fixture really discriminates)."""
    import json
    d = np.load(os.path.join(ROOT, "tests", "golden", "sqrt_ulp_cases.npz"))
    old = json.load(open(os.path.join(ROOT, "tests", "golden", "sqrt_ulp_cases.json")))["cases"]
    cd = gpu_decoder.find_sync(d["mag"][:1])[0].dtype
    n = d["mag"].shape[0]
    cands = np.zeros((n, 120), cd)
    for k in range(n):
        cands[k, 0] = tuple(int(x) for x in d["cand"][k])
        assert [int(x) for x in d["cand"][k]] == old[k]["candidate"]
    counts = np.ones(n, np.int32)
    reproduced_old = 0
    try:
        for it in range(1, 21):
            gpu_decoder.set_params(ldpc_iters=it)
            st = gpu_decoder.decode_candidates(d["mag"], cands, counts)
            for k in range(n):
                ref = oracle.decode(d["mag"][k], cands[k, :1].view(oracle.CAND_DTYPE), it)
                _compare_status(f"case {k} max_iterations {it}", st[k], [ref])
                g_old = old[k]["by_max_iterations"][it - 1]
                reproduced_old += int((int(st[k, 0]["ldpc_errors"]), bytes(st[k, 0]["a91"]).hex()) == (g_old[0], g_old[1]) and (g_old[0], g_old[1]) != (g_old[2], g_old[3]))
    finally:
        gpu_decoder.set_params(ldpc_iters=20)
    assert reproduced_old == 0
