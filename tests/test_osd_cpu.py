"""CPU tests of ordered-statistics decoding: the tables behind it, the numpy restatement of the rule
(tests/ft8_spec_osd.py) against a second, differently written search, its behaviour on planted codewords and on noise, and
the frozen fixture the device is held to as well (tests/golden/osd_frame.npz)."""
import os

import numpy as np

import ft8_spec_osd as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAY_INV = {g: b for b, g in enumerate([0, 1, 3, 2, 5, 6, 4, 7])}


def _codeword_of_tones(tones):
    bits = []
    for k in list(range(7, 36)) + list(range(43, 72)):
        v = GRAY_INV[int(tones[k])]
        bits += [(v >> 2) & 1, (v >> 1) & 1, v & 1]
    return np.array(bits, np.uint8)


def _cq_frames(oracle, seeds, nsig, snr=(-22.0, 0.0)):
    import synth_util as S
    enc = S.oracle_encode_fn(oracle)
    return np.stack([S.make_frame(s, nsig, enc, snr_range=snr)[0] for s in seeds])


def test_generator_times_parity_check_is_zero():
    G, H = so.generator_matrix(), so.parity_check_matrix()
    assert G.shape == (91, 174) and H.shape == (83, 174)
    assert np.array_equal(G[:, :91], np.eye(91, dtype=np.uint8))
    assert not ((G.astype(np.int32) @ H.T.astype(np.int32)) & 1).any()
    assert sorted(set(H.sum(axis=1))) == [6, 7] and set(H.sum(axis=0)) == {3}


def test_generator_rows_are_the_encoders_codewords(oracle):
    """Row k of G is the codeword of the unit message k.  Two encoders: a byte-wise restatement of ft8_lib's encode174 on all
    91 unit messages, and the project's ft8_encode (payload -> CRC -> codeword -> tones) on the 77 unit payloads and on random
    ones, whose codeword must be a91 x G -- the CRC bits bring rows 77..90 in."""
    import rtlsdr_ft8d_amd as ft8
    G = so.generator_matrix()
    gen = np.array(so._table("kFT8_generator"), np.uint8).reshape(83, 12)
    for k in range(91):
        msg = np.zeros(12, np.uint8)
        msg[k >> 3] = 0x80 >> (k & 7)
        cw = np.zeros(22, np.uint8)
        cw[:12] = msg
        for i in range(83):
            par = 0
            for j in range(12):
                par ^= bin(int(msg[j] & gen[i, j])).count("1") & 1
            if par:
                cw[(91 + i) >> 3] |= 0x80 >> ((91 + i) & 7)
        assert np.array_equal(np.unpackbits(cw)[:174], G[k]), k
    rng = np.random.default_rng(3)
    payloads = [np.packbits(np.eye(80, dtype=np.uint8)[k]) for k in range(77)]
    payloads += [rng.integers(0, 256, 10).astype(np.uint8) & np.array([255] * 9 + [0xF8], np.uint8) for _ in range(200)]
    for p in payloads:
        for enc in (ft8.encode, oracle.encode):
            cw = _codeword_of_tones(enc(p))
            assert np.array_equal(cw, (cw[:91].astype(np.int32) @ G.astype(np.int32)) & 1)
            assert np.array_equal(cw[:77], np.unpackbits(p)[:77])


def test_crc14_equals_the_decoders(oracle):
    rng = np.random.default_rng(4)
    for _ in range(300):
        bits = rng.integers(0, 2, 77).astype(np.uint8)
        a = np.packbits(np.concatenate([bits, np.zeros(19, np.uint8)]))
        assert oracle.crc14(a.tobytes(), 82) == so.crc14(bits)
    assert so.crc14(np.zeros(77, np.uint8)) == 0


def test_planted_codeword_is_recovered_at_the_order_that_covers_the_flips():
    """a codeword, soft bits of random reliability, sign flips at 0 / 1 / 2 of the least reliable basis positions and at
    four positions outside the basis: the search finds it at the order that covers the flips inside the basis, and at no
    lower order (no pattern of a lower order agrees with it on the basis)"""
    G = so.generator_matrix()
    rng = np.random.default_rng(11)
    for trial in range(12):
        msg = rng.integers(0, 2, 91)
        cw = ((msg @ G.astype(np.int64)) & 1).astype(np.uint8)
        llr = ((2.0 * cw - 1.0) * rng.uniform(1.0, 6.0, 174)).astype(np.float32)
        basis, _ = so.reduced_basis(so.sort_order(llr))
        outside = np.setdiff1d(np.arange(174), basis)
        for nflip in (0, 1, 2):
            x = llr.copy()
            x[basis[[90, 88][:nflip]]] *= -1                    # magnitudes stay: the same order, the same basis
            x[rng.choice(outside, 4, replace=False)] *= -1
            res = so.search(x)
            for order in range(3):
                metric, pat, nhard, c = res[order]
                if order >= nflip:
                    assert np.array_equal(c, cw) and nhard == nflip + 4, (trial, nflip, order)
                    assert pat == [0, 1 + 90, 92 + (88 * 90 - 88 * 87 // 2) + 1][nflip], (trial, nflip, pat)
                else:
                    assert not np.array_equal(c, cw), (trial, nflip, order)


def _independent_search(llr):
    """the rule written another way: the basis from an XOR-basis of the generator's columns as integers, the inverse of the
    91 x 91 basis submatrix by Gauss-Jordan, then EVERY pattern of order <= 2 as (h on the basis + e) x inverse x G"""
    G = so.generator_matrix()
    llr = np.asarray(llr, np.float32)
    mags = np.abs(llr).view(np.uint32)
    order = sorted(range(174), key=lambda i: (-int(mags[i]), i))
    cols = [int("".join(map(str, G[:, c])), 2) for c in range(174)]
    reduced, basis = {}, []                                   # top bit -> vector
    for c in order:
        v = cols[c]
        while v:
            t = v.bit_length()
            if t not in reduced:
                reduced[t] = v
                basis.append(c)
                break
            v ^= reduced[t]
        if len(basis) == 91:
            break
    A = np.concatenate([G[:, basis], np.eye(91, dtype=np.uint8)], axis=1)
    for c in range(91):
        p = c + int(np.flatnonzero(A[c:, c])[0])
        A[[c, p]] = A[[p, c]]
        for r in np.flatnonzero(A[:, c]):
            if r != c:
                A[r] ^= A[c]
    inv = A[:, 91:]
    h = (llr > 0).astype(np.uint8)
    w = np.array([255 if abs(float(v)) >= 32.0 else int(np.float32(abs(v)) * np.float32(8.0)) for v in llr], np.int64)
    E = [np.zeros(91, np.uint8)]
    for k in range(91):
        e = np.zeros(91, np.uint8); e[k] = 1; E.append(e)
    for i in range(91):
        for j in range(i + 1, 91):
            e = np.zeros(91, np.uint8); e[i] = e[j] = 1; E.append(e)
    E = np.array(E)
    msgs = ((E ^ h[basis][None, :]).astype(np.float32) @ inv.astype(np.float32)).astype(np.int64) & 1
    C = ((msgs.astype(np.float32) @ G.astype(np.float32)).astype(np.int64) & 1).astype(np.uint8)
    metrics = (C ^ h[None, :]).astype(np.int64) @ w
    return np.array(basis), C, metrics


def test_best_pattern_against_brute_force_on_crowded_frames(oracle):
    """every failing candidate of 16 frames of 20 signals: the best pattern is a codeword, differs from h on the basis in at
    most `order` positions, and no pattern of that order has a smaller (metric, index)"""
    import ft8_spec_messages as sm
    import rtlsdr_ft8d_amd as ft8
    H = so.parity_check_matrix().astype(np.int32)
    iq = _cq_frames(oracle, range(1000, 1016), 20)
    mag, cands, counts, status = sm.oracle_stages(oracle, iq)
    st = status.view(ft8.STATUS_DTYPE).reshape(len(iq), -1)
    seen = 0
    for f in range(len(iq)):
        for i in range(int(counts[f])):
            if st[f, i]["ok"] != 0 or st[f, i]["ldpc_errors"] == 0:
                continue
            llr = oracle.llr(mag[f], cands[f, i])
            res = so.search(llr)
            basis, C, metrics = _independent_search(llr)
            h = (llr > 0).astype(np.uint8)
            for order in range(3):
                metric, pat, nhard, c = res[order]
                assert not ((H @ c) & 1).any()
                assert int((c ^ h)[basis].sum()) <= order
                k = int(np.argmin(metrics[:so.NPAT[order]]))          # first minimum: ties to the smallest index
                assert (metric, pat) == (int(metrics[k]), k), (f, i, order)
                assert np.array_equal(c, C[k]) and nhard == int((c ^ h).sum())
            seen += 1
    assert seen > 900


def test_noise_only_frames_decode_nothing(oracle):
    """96 frames without a signal (make_frame(seed, 0, ...), seeds 5000..5095): nothing is accepted at orders 1 and 2 with
    the gate wide open"""
    import ft8_spec_messages as sm
    iq = _cq_frames(oracle, range(5000, 5096), 0)
    mag, cands, counts, status = sm.oracle_stages(oracle, iq)
    searches = {}
    for order in (1, 2):
        out, info = so.osd_candidates(oracle, mag, cands, counts, status, order, 174, searches=searches)
        assert (info["result"] == 1).sum() == 0 and out.tobytes() == status.tobytes()
        assert (info["result"] >= 2).sum() > 800


def test_frozen_fixture(oracle):
    d = np.load(os.path.join(ROOT, "tests", "golden", "osd_frame.npz"))
    import rtlsdr_ft8d_amd as ft8
    cands = d["cands"].view(ft8.CAND_DTYPE).reshape(1, -1)
    searches = {}
    accepted = 0
    for order, gate in d["configs"]:
        st, info = so.osd_candidates(oracle, d["mag"], cands, d["counts"], d["status_in"], int(order), int(gate), searches=searches)
        assert st.tobytes() == d[f"status_o{order}_g{gate}"].tobytes(), (order, gate)
        assert info.tobytes() == d[f"info_o{order}_g{gate}"].tobytes(), (order, gate)
        accepted += int((info["result"] == 1).sum())
    assert accepted >= 3
