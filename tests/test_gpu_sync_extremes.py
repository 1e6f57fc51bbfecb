"""The sync search on waterfalls that reach its whole range (tests/sync_craft.py: scores +-255, numerators +-19125, every
residue of every navg class beyond |num| 8192, thresholds up to and across the saturation of the packed threshold, and the heap
orders radio frames never produce), byte for byte against the oracle: all 35 856 scores per frame, counts and ordered candidate
lists at every family's caps and thresholds through host and device pointers, both heap kernels of the A/B build, and the status
records of the full-contrast candidates.  No tolerance anywhere.  tests/test_sync_craft_cpu.py proves on the CPU that the frames
have the properties they are named for."""
import numpy as np
import pytest

import ft8_spec_decode as spec
import sync_craft as sc

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xA5
SPEC_TOO = ("full_scale", "thresholds")                       # also held against the independent numpy restatement


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


@pytest.fixture(scope="module")
def expected(oracle):
    """per family: the oracle's score maps and, per (max_candidates, min_score), its candidate lists (zeros behind the counts)"""
    out = {}
    for name in sc.FAMILIES:
        fam = sc.family(name)
        lists = {cfg: oracle.find_sync_batch(fam["mags"], cfg[0], cfg[1], nthreads=8) for cfg in fam["configs"]}
        out[name] = dict(scores=np.stack([oracle.score_map(m) for m in fam["mags"]]), lists=lists)
    return out


def differing(cands, counts, want_cands, want_counts):
    """frames whose count, list or tail differs"""
    return [k for k in range(len(want_counts)) if counts[k] != want_counts[k] or cands[k].tobytes() != want_cands[k].tobytes()]


@pytest.mark.parametrize("name", sc.FAMILIES)
def test_score_map(gpu_decoder, expected, name):
    fam = sc.family(name)
    want = expected[name]["scores"]
    try:
        for ms in (10, fam["configs"][-1][1]):                # the scores do not depend on the threshold the same launch applies
            gpu_decoder.set_params(min_score=ms)
            got = gpu_decoder.score_map(fam["mags"])
            assert got.shape == want.shape and got.dtype == want.dtype
            assert got.tobytes() == want.tobytes(), (name, ms, f"{int((got != want).sum())} scores differ, first at {np.argwhere(got != want)[:3].tolist()}")
    finally:
        gpu_decoder.set_params(min_score=10)
    if name in SPEC_TOO:
        for k, mag in enumerate(fam["mags"]):
            assert np.array_equal(got[k], spec.score_map(mag).astype(np.int16)), (name, k)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", sc.FAMILIES)
def test_find_sync(gpu_decoder, expected, name, form):
    import torch
    fam = sc.family(name)
    mags = fam["mags"]
    B = len(mags)
    bad = []
    try:
        mag_d = up(mags) if form == "device" else None
        for (cap, ms), (want_cands, want_counts) in expected[name]["lists"].items():
            gpu_decoder.set_params(min_score=ms, max_candidates=cap)
            if form == "host":
                cands, counts = gpu_decoder.find_sync(mags)
            else:
                c_b = guarded(np.full((B, cap), FILL, np.uint8).repeat(8, axis=1))     # every record has to be written, zeros behind the count
                n_b = guarded(np.full(B, -1, np.int32))
                torch.cuda.synchronize()
                gpu_decoder.find_sync_dev(mag_d, B, c_b[GUARD:], n_b[GUARD:])
                gpu_decoder.synchronize()
                cands = unguard(c_b, 8 * B * cap).view(want_cands.dtype).reshape(B, cap)
                counts = unguard(n_b, 4 * B).view(np.int32)
            bad += [(cap, ms, k) for k in differing(cands, counts, want_cands, want_counts)]
            if form == "host" and name in SPEC_TOO and (name == "full_scale" or cap == 120):
                for k in range(B):
                    mine = spec.find_sync(mags[k], cap, ms, scores=expected[name]["scores"][k].astype(np.int64))
                    assert sc.as_list(cands[k, :counts[k]]) == [tuple(c) for c in mine], (name, cap, ms, k)
        if form == "device":
            assert mag_d.cpu().numpy().tobytes() == mags.tobytes()
    finally:
        gpu_decoder.set_params(min_score=10, max_candidates=120)
    assert not bad, (name, form, bad[:8])


def _forced(ft8, form):
    return ft8.AB_HEAP_LANE_PER_FRAME if form == "lane" else ft8.AB_HEAP_WAVE_PER_FRAME


@pytest.mark.parametrize("form", ["lane", "wave"])
def test_heap_forms_on_the_heap_orders(oracle, expected, form):
    """ft8_heap_simt_kernel and the wave-per-frame kernel, each forced for every launch in the A/B build: the seven orders at
    the seven caps on 65 frames (one wave of the lane-per-frame kernel and a ragged second one) and on one frame at a time"""
    import rtlsdr_ft8d_amd as ft8
    fam = sc.family("heap_orders")
    mags = fam["mags"]
    pick = np.arange(65) % len(mags)
    bad = []
    with ft8.Decoder(device=0, max_frames=65, lib=ft8.load_ab_library()) as d:
        d.set_debug_flags(_forced(ft8, form))
        for (cap, ms), (want_cands, want_counts) in expected["heap_orders"]["lists"].items():
            d.set_params(min_score=ms, max_candidates=cap)
            cands, counts = d.find_sync(mags[pick])
            bad += [(65, cap, int(k)) for k in differing(cands, counts, want_cands[pick], want_counts[pick])]
            for k in range(len(mags)):
                cands, counts = d.find_sync(mags[k:k + 1])
                bad += [(1, cap, k) for _ in differing(cands, counts, want_cands[k:k + 1], want_counts[k:k + 1])]
    assert not bad, (form, bad[:8])


@pytest.mark.parametrize("form", ["lane", "wave"])
def test_heap_forms_on_the_other_families(expected, form):
    import rtlsdr_ft8d_amd as ft8
    bad = []
    with ft8.Decoder(device=0, max_frames=16, lib=ft8.load_ab_library()) as d:
        d.set_debug_flags(_forced(ft8, form))
        for name in ("full_scale", "quotients", "thresholds"):
            mags = sc.family(name)["mags"]
            for (cap, ms), (want_cands, want_counts) in expected[name]["lists"].items():
                d.set_params(min_score=ms, max_candidates=cap)
                cands, counts = d.find_sync(mags)
                bad += [(name, cap, ms, k) for k in differing(cands, counts, want_cands, want_counts)]
    assert not bad, (form, bad[:8])


def test_decode_candidates_at_full_contrast(oracle, gpu_decoder, expected):
    """every site of the full_scale frames that scores +255 (256 per frame, the time edges t0 = -12 and 23 among them) through the
    LLR extraction and the LDPC decoder: the status records of the oracle, byte for byte"""
    mags = sc.family("full_scale")["mags"]
    cands, counts = expected["full_scale"]["lists"][(480, 255)]
    assert (counts > 200).all() and {-12, 23} <= set(cands["time_offset"][cands["score"] == 255].tolist())
    want = oracle.decode_candidates_batch(mags, cands, counts, 20, 8)
    try:
        gpu_decoder.set_params(max_candidates=480)
        st = gpu_decoder.decode_candidates(mags, cands, counts)
    finally:
        gpu_decoder.set_params(max_candidates=120)
    got = st.view(np.uint8).reshape(want.shape)
    wrong = np.argwhere((got != want).any(axis=2))
    assert wrong.size == 0, f"{len(wrong)} of {int(counts.sum())} records differ, first (frame, candidate) {wrong[:3].tolist()}"
