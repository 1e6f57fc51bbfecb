"""The second output path on constructed inputs (tests/messages_craft.py): ft8_noise_baseline_kernel and ft8_messages_kernel
(messages.hip), ft8_mask_kernel and ft8_append_kernel (multipass.hip) and dedup_dev.h / tone_dev.h behind them, through the stage
entries in host and device form, byte for byte against the numpy restatements (tests/ft8_spec_messages.py,
tests/ft8_spec_multipass.py), counts included, no tolerance.  Every output is pre-filled with 0xA5 and, in the device form, lies
between guard bands.  The append with empty record arrays and the waterfall's own baseline is held to the collect on the same
input, record for record: the two copies of the record arithmetic on the device against each other.
tests/test_messages_craft_cpu.py proves on the CPU what the families contain and which wrong rule each of them catches."""
import numpy as np
import pytest

import ft8_spec_messages as sm
import ft8_spec_multipass as smp
import messages_craft as mc

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, mc.FILL


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


def filled(B):
    import rtlsdr_ft8d_amd as ft8
    return np.full((B, 50 * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(B, 50)


def as_msgs(raw, B):
    import rtlsdr_ft8d_amd as ft8
    return raw.view(ft8.MESSAGE_DTYPE).reshape(B, 50)


@pytest.fixture(scope="module")
def expected():
    """per family and group, computed once: the baseline, the collect, and the family's own append where it has one"""
    out = {}
    for name in mc.FAMILIES:
        rows = []
        for g in mc.family(name)["groups"]:
            B = len(g["counts"])
            row = dict(base=sm.noise_baseline(g["mags"]),
                       collect=sm.collect(g["mags"], g["cands"], g["counts"], g["status"], min_score=g["min_score"], msgs=filled(B)))
            if "append" in g:
                ap = g["append"]
                row["append"] = smp.append(g["mags"], ap["base"], g["cands"], g["counts"], g["status"], ap["msgs"], ap["n_msgs"],
                                           min_score=g["min_score"])
            rows.append(row)
        out[name] = rows
    return out


@pytest.fixture(scope="module")
def chunking_decoder():
    """max_frames 2: every family walks through it in several chunks, the last one ragged where the frame count is odd"""
    import rtlsdr_ft8d_amd as ft8
    dec = ft8.Decoder(device=0, max_frames=2)
    yield dec
    dec.close()


def same(got, gn, want, wn):
    """None when counts and every byte agree (the slots past a count must still hold the caller's bytes), else what differs"""
    if np.array_equal(gn, wn) and got.tobytes() == want.tobytes():
        return None
    d = sm.check(got, gn, want, wn)
    if d is not None:
        return d
    f, j = np.argwhere(got.view(np.uint8).reshape(len(wn), 50, 64) != want.view(np.uint8).reshape(len(wn), 50, 64))[0][:2]
    return f"frame {f} slot {j} (behind the count {int(wn[f])}) was written"


def run_collect(dec, g, form):
    import torch
    B = len(g["counts"])
    if form == "host":
        return dec.collect_messages(g["mags"], g["cands"], g["counts"], g["status"], msgs=filled(B))
    ins = [up(g[k]) for k in ("mags", "cands", "counts", "status")]
    m_b, n_b = guarded(filled(B)), guarded(np.full(B, -0x5A5A5A5B, np.int32))
    torch.cuda.synchronize()
    dec.collect_messages_dev(*ins, B, m_b[GUARD:], n_b[GUARD:])
    dec.synchronize()
    for k, t in zip(("mags", "cands", "counts", "status"), ins):
        assert t.cpu().numpy().tobytes() == g[k].tobytes(), f"input {k} was written"
    return as_msgs(unguard(m_b, B * 3200), B), unguard(n_b, 4 * B).view(np.int32)


def run_append(dec, g, base, msgs, n_msgs, form):
    import torch
    B = len(g["counts"])
    if form == "host":
        return dec.append_messages(g["mags"], base, g["cands"], g["counts"], g["status"], msgs, n_msgs)
    ins = [up(a) for a in (g["mags"], base, g["cands"], g["counts"], g["status"])]
    m_b, n_b = guarded(msgs), guarded(np.ascontiguousarray(n_msgs, np.int32))
    torch.cuda.synchronize()
    dec.append_messages_dev(*ins, B, m_b[GUARD:], n_b[GUARD:])
    dec.synchronize()
    assert ins[1].cpu().numpy().tobytes() == np.ascontiguousarray(base).tobytes()
    return as_msgs(unguard(m_b, B * 3200), B), unguard(n_b, 4 * B).view(np.int32)


def decoder_for(form, gpu_decoder, chunking_decoder):
    """host form: chunked at 2 frames; device form: one chunk of up to 16"""
    return chunking_decoder if form == "host" else gpu_decoder


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", mc.FAMILIES)
def test_collect_messages(gpu_decoder, chunking_decoder, expected, name, form):
    dec = decoder_for(form, gpu_decoder, chunking_decoder)
    bad = []
    try:
        for g, row in zip(mc.family(name)["groups"], expected[name]):
            dec.set_params(min_score=g["min_score"], max_candidates=g["cap"])
            got, gn = run_collect(dec, g, form)
            d = same(got, gn, *row["collect"])
            if d is not None:
                bad.append((g["cap"], d))
    finally:
        dec.set_params(min_score=10, max_candidates=120)
    assert not bad, (name, form, bad[:4])


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", mc.FAMILIES)
def test_append_messages(gpu_decoder, chunking_decoder, expected, name, form):
    """(a) no records yet and the waterfall's own baseline: the append is the collect, record for record -- against the
    restatement and against what ft8_messages_kernel itself wrote for the same input; (b) the family's own append view (seed
    records, n_msgs in-values outside [0, 50], a base that is not the waterfall's baseline) against the restatement"""
    dec = decoder_for(form, gpu_decoder, chunking_decoder)
    bad = []
    try:
        for g, row in zip(mc.family(name)["groups"], expected[name]):
            dec.set_params(min_score=g["min_score"], max_candidates=g["cap"])
            B = len(g["counts"])
            base = dec.noise_baseline(g["mags"])
            assert np.array_equal(base, row["base"])
            got, gn = run_append(dec, g, base, filled(B), np.zeros(B, np.int32), form)
            d = same(got, gn, *row["collect"])
            if d is not None:
                bad.append((g["cap"], "own base", d))
            cm, cn = run_collect(dec, g, form)
            if not (np.array_equal(cn, gn) and cm.tobytes() == got.tobytes()):
                bad.append((g["cap"], "append != collect on the device", sm.check(got, gn, cm, cn)))
            if "append" in g:
                ap = g["append"]
                got, gn = run_append(dec, g, ap["base"], ap["msgs"], ap["n_msgs"], form)
                d = same(got, gn, *row["append"])
                if d is not None:
                    bad.append((g["cap"], "own view", d))
    finally:
        dec.set_params(min_score=10, max_candidates=120)
    assert not bad, (name, form, bad[:4])


def test_append_follows_a_foreign_base(gpu_decoder, expected):
    """noise_window with a base that is not the waterfall's baseline: snr_db follows the base that was passed, so the records
    differ from the collect's in snr_db and in nothing else"""
    (g,), (row,) = mc.family("noise_window")["groups"], expected["noise_window"]
    ap = g["append"]
    got, gn = run_append(gpu_decoder, g, ap["base"], ap["msgs"], ap["n_msgs"], "host")
    assert same(got, gn, *row["append"]) is None
    cm, cn = row["collect"]
    assert np.array_equal(gn, cn)
    moved = 0
    for f in range(len(cn)):
        for j in range(int(cn[f])):
            a, b = got[f, j].copy(), cm[f, j].copy()
            moved += int(a["snr_db"]) != int(b["snr_db"])
            a["snr_db"] = b["snr_db"] = 0
            assert a.tobytes() == b.tobytes(), (f, j)
    assert moved > int(cn.sum()) // 2, moved


@pytest.mark.parametrize("name", mc.FAMILIES)
def test_noise_baseline_equals_np_partition(gpu_decoder, chunking_decoder, expected, name):
    import torch
    for g, row in zip(mc.family(name)["groups"], expected[name]):
        B = len(g["counts"])
        assert np.array_equal(chunking_decoder.noise_baseline(g["mags"]), row["base"])
        mag_d = up(g["mags"])
        b_b = guarded(np.full((B, 512), FILL, np.uint8))
        torch.cuda.synchronize()
        gpu_decoder.noise_baseline_dev(mag_d, B, b_b[GUARD:])
        gpu_decoder.synchronize()
        assert np.array_equal(unguard(b_b, 512 * B).reshape(B, 2, 256), row["base"])
        assert mag_d.cpu().numpy().tobytes() == g["mags"].tobytes()


def test_mask_edges_three_ways(gpu_decoder, chunking_decoder):
    """out of place (the input intact, guard bands), in place, and chunked at max_frames 2: the changed cells are the rule's set
    exactly, each holding the baseline of its column"""
    import torch
    (g,) = mc.family("mask_edges")["groups"]
    mk = g["mask"]
    mag, B = g["mags"], len(g["counts"])
    want = smp.mask(mag, mk["base"], mk["msgs"], mk["first"], mk["n_msgs"])
    rule = mc.mask_cells(mk["msgs"], mk["first"], mk["n_msgs"])

    def check(got, how):
        got = np.asarray(got).reshape(B, mc.MAG_ARRAY)
        for f in range(B):
            assert sorted(np.flatnonzero(got[f] != mag[f]).tolist()) == rule[f], (how, f)
        assert got.tobytes() == want.tobytes(), how
    check(chunking_decoder.mask_messages(mag, mk["base"], mk["msgs"], mk["first"], mk["n_msgs"]), "chunked")
    check(gpu_decoder.mask_messages(mag, mk["base"], mk["msgs"], mk["first"], mk["n_msgs"]), "host")
    ins = [up(a) for a in (mk["base"], mk["msgs"], mk["first"], mk["n_msgs"])]
    mag_b, out_b = guarded(mag), guarded(np.full((B, mc.MAG_ARRAY), FILL, np.uint8))
    torch.cuda.synchronize()
    gpu_decoder.mask_messages_dev(mag_b[GUARD:], *ins, B, out_b[GUARD:])
    gpu_decoder.synchronize()
    check(unguard(out_b, B * mc.MAG_ARRAY), "device, out of place")
    assert unguard(mag_b, B * mc.MAG_ARRAY).tobytes() == mag.tobytes(), "the input was written"
    gpu_decoder.mask_messages_dev(mag_b[GUARD:], *ins, B, mag_b[GUARD:])
    gpu_decoder.synchronize()
    check(unguard(mag_b, B * mc.MAG_ARRAY), "device, in place")
    for a, t in zip((mk["base"], mk["msgs"], mk["first"], mk["n_msgs"]), ins):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def test_dedup_spots_count_what_messages_count(gpu_decoder, expected):
    """dedup_dev.h is shared: ft8gpu_collect_spots numbers the unique messages of the dedup family as ft8gpu_collect_messages
    does, n_results == n_msgs on every frame"""
    bad = []
    try:
        for g, row in zip(mc.family("dedup")["groups"], expected["dedup"]):
            gpu_decoder.set_params(min_score=g["min_score"], max_candidates=g["cap"])
            _, nres = gpu_decoder.collect_spots(g["cands"], g["counts"], g["status"])
            _, n = gpu_decoder.collect_messages(g["mags"], g["cands"], g["counts"], g["status"])
            if not (np.array_equal(nres, n) and np.array_equal(n, row["collect"][1])):
                bad.append((g["cap"], nres.tolist(), n.tolist(), row["collect"][1].tolist()))
    finally:
        gpu_decoder.set_params(min_score=10, max_candidates=120)
    assert not bad, bad
