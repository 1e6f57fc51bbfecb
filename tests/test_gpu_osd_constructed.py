"""GPU tests of ordered-statistics decoding on constructed soft bits (tests/osd_craft.py): ft8gpu_osd_candidates against the
numpy restatement (tests/ft8_spec_osd.py) byte for byte on vectors synthesised radio frames never give it -- a pivot in the
third 64-column slot, saturated weights, zero and constant vectors, every result code, the gate on both sides of a planted
message's hard errors, the seams of the pattern index, tied metrics, a random sweep -- with fabricated status records, every
output pre-filled with 0xA5, in the host form (chunked), the device form and the device form in place; the frozen fixture.
tests/test_osd_constructed_cpu.py proves on the CPU that the cases are what their names say."""
import os

import numpy as np
import pytest

import ft8_spec_osd as so
import osd_craft as oc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = oc.FILL


@pytest.fixture(scope="module")
def built(oracle):
    """the cases in their frames and the restatement's answers at every (order, gate), computed once and not changed"""
    cases = oc.build_cases(oracle)
    frames = oc.build_frames(cases)
    mag = oc.waterfalls(oc.vectors_of(cases), frames)
    B = len(mag)
    fill_st = np.full((B, oc.CAP, 48), FILL, np.uint8)
    fill_info = np.full((B, oc.CAP * 8), FILL, np.uint8).view(so.INFO_DTYPE).reshape(B, oc.CAP)
    searches, want, inplace = {}, {}, {}
    for order, gate in oc.CONFIGS:
        want[(order, gate)] = so.osd_candidates(oracle, mag, frames["cands"], frames["counts"], frames["status_in"], order, gate,
                                                status_out=fill_st, info=fill_info, searches=searches)
        inplace[(order, gate)] = so.osd_candidates(oracle, mag, frames["cands"], frames["counts"], frames["status_in"], order, gate,
                                                   status_out=frames["status_in"], searches=searches)[0]
    for a in (mag, fill_st, fill_info, frames["status_in"], frames["cands"], frames["counts"]):
        a.setflags(write=False)
    return cases, frames, mag, fill_st, fill_info, want, inplace


def test_the_run_is_meaningful(oracle, built):
    """the tallies, from the restatement's answers: every result code, every pattern index of case g, a last pivot in the
    third slot, 1 / 2 / 3 / 4 saturated weights; an accepted record carries iters through and nothing else of status_in"""
    import rtlsdr_ft8d_amd as ft8
    cases, frames, mag, _, _, want, _ = built
    t = oc.tallies(oracle, cases, frames, mag, {k: v[1] for k, v in want.items()})
    print(t)
    assert t["results_seen"] == [0, 1, 2, 3, 4, 5, 6]
    assert tuple(t["case_g_patterns"]) == oc.G_PATTERNS
    assert t["max_last_pivot"] >= 128 and t["last_pivots_at_or_past_128"] >= 4
    assert all(t["saturated_weight_counts"].get(str(k), 0) >= 1 for k in (1, 2, 3, 4))
    where = oc.slots(frames)
    sin = frames["status_in"].view(ft8.STATUS_DTYPE).reshape(len(mag), -1)
    for ci, c in enumerate(cases):
        if c["case"] != "f":
            continue
        f, i = where[ci]
        for order in range(3):
            e = c["errors"]
            st, info = want[(order, e)]
            rec = st[f, i].view(ft8.STATUS_DTYPE)[0]
            assert tuple(info[f, i])[:3] == (1, e, 0) and rec["ok"] == 1 and rec["text"].decode() == c["text"]
            assert rec["iters"] == sin[f, i]["iters"] and rec["ldpc_errors"] == 0 and rec["pad"] == 0
            st, info = want[(order, e - 1)]
            assert tuple(info[f, i])[:3] == (2, e, 0) and st[f, i].tobytes() == frames["status_in"][f, i].tobytes()


def _first_difference(got_info, want_info, frames, cases):
    bad = np.argwhere(got_info.view(np.uint64) != want_info.view(np.uint64))
    if not len(bad):
        return None
    f, i = bad[0]
    ci = int(frames["vec"][f, i])
    return len(bad), (int(f), int(i)), cases[ci]["name"] if ci >= 0 else None, got_info[f, i], want_info[f, i]


@pytest.mark.parametrize("order", [0, 1, 2])
def test_stage_entry_equals_restatement_on_constructed_cases(built, order):
    """every gate of osd_craft.CONFIGS; host form chunked by max_frames 5 over 12 frames, device form out of place, device
    form in place"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    cases, frames, mag, fill_st, fill_info, want, inplace = built
    B = len(mag)
    cands, counts, status_in = frames["cands"], frames["counts"], frames["status_in"]
    with ft8.Decoder(device=0, max_frames=5, max_candidates=oc.CAP) as dec:
        ins = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda() for a in (mag, cands, counts, status_in)]
        for o, gate in oc.CONFIGS:
            if o != order:
                continue
            want_st, want_info = want[(order, gate)]
            got_st, got_info = dec.osd_candidates(mag, cands, counts, status_in, order, gate, status_out=fill_st, info=fill_info)
            assert got_info.tobytes() == want_info.tobytes(), (order, gate, _first_difference(got_info, want_info, frames, cases))
            assert got_st.tobytes() == want_st.tobytes(), (order, gate)
            out_d = torch.full((B, oc.CAP, 48), FILL, dtype=torch.uint8, device="cuda")
            info_d = torch.full((B, oc.CAP, 8), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dec.osd_candidates_dev(*ins, B, order, gate, out_d, info_d)
            dec.synchronize()
            assert info_d.cpu().numpy().tobytes() == want_info.tobytes() and out_d.cpu().numpy().tobytes() == want_st.tobytes(), (order, gate)
            same = ins[3].clone()
            info_d.fill_(FILL)
            torch.cuda.synchronize()
            dec.osd_candidates_dev(ins[0], ins[1], ins[2], same, B, order, gate, same, info_d)
            dec.synchronize()
            assert same.cpu().numpy().tobytes() == inplace[(order, gate)].tobytes(), (order, gate)
            assert info_d.cpu().numpy().tobytes() == want_info.tobytes(), (order, gate)


def test_frozen_constructed_fixture_on_the_device():
    import rtlsdr_ft8d_amd as ft8
    d = np.load(os.path.join(ROOT, "tests", "golden", "osd_constructed.npz"))
    B = len(d["counts"])
    frames = dict(cands=d["cands"].view(oc.CAND_DTYPE).reshape(B, -1), counts=d["counts"], status_in=d["status_in"], vec=d["vec"])
    mag = oc.waterfalls(d["vectors"], frames)
    cands = frames["cands"].view(ft8.CAND_DTYPE).reshape(B, -1)
    with ft8.Decoder(device=0, max_frames=B, max_candidates=cands.shape[1]) as dec:
        for order, gate in d["configs"]:
            st, info = dec.osd_candidates(mag, cands, d["counts"], d["status_in"], int(order), int(gate), status_out=d["status_in"])
            assert info.tobytes() == d[f"info_o{order}_g{gate}"].tobytes(), (order, gate)
            assert st.tobytes() == oc.fixture_status(d, order, gate).tobytes(), (order, gate)
