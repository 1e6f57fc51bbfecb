"""CPU tests of the soft-bit memory (include/ft8gpu.h "soft-bit memory"): the struct layouts against gcc, ft8gpu_softmem_reset,
the restatement tests/ft8_spec_combine.py on the constructed cases of tests/combine_craft.py -- each case has the property it
is named for, and the frozen fixture tests/golden/combine_constructed.npz (which the device is held to as well) is reproduced;
the two writings of bp_decode (numpy and the oracle's C) on the guard cases; the update rule over ring wrap-around,
store_per_slot 0, 1 and 128 and a partner overwritten in the same slot; the 2 x 4 stream scenario, where slot 2 gains messages
only through combining.  No GPU is used here."""
import os
import subprocess

import numpy as np
import pytest

import combine_craft as cc
import ft8_spec_combine as sc
import ft8_spec_messages as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc"), "-j8"])
    m.load_library()
    return m


@pytest.fixture(scope="module")
def built(oracle, ft8):
    cases = cc.build_cases(oracle)
    placed = cc.place(oracle, cases)
    return cases, placed, cc.expected(oracle, placed)


# ---- layouts, reset ---------------------------------------------------------------------------------------------------------------

def test_struct_layouts_against_gcc(ft8, tmp_path):
    """sizeof / offsetof of the four records as gcc lays them out, against the numpy dtypes of the binding and of the restatement"""
    src = tmp_path / "layout.c"
    fields = [("ft8gpu_softmem_entry", f) for f in ("cand", "used", "count", "pad", "stamp", "llr")] + \
             [("ft8gpu_softmem_state", f) for f in ("entry", "cursor", "slot", "pad")] + \
             [("ft8gpu_combine_info", f) for f in ("result", "nagree", "index", "count", "nhard", "pad")] + \
             [("ft8gpu_combine_params", f) for f in ("min_agree", "max_age", "store_per_slot")]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ft8gpu.h"', 'int main(void) {']
    for t in ("ft8gpu_softmem_entry", "ft8gpu_softmem_state", "ft8gpu_combine_info", "ft8gpu_combine_params"):
        lines.append(f'printf("{t} %zu\\n", sizeof({t}));')
    for t, f in fields:
        lines.append(f'printf("{t}.{f} %zu\\n", offsetof({t}, {f}));')
    lines.append('printf("entries %d min_agree %d store %d\\n", FT8GPU_SOFTMEM_ENTRIES, FT8GPU_COMBINE_MIN_AGREE, FT8GPU_COMBINE_STORE_PER_SLOT);')
    lines += ["return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=gnu17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines()[:-1])
    last = subprocess.check_output([str(exe)], text=True).splitlines()[-1].split()
    want = {"ft8gpu_softmem_entry": 720, "ft8gpu_softmem_state": 92176, "ft8gpu_combine_info": 8, "ft8gpu_combine_params": 12}
    for name, dt in (("ft8gpu_softmem_entry", ft8.SOFTMEM_ENTRY_DTYPE), ("ft8gpu_softmem_state", ft8.SOFTMEM_STATE_DTYPE),
                     ("ft8gpu_combine_info", ft8.COMBINE_INFO_DTYPE)):
        assert dt.itemsize == want[name]
        for f in dt.names:
            want[f"{name}.{f}"] = dt.fields[f][1]
    want.update({"ft8gpu_combine_params.min_agree": 0, "ft8gpu_combine_params.max_age": 4, "ft8gpu_combine_params.store_per_slot": 8})
    assert {k: int(v) for k, v in got.items()} == want
    assert sc.ENTRY_DTYPE == ft8.SOFTMEM_ENTRY_DTYPE and sc.STATE_DTYPE == ft8.SOFTMEM_STATE_DTYPE and sc.INFO_DTYPE == ft8.COMBINE_INFO_DTYPE
    assert [int(last[1]), int(last[3]), int(last[5])] == [ft8.SOFTMEM_ENTRIES, ft8.COMBINE_MIN_AGREE, ft8.COMBINE_STORE_PER_SLOT]
    assert ft8.SOFTMEM_ENTRIES == sc.ENTRIES == 128 and 0 <= ft8.COMBINE_MIN_AGREE <= 174 and 0 <= ft8.COMBINE_STORE_PER_SLOT <= 128
    assert C_sizeof_params(ft8) == 12


def C_sizeof_params(ft8):
    import ctypes as C
    return C.sizeof(ft8.CombineParams)


def test_softmem_reset(ft8):
    st = np.frombuffer(np.random.default_rng(1).integers(0, 256, sc.STATE_DTYPE.itemsize * 2, dtype=np.uint8).tobytes(), ft8.SOFTMEM_STATE_DTYPE).copy()
    keep = st[1:2].tobytes()
    ft8.softmem_reset(st[0:1])
    assert st[0:1].tobytes() == bytes(sc.STATE_DTYPE.itemsize) and st[1:2].tobytes() == keep
    assert ft8.softmem_state(3).tobytes() == bytes(3 * sc.STATE_DTYPE.itemsize)
    ft8.load_library().ft8gpu_softmem_reset(None)                      # a NULL state is ignored


# ---- the constructed cases -----------------------------------------------------------------------------------------------------

def test_frozen_constructed_fixture(built):
    cases, placed, want = built
    d = cc.load_golden()
    assert d["where"] == placed["where"] and [str(n) for n in d["frame_names"]] == [fr["name"] for fr in cases]
    for key in ("mag", "counts", "status_in"):
        assert np.array_equal(d[key], placed[key]), key
    assert d["cands"].tobytes() == placed["cands"].tobytes() and d["states"].tobytes() == placed["states"].tobytes()
    for name, _age, _gate in cc.CONFIGS:
        status, info, after = want[name]
        assert d["status_" + name].tobytes() == status.tobytes(), name
        assert d["info_" + name].tobytes() == info.tobytes(), name
        for s in cc.STORES:
            assert d[f"after_{name}_{s}"].tobytes() == after[s].tobytes(), (name, s)
    assert os.path.getsize(cc.GOLDEN) < 1 << 20


def test_constructed_cases_are_what_they_are_named_for(oracle, ft8, built):
    cases, placed, want = built
    assert want["open"][1].dtype == ft8.COMBINE_INFO_DTYPE and placed["states"].dtype == ft8.SOFTMEM_STATE_DTYPE
    by = {c["name"]: (fr, c) for fr in cases for c in fr["cands"]}
    at = placed["where"]
    B, cap = placed["cands"].shape

    def info(config, name):
        return want[config][1][at[name]]

    def rec(config, name):
        f, i = at[name]
        return want[config][0].view(ft8.STATUS_DTYPE).reshape(B, cap)[f, i]

    # every result code the rule can give (5 cannot be reached: bp_decode leaves at an all-zero word before it counts)
    seen = {int(r) for name in ("open", "gate") for r in want[name][1]["result"][np.arange(cap)[None, :] < placed["counts"][:, None]]}
    assert seen == {0, 1, 3, 4, 6, 7, 8}
    for name, code in (("a_accept", 1), ("a_crc", 3), ("a_unpack", 4), ("a_none", 7), ("a_allzero", 7), ("a_own6", 6)):
        assert info("open", name)["result"] == code, name
    assert info("open", "a_own6").tobytes() == bytes([6, 0, 0, 0, 0, 0, 0, 0])
    r = rec("open", "a_accept")
    f, i = at["a_accept"]
    sin = placed["status_in"].view(ft8.STATUS_DTYPE).reshape(B, cap)[f, i]
    assert r["ok"] == 1 and r["ldpc_errors"] == 0 and r["text"] == b"CQ K1ABC FN42" and r["iters"] == sin["iters"]
    assert r["crc_extracted"] == r["crc_calculated"] and r["pad"] == 0
    for name in ("a_crc", "a_unpack", "a_none"):                       # otherwise the record is unchanged
        f, i = at[name]
        assert want["open"][0][f, i].tobytes() == placed["status_in"][f, i].tobytes()
    # b: the gate at the boundary
    for nag in (cc.GATE, cc.GATE - 1, 174, 0):
        name = f"b_agree{nag}"
        assert info("open", name)["nagree"] == nag and info("gate", name)["nagree"] == nag
        assert (info("gate", name)["result"] == 8) == (nag < cc.GATE) and info("open", name)["result"] != 8
        assert (info("full", name)["result"] == 8) == (nag < 174)
    # c: ties
    for name in ("c_dist", "c_index", "c_nagree"):
        assert info("open", name)["index"] == by[name][1]["index"] and info("open", name)["result"] == 1, name
    fr = by["c_dist"][0]["state"][0]["entry"]
    assert (fr["llr"][5] > 0).tolist() == (fr["llr"][9] > 0).tolist() == (fr["llr"][3] > 0).tolist()
    # d, e: expiry at the boundary, across the wrap; dead entries
    for fr_name in ("d", "e"):
        assert info("open", f"{fr_name}_age0")["result"] == 1 and info("open", f"{fr_name}_age1")["result"] == 1
        assert info("aged", f"{fr_name}_age0")["result"] == 1 and info("aged", f"{fr_name}_age0")["count"] == 3
        assert info("aged", f"{fr_name}_age1").tobytes() == bytes(8)
        assert info("open", f"{fr_name}_dead").tobytes() == bytes(8)
    st_e = by["e_age0"][0]["state"][0]
    assert int(st_e["slot"]) == 2 and int(st_e["entry"]["stamp"][20]) > 1 << 31
    # f: what an entry may hold
    assert info("open", "f_count255")["count"] == 255 and info("open", "f_count255")["result"] == 7
    fc = info("open", "f_cancel")
    assert fc["result"] == 6 and fc["index"] == 66 and fc["nagree"] == 0
    f, i = at["f_cancel"]
    s = sc.summed(placed["states"][f]["entry"]["llr"][66], oracle.llr(placed["mag"][f], placed["cands"][f, i]))
    assert not s.any()
    for name in ("f_nan", "f_inf", "f_ninf"):
        assert info("open", name)["result"] == 6 and info("open", name)["index"] in (30, 31, 32) and info("open", name)["nagree"] > 100
    # g: the guard cases -- the normalised sum really holds the tiny values beside ordinary ones
    seen_tiny = set()
    for name, (fr, c) in by.items():
        if not name.startswith("g_"):
            continue
        f, i = at[name]
        idx = int(info("open", name)["index"])
        x = sc.normalized(sc.summed(placed["states"][f]["entry"]["llr"][idx], oracle.llr(placed["mag"][f], placed["cands"][f, i])))
        assert np.isfinite(x).all() and info("open", name)["result"] in (1, 7)
        tiny = np.abs(x[c["tiny"]])
        assert (tiny < 2.0 ** -80).all() and np.median(np.abs(x)) > 0.5
        bits = x[c["tiny"]].view(np.uint32)
        seen_tiny |= {"negzero" if b == 0x80000000 else "sub" if (b & 0x7F800000) == 0 and (b & 0x7FFFFFFF) else
                      "p120" if 0 < (b & 0x7FFFFFFF) < 0x07000000 else "p90" for b in bits}
    assert seen_tiny == {"negzero", "sub", "p120", "p90"}
    assert {int(info("open", n)["result"]) for n in by if n.startswith("g_")} == {1, 7}
    # h, i: nine offsets, and offset 2 ignored
    offs = set()
    for name, (fr, c) in by.items():
        if name[:2] in ("h_", "i_"):
            dt, df = c["off"]
            if max(abs(dt), abs(df)) <= 1:
                offs.add((dt, df))
                assert info("open", name)["result"] == 1, name
            else:
                assert info("open", name).tobytes() == bytes(8), name
    assert len(offs) == 9


def test_both_writings_of_bp_decode_agree_on_the_guard_cases(oracle, ft8, built):
    """numpy's bp_decode and the oracle's C bp_decode on the normalised sums with 2^-90, 2^-120, a subnormal and -0.0: the same
    word, error count and iteration count (float32 with subnormals kept on both sides)"""
    cases, placed, want = built
    assert placed["states"].dtype == ft8.SOFTMEM_STATE_DTYPE           # the fixture's memories are the library's records
    n = 0
    for name, (f, i) in placed["where"].items():
        if not name.startswith("g_"):
            continue
        idx = int(want["open"][1][f, i]["index"])
        x = sc.normalized(sc.summed(placed["states"][f]["entry"]["llr"][idx], oracle.llr(placed["mag"][f], placed["cands"][f, i])))
        a, b = sc.numpy_bp()(x, 20), oracle.bp_decode(x, 20)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], name
        n += 1
    assert n == 6


# ---- the update rule -------------------------------------------------------------------------------------------------------------

def test_update_rule_on_the_constructed_frames(oracle, ft8, built):
    cases, placed, want = built
    assert want["open"][2][128].dtype == ft8.SOFTMEM_STATE_DTYPE and max(cc.STORES) == ft8.SOFTMEM_ENTRIES
    at = placed["where"]
    names = [fr["name"] for fr in cases]
    old = placed["states"]
    status, info, after = want["open"]
    # store_per_slot 0: only the slot counter moves
    z = after[0]
    assert (z["slot"] == ((old["slot"].astype(np.int64) + 1) & 0xFFFFFFFF)).all() and (z["cursor"] == old["cursor"]).all()
    assert z["entry"].tobytes() == old["entry"].tobytes()
    # store_per_slot 1: exactly the first failing candidate with finite own
    one = after[1]
    fa = names.index("a")
    changed = np.flatnonzero([one[fa]["entry"][k].tobytes() != old[fa]["entry"][k].tobytes() for k in range(sc.ENTRIES)])
    assert changed.tolist() == [0] and one[fa]["cursor"] == 1
    # frame a at 128: accepted and own-6 candidates are not stored; BP-ran candidates store the sum with count + 1, the others own
    full = after[128]
    e = full[fa]["entry"]
    stored = [n for n in ("a_crc", "a_unpack", "a_none", "a_allzero") if True]
    cands = placed["cands"]
    got = {tuple(e["cand"][k].tolist()): k for k in range(int(full[fa]["cursor"]))}
    for n in stored:
        f, i = at[n]
        k = got[tuple(cands[f, i].tolist())]
        own = oracle.llr(placed["mag"][f], cands[f, i])
        s = sc.summed(old[f]["entry"]["llr"][int(info[f, i]["index"])], own)
        assert e["llr"][k][:174].tobytes() == s.tobytes() and e["count"][k] == 2 and e["stamp"][k] == old[f]["slot"] and e["used"][k] == 1
        assert not e["llr"][k][174:].any()
    for n in ("a_accept", "a_own6"):
        assert tuple(cands[at[n]].tolist()) not in got
    assert int(full[fa]["cursor"]) == 4
    # count saturates at 255
    ff = names.index("f")
    k = [k for k in range(sc.ENTRIES) if full[ff]["entry"]["cand"][k].tolist() == cands[at["f_count255"]].tolist() and full[ff]["entry"]["stamp"][k] == old[ff]["slot"]]
    assert len(k) == 1 and full[ff]["entry"]["count"][k[0]] == 255
    # the ring: cursor 126 + 384 wraps; the partner at 126 is overwritten by the first stored candidate, and the second one's
    # sum is still formed from what entry 126 held at entry to the slot
    fj = names.index("j")
    ej, oj = full[fj]["entry"], old[fj]["entry"]
    order = ["j_first", "j_partner_overwritten", "j_more0", "j_more1", "j_more2"]
    for rank, n in enumerate(order):
        k = (126 + rank) % 128
        assert ej["cand"][k].tolist() == cands[at[n]].tolist() and ej["stamp"][k] == 41, n
    f, i = at["j_partner_overwritten"]
    assert info[f, i]["result"] == 7 and info[f, i]["index"] == 126
    s = sc.summed(oj["llr"][126], oracle.llr(placed["mag"][f], cands[f, i]))
    assert ej["llr"][127][:174].tobytes() == s.tobytes() and ej["count"][127] == 8
    assert ej["llr"][126][:174].tobytes() == oracle.llr(placed["mag"][f], cands[at["j_first"]]).tobytes() and ej["count"][126] == 1
    assert int(full[fj]["cursor"]) == 3 and int(full[fj]["slot"]) == 42
    assert tuple(cands[at["j_accept_not_stored"]].tolist()) not in {tuple(ej["cand"][k].tolist()) for k in (126, 127, 0, 1, 2)}
    three = after[3][fj]
    assert int(three["cursor"]) == 1 and three["entry"][1].tobytes() == oj[1].tobytes()
    # the frame without candidates
    assert full[-1]["entry"].tobytes() == old[-1]["entry"].tobytes() and full[-1]["slot"] == old[-1]["slot"] + 1


# ---- the stream scenario ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stream(oracle, ft8):
    iq, texts = cc.scenario()
    R, S = iq.shape[:2]
    stages = sm.oracle_stages(oracle, iq.reshape(R * S, 2, -1), 120, 10, 8, 20)
    return iq, texts, stages


def test_stream_scenario_gains_only_through_combining(oracle, ft8, stream):
    """2 receivers x 4 slots, the same CQ messages in slots 0 / 2 and in 1 / 3: slot 0 and 1 gain nothing (nothing is
    remembered yet, or only other stations), slot 2 gains planted messages that BP alone does not decode in that slot, and
    nothing appended is outside the planted texts"""
    iq, texts, stages = stream
    assert iq.shape[0] * iq.shape[1] >= 8
    gains, (msgs, n, nbs, state) = cc.scenario_gains(oracle, iq, texts, ft8.COMBINE_MIN_AGREE, ft8.COMBINE_STORE_PER_SLOT, stages=stages)
    print("per slot (BP alone, gained, not planted):", gains)
    assert gains[0][1] == 0 and gains[2][1] >= 1
    assert all(bad == 0 for _b, _g, bad in gains)
    for r in range(iq.shape[0]):
        bp2 = {msgs[r, 2, k]["text"] for k in range(int(nbs[r, 2, 0]))}
        new = [msgs[r, 2, k] for k in range(int(nbs[r, 2, 0]), int(nbs[r, 2, 1]))]
        assert all(m["pad"][2] == 2 and m["text"] not in bp2 for m in new)
        assert all(m["pad"][2] == 0 for m in msgs[r, 2, :int(nbs[r, 2, 0])])
    assert (state["slot"] == 4).all()
    # without a memory (nothing stored) the path is ft8gpu_decode_messages
    gains0, (m0, n0, nbs0, st0) = cc.scenario_gains(oracle, iq, texts, ft8.COMBINE_MIN_AGREE, 0, stages=stages)
    assert all(g == 0 for _b, g, _x in gains0) and np.array_equal(nbs0[:, :, 0], nbs0[:, :, 1]) and not st0["entry"]["used"].any()
    # the numpy and the C writing of bp_decode give the same records on one receiver's slots 0 and 2
    a = sc.decode_combined(oracle, iq[:1, ::2], min_agree=ft8.COMBINE_MIN_AGREE, store_per_slot=16, max_candidates=24, bp=oracle.bp_decode)
    b = sc.decode_combined(oracle, iq[:1, ::2], min_agree=ft8.COMBINE_MIN_AGREE, store_per_slot=16, max_candidates=24)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
