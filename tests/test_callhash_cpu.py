"""CPU tests of the call hash table (include/ft8gpu.h "hashed call signs"): the restatement tests/ft8_spec_callhash.py against
properties of the rule and against expectations written out by hand, the frozen cases against the craft module that made
them, the host helpers of the library (plain C, no GPU) against the restatement, the struct layouts against gcc, the line
formatter, and the helpers under AddressSanitizer in a program of their own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import callhash_craft as cc
import ft8_spec_callhash as sc
import ft8_spec_pack as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    m.load_library()
    return m


@pytest.fixture(scope="module")
def golden():
    cases = cc.load_golden()
    for c in cases:
        for k in ("msgs", "n_msgs", "state", "resolved", "state_out"):
            c[k].setflags(write=False)
    return {c["name"]: c for c in cases}


def texts_of(resolved, n):
    """the texts without the blank the unpacker leaves behind a last call that no report follows (the bytes keep it)"""
    return [r["text"].decode().rstrip(" ") for r in resolved[:n]]


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def test_pinned_hashes_agree_with_the_protocol_formula():
    assert sp.call_hash("K1ABC", 22) == 2920267 and sp.call_hash("K1ABC", 12) == 2851 and sp.call_hash("PJ4/K1ABC", 22) == 1420834
    assert sp.call_hash("K1ABC", 22) >> 10 == sp.call_hash("K1ABC", 12)


def test_a_call_heard_in_slot_s_resolves_in_slot_s_and_s_plus_1(golden):
    c = golden["basic"]
    res, st = sc.resolve(c["msgs"], c["n_msgs"])
    # receiver 0: K1ABC and PJ4/K1ABC heard in slot 0, asked for in slot 1; PJ4/W9XYZ was never heard, PJ4/W1AW is heard there
    assert texts_of(res[0, 0], 2) == ["CQ K1ABC FN42", "CQ PJ4/K1ABC"]
    assert texts_of(res[0, 1], 3) == ["<K1ABC> PJ4/W1AW RR73", "<PJ4/K1ABC> W9XYZ -11", "<...> K1ABC R-03"]
    assert [int(x) for x in res[0, 1]["resolved_mask"][:3]] == [1, 1, 0] and [int(x) for x in res[0, 1]["n_hashed"][:3]] == [1, 1, 1]
    assert [int(x) for x in res[0, 1]["n_inserted"][:3]] == [1, 1, 1]
    # receiver 1: the hashed record at index 0 resolves against the full call at index 7 of the same slot, and in the next slot
    assert texts_of(res[1, 0], 9)[0] == "<KH1/KH7Z> K1ABC -09" and texts_of(res[1, 0], 9)[7:] == ["CQ KH1/KH7Z", "<KH1/KH7Z> W1AW 73"]
    assert texts_of(res[1, 1], 1) == ["KH7Z <KH1/KH7Z> RRR"]
    assert int(st[0]["slot"]) == 2 and int(st[1]["slot"]) == 2
    e = st[0]["entry"][2851]
    assert e["call"] == b"K1ABC      " and e["len"] == 5 and e["h22"] == 2920267
    assert st[0]["stamp"][2851] == 1 and st[0]["stamp"][1420834 >> 10] == 0       # K1ABC was heard again in slot 1, PJ4/K1ABC was not
    # receiver 1 never heard PJ4/K1ABC: receivers do not share a table
    assert st[1]["entry"][1420834 >> 10]["len"] == 0 and st[0]["entry"][1420834 >> 10]["call"] == b"PJ4/K1ABC  "


def test_type4_both_ways_reports_and_icq(golden):
    c = golden["type4"]
    res, st = sc.resolve(c["msgs"], c["n_msgs"])
    assert texts_of(res[0, 0], 9) == ["CQ K1ABC FN42", "<K1ABC> PJ4/K1ABC", "PJ4/K1ABC <K1ABC>", "<K1ABC> PJ4/K1ABC RRR",
                                      "PJ4/K1ABC <K1ABC> RR73", "<K1ABC> PJ4/K1ABC 73", "PJ4/K1ABC <...> 73", "CQ KH1/KH7Z",
                                      "W1AW <KH1/KH7Z> RRR"]
    assert texts_of(res[0, 1], 3) == ["<KH1/KH7Z> PJ4/K1ABC RR73", "<W1AW> KH1/KH7Z", "CQ W1AW/QRP"]
    # icq inserts and has no lookup
    assert (int(res[0, 0, 7]["n_hashed"]), int(res[0, 0, 7]["n_inserted"])) == (0, 1)
    assert st[0]["entry"][sp.call_hash("W1AW/QRP", 12)]["call"] == b"W1AW/QRP   "


def test_collisions_last_writer_wins(golden):
    (a, b), (c22, d22), drawn12, drawn22 = cc.colliding_pairs()
    assert sp.call_hash(a, 12) == sp.call_hash(b, 12) and sp.call_hash(a, 22) != sp.call_hash(b, 22)
    assert c22 != d22 and sp.call_hash(c22, 22) == sp.call_hash(d22, 22)
    assert drawn12 < 1000 and drawn22 < 20000
    g = golden["collide_12_record_order"]
    res, _ = sc.resolve(g["msgs"], g["n_msgs"])
    # records: 12-bit lookup of a, 22-bit of a, 22-bit of b, then the two CQs; the later CQ owns the entry
    assert texts_of(res[0, 0], 3) == [f"<{b}> PJ4/W1AW RR73", "<...> W9XYZ -11", f"<{b}> W9XYZ -11"]
    assert texts_of(res[1, 0], 3) == [f"<{a}> PJ4/W1AW RR73", f"<{a}> W9XYZ -11", "<...> W9XYZ -11"]
    g = golden["collide_12_field_order"]
    res, _ = sc.resolve(g["msgs"], g["n_msgs"])
    assert texts_of(res[0, 0], 4)[1:] == [f"<{b}> PJ4/W1AW RR73", "<...> W9XYZ -11", f"<{b}> W9XYZ -11"]
    assert texts_of(res[1, 0], 4)[1:] == [f"<{a}> PJ4/W1AW RR73", f"<{a}> W9XYZ -11", "<...> W9XYZ -11"]
    g = golden["collide_12_across_slots"]
    res, _ = sc.resolve(g["msgs"], g["n_msgs"])
    assert texts_of(res[0, 0], 2)[1] == f"<{a}> W9XYZ -11"
    assert texts_of(res[0, 1], 4)[1:] == [f"<{b}> PJ4/W1AW RR73", "<...> W9XYZ -11", f"<{b}> W9XYZ -11"]
    assert texts_of(res[0, 2], 2) == [f"<{a}> PJ4/W1AW RR73", f"<{a}> W9XYZ -11"]
    g = golden["collide_22"]
    res, _ = sc.resolve(g["msgs"], g["n_msgs"])
    assert texts_of(res[0, 0], 3)[1:] == [f"<{c22}> W9XYZ -11", f"<{c22}> PJ4/W1AW RR73"]
    assert texts_of(res[0, 1], 4)[1:] == [f"<{d22}> W9XYZ -11", f"<{d22}> W9XYZ -11", f"<{d22}> PJ4/W1AW RR73"]
    assert texts_of(res[0, 2], 2)[1] == f"<{c22}> W9XYZ -11"                 # "d c 73": c is the second field, the later writer


@pytest.mark.parametrize("wrap", ["", "_wrap"])
def test_ageing(golden, wrap):
    for max_age, alive in ((0, 4), (1, 2), (2, 3)):
        g = golden[f"age_{max_age}{wrap}"]
        res, st = sc.resolve(g["msgs"], g["n_msgs"], g["state"], max_age)
        for s in range(4):
            got = texts_of(res[0, s], 4 if s == 0 else 2)[-2:]
            want = ["<K1ABC> PJ4/W1AW RR73", "<PJ4/K1ABC> W9XYZ -11"] if s < alive else ["<...> PJ4/W1AW RR73", "<...> W9XYZ -11"]
            assert got == want, (max_age, wrap, s)
        assert int(st[0]["slot"]) == ((0xFFFFFFFE if wrap else 0) + 4) & 0xFFFFFFFF


def test_counts_are_clamped_and_empty_slots_count(golden):
    g = golden["counts"]
    res, st = cc.expected(g)                                             # on a prefill of JUNK bytes
    assert [int(x) for x in g["n_msgs"][0]] == [0, 50, 51, -1, 3]
    junk = bytes([cc.JUNK]) * 48
    assert all(res[0, 0, k].tobytes() == junk for k in range(50)) and all(res[0, 3, k].tobytes() == junk for k in range(50))
    assert res[0, 1].tobytes() == res[0, 2].tobytes()                    # 51 is clamped to 50
    assert int(res[0, 1]["n_resolved"][24:49].sum()) == 25               # the 50th record's call resolves the 25 before it
    # slot 0 had count 0: K1ABC was never inserted; W1AW's own frame had count -1, but the second record here carries it in clear
    assert texts_of(res[0, 4], 3) == ["<...> PJ4/W1AW 73", "<PJ4/K1ABC> W1AW 73", "<W1AW> PJ4/W1AW"]
    assert int(st[0]["slot"]) == 5


def test_long_texts_suffixes_and_plain_messages(golden):
    g = golden["long"]
    res, st = sc.resolve(g["msgs"], g["n_msgs"])
    A, B = cc.LONG_A, cc.LONG_B
    t = texts_of(res[0, 0], 12)
    assert t == [f"CQ {A}", f"CQ {B}", f"<{A}> <{B}> R FN20", f"<{B}> <{A}> RR73", "K1ABC/R W9XYZ EN37", "W1AW K9AN/P -05",
                 "<K1ABC> PJ4/W1AW", "<K9AN> PJ4/W1AW", "<PJ4/W1AW> K1ABC/R R FN42", f"<{A}> <...> R FN20", f"<...> <{B}> 73",
                 f"W9XYZ <{A}> -30"]
    assert len(t[2]) == 34 and max(map(len, t)) == 34
    assert [int(x) for x in res[0, 0]["resolved_mask"][[2, 9, 10, 11]]] == [3, 1, 2, 1]
    assert [int(x) for x in res[0, 0]["n_hashed"][[2, 9, 10, 11]]] == [2, 2, 2, 1]
    assert st[0]["entry"][sp.call_hash("K1ABC", 12)]["call"] == b"K1ABC      "       # the base call, not K1ABC/R
    g = golden["plain"]
    res, _ = sc.resolve(g["msgs"], g["n_msgs"])
    assert texts_of(res[0, 0], 6) == ["TNX BOB 73 GL", "123456789ABCDEF012", "CQ K1ABC FN42", "0F00000000000000FF", "A", "+-./? 0Z"]
    assert [int(x) for x in res[0, 0]["n_inserted"][:6]] == [0, 0, 1, 0, 0, 0] and not res[0, 0]["n_hashed"][:6].any()


def test_text_rule_on_texts_that_do_not_match_their_bits():
    """the text is copied from the record, the bits decide what resolves: a text without "<...>", one with three, one that
    fills all 25 bytes, and the cut at 39 characters"""
    assert sc.resolved_text(b"K1ABC W9XYZ -11".ljust(25, b"\0"), ["PJ4/K1ABC"]) == b"K1ABC W9XYZ -11"
    assert sc.resolved_text(b"<...> <...> <...>".ljust(25, b"\0"), ["A", None, "B"]) == b"<A> <...> <...>"
    assert sc.resolved_text(b"<...><...><...><...><...>", ["ABCDEFGHIJK", "ABCDEFGHIJK"]) == b"<ABCDEFGHIJK><ABCDEFGHIJK><...><...><.."
    assert sc.resolved_text(b"AB\0<...>".ljust(25, b"\0"), ["X"]) == b"AB"
    assert sc.resolved_text(b"<..><...".ljust(25, b"\0"), ["X"]) == b"<..><..."


def test_chunking_invariance_and_independent_receivers(golden):
    g = golden["chain"]
    msgs, n_msgs = g["msgs"], g["n_msgs"]
    whole, st = sc.resolve(msgs, n_msgs, max_age=2)
    assert int(whole["n_resolved"].sum()) >= 10 and int((whole["n_hashed"] - whole["n_resolved"]).sum()) >= 3
    for cuts in ((1, 1, 1, 1), (2, 2), (1, 3), (3, 1)):
        state, at, parts = None, 0, []
        for k in cuts:
            r, state = sc.resolve(msgs[:, at:at + k], n_msgs[:, at:at + k], state, 2)
            parts.append(r)
            at += k
        assert np.concatenate(parts, axis=1).tobytes() == whole.tobytes() and state.tobytes() == st.tobytes(), cuts
    perm = [2, 0, 1]
    r, s = sc.resolve(msgs[perm], n_msgs[perm], max_age=2)
    assert r.tobytes() == whole[perm].tobytes() and s.tobytes() == st[perm].tobytes()
    for k in range(3):
        r, s = sc.resolve(msgs[k:k + 1], n_msgs[k:k + 1], max_age=2)
        assert r.tobytes() == whole[k:k + 1].tobytes() and s.tobytes() == st[k:k + 1].tobytes()


def test_golden_file_is_what_the_craft_module_and_the_restatement_give(oracle, golden):
    cases = cc.build_cases(oracle)
    assert [c["name"] for c in cases] == list(golden)
    for c in cases:
        g = golden[c["name"]]
        assert c["msgs"].tobytes() == g["msgs"].tobytes() and np.array_equal(c["n_msgs"], g["n_msgs"]), c["name"]
        assert c["state"].tobytes() == g["state"].tobytes() and c["max_age"] == g["max_age"], c["name"]
        res, st = cc.expected(c)
        assert res.tobytes() == g["resolved"].tobytes() and st.tobytes() == g["state_out"].tobytes(), c["name"]
        # the text of every record is the unpacker's, with "<...>" for each hashed field the bits hold
        for r in range(len(c["printed"])):
            for s in range(len(c["printed"][r])):
                for k, shown in enumerate(c["printed"][r][s]):
                    assert shown.count("<...>") == len(sc.parse(c["msgs"][r, s, k]["a91"])[1]), shown


# ---- the host helpers of the library -----------------------------------------------------------------------------------------

def test_host_helpers_against_the_restatement(ft8):
    assert ft8.call_hash("K1ABC", 22) == 2920267 and ft8.call_hash("K1ABC", 12) == 2851 and ft8.call_hash("PJ4/K1ABC") == 1420834
    rng = np.random.default_rng(0xCA11)
    alphabet = np.array(list(sp.A_CALL11))
    state, spec = ft8.callhash_state(1), sc.new_state(1)
    assert state.dtype.itemsize == spec.dtype.itemsize == 81936
    calls = []
    for k in range(3000):
        if k % 3 == 0:
            call = cc.random_call(rng)
        else:
            call = "".join(rng.choice(alphabet, size=rng.integers(1, 12))).strip()
        if not call:
            continue
        for bits in (12, 22, 10, 1, 32):
            assert ft8.call_hash(call, bits) == sp.call_hash(call, bits), (call, bits)
        state["slot"] = spec["slot"] = k * 7919 % (1 << 32)
        ft8.callhash_insert(state, call)
        sc.insert(spec[0], call)
        calls.append(call)
    assert state.tobytes() == spec.tobytes()
    assert len({sp.call_hash(c, 12) for c in calls}) < len(set(calls))           # entries were overwritten on the way
    slot = int(spec["slot"][0])
    for call in calls[::7] + ["K1ABC", "NEVER/HEARD"]:
        for bits in (12, 22):
            h = sp.call_hash(call, bits)
            for max_age in (0, 1, 5000, 0xFFFFFFFF):
                for at in (slot, (slot + 5000) & 0xFFFFFFFF):
                    state["slot"] = spec["slot"] = at
                    assert ft8.callhash_lookup(state, bits, h, max_age) == sc.lookup(spec[0], bits, h, max_age), (call, bits, max_age)
    for bad in ("", " K1ABC", "K1ABC ", "k1abc", "K1ABC+", "ABCDEFGHIJKL"):
        with pytest.raises(ValueError):
            ft8.call_hash(bad)
        with pytest.raises(ValueError):
            ft8.callhash_insert(state, bad)
    with pytest.raises(ValueError):
        ft8.callhash_lookup(state, 12, 4096)
    with pytest.raises(ValueError):
        ft8.callhash_lookup(state, 10, 1)
    state[:] = np.frombuffer(bytes([0x5A]) * 81936, ft8.CALLHASH_STATE_DTYPE)
    ft8.callhash_reset(state)
    assert state.tobytes() == bytes(81936)


def test_struct_layouts_against_the_c_compiler(ft8, tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "ft8gpu.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ft8gpu_callhash_entry),
 offsetof(ft8gpu_callhash_entry, len), offsetof(ft8gpu_callhash_entry, h22), sizeof(ft8gpu_callhash_state),
 offsetof(ft8gpu_callhash_state, stamp), offsetof(ft8gpu_callhash_state, slot), offsetof(ft8gpu_callhash_state, pad),
 sizeof(ft8gpu_resolved), offsetof(ft8gpu_resolved, n_hashed), offsetof(ft8gpu_resolved, n_resolved),
 offsetof(ft8gpu_resolved, n_inserted), offsetof(ft8gpu_resolved, resolved_mask), offsetof(ft8gpu_resolved, pad),
 (size_t)FT8GPU_CALLHASH_ENTRIES); return 0; }'''
    src = tmp_path / "t.c"
    src.write_text(prog)
    vals = {}
    for cc_, std, name in (("gcc", "-std=gnu17", "c"), ("g++", "-std=c++17", "cpp")):
        exe = str(tmp_path / name)
        subprocess.check_call([cc_, std, "-x", "c" if name == "c" else "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
        vals[name] = list(map(int, subprocess.check_output([exe]).split()))
    assert vals["c"] == vals["cpp"] == [16, 11, 12, 81936, 65536, 81920, 81924, 48, 40, 41, 42, 43, 44, 4096]
    for dt in (ft8.CALLHASH_ENTRY_DTYPE, sc.ENTRY_DTYPE):
        assert dt.itemsize == 16 and [dt.fields[k][1] for k in ("call", "len", "h22")] == [0, 11, 12]
    for dt in (ft8.CALLHASH_STATE_DTYPE, sc.STATE_DTYPE):
        assert dt.itemsize == 81936 and [dt.fields[k][1] for k in ("entry", "stamp", "slot", "pad")] == [0, 65536, 81920, 81924]
    for dt in (ft8.RESOLVED_DTYPE, sc.RESOLVED_DTYPE):
        assert dt.itemsize == 48
        assert [dt.fields[k][1] for k in ("text", "n_hashed", "n_resolved", "n_inserted", "resolved_mask", "pad")] == [0, 40, 41, 42, 43, 44]
    assert ft8.CALLHASH_ENTRIES == sc.ENTRIES == 4096


def test_format_resolved(ft8, golden):
    g = golden["long"]
    msgs = np.array(g["msgs"][0, 0], copy=True)
    msgs["snr_db"][:12] = np.arange(-30, -18)
    msgs["dt_s"][:12] = np.linspace(-1.5, 2.0, 12, dtype=np.float32)
    msgs["freq_hz"][:12] = np.linspace(100.0, 2999.9, 12, dtype=np.float32)
    res = g["resolved"][0, 0]
    text = ft8.format_resolved(msgs, res, 12)
    want = "".join("%3d %4.1f %4d ~  %s\n" % (m["snr_db"], m["dt_s"], int(m["freq_hz"]), r["text"].decode()) for m, r in zip(msgs[:12], res[:12]))
    assert text == want and f"<{cc.LONG_A}> <{cc.LONG_B}> R FN20\n" in text
    # the same lines as format_messages, with the resolved text in place of the record's
    plain = ft8.format_messages(msgs, 12).splitlines()
    assert [a.split("~")[0] for a in plain] == [b.split("~")[0] for b in text.splitlines()]
    assert plain[2].endswith("<...> <...> R FN20")
    assert ft8.format_resolved(msgs, res, 0) == ""
    lib = ft8.load_library()
    buf = C.create_string_buffer(30)
    assert lib.ft8gpu_format_resolved(msgs.ctypes.data, np.ascontiguousarray(res).ctypes.data, 12, buf, 30) == len(want)
    assert buf.value.decode() == want[:29]
    assert lib.ft8gpu_format_resolved(None, None, 3, None, 0) == -1


def test_entries_refuse_bad_arguments_before_touching_a_gpu(ft8):
    lib = ft8.load_library()
    assert lib.ft8gpu_resolve_calls(None, None, None, 1, 1, None, 0, None, 0) == -1 and b"ctx is NULL" in lib.ft8gpu_last_error()
    assert lib.ft8gpu_decode_messages_resolved(None, None, 1, 1, None, None, 0, None, None, None, 0) == -1
    assert b"ctx is NULL" in lib.ft8gpu_last_error()


def test_host_helpers_under_asan_ubsan(tmp_path):
    """a program of its own (tests/host_asan/callhash_asan_main.c) linked with csrc/ft8_pack.c; nothing is loaded into python"""
    exe = str(tmp_path / "callhash_asan")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_asan", "callhash_asan_main.c"),
                           os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc", "ft8_pack.c"), "-lm", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "callhash_asan ok" in out.stdout, (out.stdout + out.stderr)[-3000:]
