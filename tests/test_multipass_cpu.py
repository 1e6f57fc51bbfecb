"""CPU tests of multi-pass decoding: the entries are declared and exported, the restatement's mask rule has the properties
the device relies on (masking the first pass's waterfall with every record so far == masking pass by pass; idempotent),
its later passes keep the first pass's records and never shrink a count, and the committed gain profile is what
tools/multipass_gain.py measures."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ft8_spec_messages as sm
import ft8_spec_multipass as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc"), "-j8"])
    m.load_library()
    return m


def test_multipass_entries_declared_and_exported(ft8):
    hdr = open(os.path.join(ROOT, "include", "ft8gpu.h")).read()
    assert re.search(r"^#define FT8GPU_MAX_PASSES 4\b", hdr, re.M)
    lib = ft8.load_library()
    for name in ("ft8gpu_decode_messages_passes", "ft8gpu_mask_messages", "ft8gpu_append_messages"):
        assert name in ft8.ABI_SYMBOLS and hasattr(lib, name) and name + "(" in hdr, name
    for name in ("decode_messages_passes", "decode_messages_passes_dev", "mask_messages", "mask_messages_dev",
                 "append_messages", "append_messages_dev"):
        assert callable(getattr(ft8.Decoder, name)), name


def _crowded(oracle, seeds, nsig=30):
    import synth_util as S
    enc = S.oracle_encode_fn(oracle)
    fr = [S.make_frame(s, nsig, enc, snr_range=(-22.0, 0.0)) for s in seeds]
    return np.stack([f[0] for f in fr]), [f[1] for f in fr]


def test_mask_rule_properties(ft8, oracle):
    iq, _ = _crowded(oracle, range(1000, 1008))
    stages = sm.oracle_stages(oracle, iq)
    msgs, n, nbp = spec.decode_passes(oracle, iq, 3, stages=stages)
    mag = stages[0]
    base = sm.noise_baseline(mag)
    zero = np.zeros(len(n), np.int32)
    # pass by pass (the rule) == the first pass's waterfall masked with every record so far (what the device computes)
    W = mag
    for p in range(3):
        W = spec.mask(W, base, msgs, zero if p == 0 else nbp[:, p - 1], nbp[:, p])
    once = spec.mask(mag, base, msgs, zero, n)
    assert W.tobytes() == once.tobytes()
    assert spec.mask(once, base, msgs, zero, n).tobytes() == once.tobytes()           # idempotent
    assert (once != mag).any(axis=1).all()
    # a masked cell holds the baseline of its column
    diff = np.nonzero(once != mag)
    cols = diff[1] % 512
    assert np.array_equal(once[diff], base.reshape(len(n), 512)[diff[0], cols])


def test_later_passes_keep_the_first_and_never_shrink(ft8, oracle):
    iq, planted = _crowded(oracle, range(1100, 1112))
    stages = sm.oracle_stages(oracle, iq)
    m1, n1 = sm.collect(*stages)
    for passes in (1, 2, 3):
        m, n, nbp = spec.decode_passes(oracle, iq, passes, stages=stages)
        assert np.array_equal(nbp[:, 0], n1) and np.array_equal(nbp[:, -1], n)
        assert (np.diff(nbp, axis=1) >= 0).all()
        assert sm.records_bytes(m, n1) == sm.records_bytes(m1, n1)
        for f in range(len(n)):                                        # appended records: unique, index this pass's list
            keys = [(int(r["hash"]), r["text"]) for r in m[f, :n[f]]]
            assert len(set(keys)) == len(keys)
            assert all(bytes(r["pad"]) == b"\0\0\0\0" for r in m[f, :n[f]])
    hit, miss = spec.planted_hits(m, n, planted)
    hit1, _ = spec.planted_hits(m1, n1, planted)
    assert hit > hit1 and miss == 0


def test_gain_profile_is_what_the_tool_measures(ft8, oracle):
    """profiles/multipass_gain.json, CQ at 30 signals per frame: recomputed with the restatement over the same 96 frames"""
    doc = json.load(open(os.path.join(ROOT, "profiles", "multipass_gain.json")))
    row = next(r for r in doc["rows"] if r["traffic"] == "cq" and r["signals_per_frame"] == 30)
    lo, hi = doc["seeds"]
    iq, planted = _crowded(oracle, range(lo, hi + 1))
    m, n, nbp = spec.decode_passes(oracle, iq, 3)
    got = []
    for p in range(3):
        got.append(sum(1 for f in range(len(n)) for r in m[f, :nbp[f, p]] if r["text"].decode() in planted[f]))
    assert got == row["correct_by_pass"] and row["outside_planted_by_pass"] == [0, 0, 0]
    assert got[1] > got[0]
