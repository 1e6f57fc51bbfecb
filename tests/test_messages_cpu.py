"""CPU tests of the messages path: the record layout the C compiler sees, the host-side text formatting, the SNR
estimate's accuracy on the oracle's waterfalls (through the numpy restatement the GPU tests hold the device to), the
checker itself, and the calibration record."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ft8_spec_messages as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ft8():
    import rtlsdr_ft8d_amd as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc"), "-j8"])
    m.load_library()
    return m


def test_message_record_layout(ft8):
    """ft8gpu_message: 64 bytes at the offsets the header documents, as gcc and g++ see it, and as MESSAGE_DTYPE says"""
    fields = ["text", "snr_db", "score", "freq_hz", "dt_s", "hash", "cand_index", "cand", "a91", "pad"]
    want = [0, 25, 26, 28, 32, 36, 38, 40, 48, 60]
    d = ft8.MESSAGE_DTYPE
    assert d.itemsize == 64 and [d.fields[k][1] for k in fields] == want
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"ft8gpu.h\"\nint main(void){ printf(\"%zu" + " %zu" * len(fields) + "\\n\", sizeof(ft8gpu_message)" + \
        "".join(f", offsetof(ft8gpu_message, {f})" for f in fields) + "); return 0; }\n"
    with tempfile.TemporaryDirectory() as td:
        for compiler, ext, std in (("gcc", "c", "-std=gnu17"), ("g++", "cpp", "-std=c++17")):
            src = os.path.join(td, f"t.{ext}")
            open(src, "w").write(prog)
            exe = os.path.join(td, f"t_{ext}")
            subprocess.check_call([compiler, std, "-I", os.path.join(ROOT, "include"), src, "-o", exe])
            assert list(map(int, subprocess.check_output([exe]).split())) == [64] + want, compiler


def _records():
    import rtlsdr_ft8d_amd as ft8
    m = np.zeros(3, ft8.MESSAGE_DTYPE)
    rows = [(b"CQ K1JT FN20", -7, 0.32, 1234.375), (b"K1ABC W9XYZ -15", 12, -0.16, 37.5), (b"TNX BOB 73 GL", -30, 2.4, 0.0)]
    for r, (t, s, dt, f) in zip(m, rows):
        r["text"], r["snr_db"], r["dt_s"], r["freq_hz"] = t, s, dt, f
    return m


def test_format_messages_on_fixed_records(ft8):
    m = _records()
    want = "".join("%3d %4.1f %4d ~  %s\n" % (int(r["snr_db"]), float(r["dt_s"]), int(float(r["freq_hz"])), r["text"].decode()) for r in m)
    assert want == " -7  0.3 1234 ~  CQ K1JT FN20\n 12 -0.2   37 ~  K1ABC W9XYZ -15\n-30  2.4    0 ~  TNX BOB 73 GL\n"
    assert ft8.format_messages(m, 3) == want
    assert ft8.format_messages(m, 0) == ""
    # truncated to cap (NUL-terminated), the untruncated length returned
    lib = ft8.load_library()
    buf = C.create_string_buffer(b"\xAA" * 16, 16)
    n = lib.ft8gpu_format_messages(m.ctypes.data, 3, buf, 10)
    assert n == len(want)
    assert buf.raw[:10] == want[:9].encode() + b"\0" and buf.raw[10:] == b"\xAA" * 6
    assert lib.ft8gpu_format_messages(m.ctypes.data, 3, None, 0) == len(want)


def _accuracy_frames(oracle, snrs, seed):
    import snr_calibrate
    iq, snr, s0, texts = [], [], [], []
    for k, s in enumerate(snrs):
        a, b, c, d = snr_calibrate.synth_frames(oracle, 1, s, s, seed + k)
        iq.append(a)
        snr.append(b)
        s0.append(c)
        texts += d
    return np.concatenate(iq), np.concatenate(snr), np.concatenate(s0), texts


@pytest.fixture(scope="module")
def tools_path():
    import sys
    p = os.path.join(ROOT, "tools")
    if p not in sys.path:
        sys.path.insert(0, p)
    return p


def test_snr_estimate_accuracy_on_oracle_waterfalls(ft8, oracle, tools_path):
    """about 40 frames from -18 to +18 dB through the oracle's stages and the restatement: median |error| <= 1 dB, every
    decode within 2.5 dB"""
    import snr_calibrate
    snrs = np.repeat(np.arange(-18.0, 19.0, 4.0), 4)                  # 10 levels x 4 frames
    iq, snr, s0, texts = _accuracy_frames(oracle, snrs, 0x5EED)
    mag, cands, counts, status = spec.oracle_stages(oracle, iq)
    msgs, n = spec.collect(mag, cands, counts, status)
    err = []
    for f in range(len(n)):
        for j in range(int(n[f])):
            if msgs[f, j]["text"].decode() == texts[f]:
                err.append(int(msgs[f, j]["snr_db"]) - snr[f])
    assert len(err) >= 34, f"only {len(err)} of {len(snrs)} planted messages decoded"
    err = np.abs(np.array(err))
    assert np.median(err) <= 1.0, err
    assert err.max() <= 2.5, err
    assert snr_calibrate.SEED != 0x5EED                               # not the calibration's own frames


def test_dedup_restatement_counts_what_the_reference_counts(ft8, oracle):
    """n of the restatement == n_results of the oracle's ft8_subsystem on the same waterfalls (mixed traffic, one
    message heard twice per frame)"""
    import synth_util as S
    from rtlsdr_ft8d_amd import workload
    texts, tones = workload.mixed_message_pool(256, seed=3)
    iq = np.stack([S.make_mixed_frame(100 + k, 12, (-12.0, 6.0), texts, tones)[0] for k in range(6)])
    mag, cands, counts, status = spec.oracle_stages(oracle, iq)
    _, n = spec.collect(mag, cands, counts, status)
    _, ref_n = oracle.subsystem_from_waterfall_batch(mag, nthreads=8)
    assert np.array_equal(n, ref_n) and n.sum() > 30


def test_checker_fails_on_doctored_records(ft8, oracle):
    from rtlsdr_ft8d_amd import workload
    import synth_util as S
    texts, tones = workload.mixed_message_pool(128, seed=5)
    iq = np.stack([S.make_mixed_frame(7, 10, (-6.0, 10.0), texts, tones)[0]])
    mag, cands, counts, status = spec.oracle_stages(oracle, iq)
    msgs, n = spec.collect(mag, cands, counts, status)
    assert n[0] >= 3
    assert spec.check(msgs, n, msgs.copy(), n.copy()) is None
    flipped = msgs.copy()
    flipped[0, 1]["snr_db"] = np.int8(int(flipped[0, 1]["snr_db"]) ^ 1)
    assert spec.check(flipped, n, msgs, n) is not None
    swapped = msgs.copy()
    swapped[0, [0, 1]] = swapped[0, [1, 0]]
    assert spec.check(swapped, n, msgs, n) is not None
    assert spec.check(msgs, n + 1, msgs, n) is not None


def test_restatement_tones_match_the_oracle_encoder(ft8, oracle):
    """the restatement encodes the 91 stored bits of a91 (as the device does); where the CRC field matches the payload that is
    ft8_encode (the oracle's own) on the payload of a91"""
    from rtlsdr_ft8d_amd import workload
    texts, tones = workload.mixed_message_pool(64, seed=11)
    for t in texts:
        if t is None:
            continue
        p = ft8.pack77(t)
        a91 = np.zeros(12, np.uint8)
        a91[:10] = p
        crc = oracle.crc14(bytes(np.concatenate([a91[:9], [a91[9] & 0xF8], [0, 0]]).astype(np.uint8)), 82)
        a91[9] = (a91[9] & 0xF8) | (crc >> 11)
        a91[10] = (crc >> 3) & 0xFF
        a91[11] = (crc << 5) & 0xFF
        assert spec.crc_in_a91(a91) == spec.crc_of_payload(a91) == crc
        assert np.array_equal(spec.tones_of(a91), oracle.encode(np.concatenate([p, [0, 0]]).astype(np.uint8)))


def test_calibration_record_matches_the_source():
    cal = json.load(open(os.path.join(ROOT, "profiles", "snr_calibration.json")))
    assert cal["K"] == spec.calibration_k()
    assert cal["decodes"] >= 500 and cal["snr_range_db"] == [-20.0, 20.0]
    assert abs(cal["K_unrounded"] - cal["K"]) <= 0.005
    assert -0.2 < cal["d0_s"] < 0.2
