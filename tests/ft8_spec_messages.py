"""CPU restatement of the messages path (ft8gpu_decode_messages / ft8gpu_collect_messages / ft8gpu_noise_baseline) in
numpy, fed by the oracle's waterfall / find_sync / decode: the dedup order of rtlsdr_ft8d.c:1487-1520, the record fields,
the noise baseline and the SNR threshold rule (DESIGN.md "Every decoded message").  Every step of the SNR decision is the
same IEEE double operation in the same order as on the device, so records compare byte for byte."""
import functools
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_MESSAGES = 50
MAG_ARRAY = 94208
SNR_MIN, SNR_MAX = -30, 49
BASE_RANK = 46


@functools.lru_cache(None)
def calibration_k():
    """K as compiled into the library (csrc/api_messages.hip)"""
    src = open(os.path.join(ROOT, "rtlsdr_ft8d_amd", "csrc", "api_messages.hip")).read()
    return float(re.search(r"constexpr double kSnrCalibrationK = ([-0-9.eE+]+);", src).group(1))


@functools.lru_cache(None)
def power_table():
    return np.array([math.pow(10.0, float(v - 240) / 20.0) for v in range(256)], np.float64)


def threshold_table(k=None):
    return _threshold_table(calibration_k() if k is None else float(k))


@functools.lru_cache(None)
def _threshold_table(k):
    q = -math.log(0.75)
    return np.array([(1.0 + math.pow(10.0, (float(d) - 0.5 + k) / 10.0)) / q for d in range(SNR_MIN, SNR_MAX + 1)], np.float64)


def noise_baseline(mag):
    """[B][94208] -> uint8 [B][2][256]: the 47th smallest of mag[b][ts][fs][j] over (b, ts)"""
    m = np.asarray(mag, np.uint8).reshape(-1, 184, 2, 256)
    return np.partition(m, BASE_RANK, axis=1)[:, BASE_RANK].copy()


def lower_median(values):
    v = np.sort(np.asarray(values))
    return int(v[(len(v) - 1) // 2])


def snr_parts(mag, base, cand, tones):
    """(S, nsym, nb) of the estimate for one message: mag [94208] of its frame, base [2][256], its first candidate"""
    to, ts, fo, fs = int(cand["time_offset"]), int(cand["time_sub"]) & 1, int(cand["freq_offset"]), int(cand["freq_sub"]) & 1
    fo = min(max(fo, 0), 248)
    P = power_table()
    S, nsym = 0.0, 0
    for k in range(79):
        blk = to + k
        if 0 <= blk < 92:
            S = S + float(P[mag[blk * 1024 + ts * 512 + fs * 256 + fo + int(tones[k])]])
            nsym += 1
    js = [j for j in list(range(fo - 16, fo)) + list(range(fo + 8, fo + 24)) if 0 <= j < 256]
    nb = lower_median(base[fs][js])
    return S, nsym, nb


def snr_db(S, nsym, nb, k=None):
    P, T = power_table(), threshold_table(k)
    floor_sum = float(nsym) * float(P[nb])
    snr = SNR_MIN
    for d in range(SNR_MAX - SNR_MIN + 1):
        if S >= floor_sum * float(T[d]):
            snr = SNR_MIN + d
    return snr


def snr_continuous(S, nsym, nb, k=0.0):
    """10 log10(q S / (nsym P[nb]) - 1) - k (no rounding, no clamp): what the threshold rule rounds; None below 0"""
    r = -math.log(0.75) * S / (nsym * float(power_table()[nb])) - 1.0
    return None if r <= 0 else 10.0 * math.log10(r) - k


def tones_of(a91):
    """79 tones of a decoded message, encoded from the 91 bits of a91 AS STORED (payload and CRC field; the low five bits of
    a91[11] play no part), as tone_dev.h and the two whole-codeword encoders of the device do.  For a record whose CRC field
    matches its payload this is ft8_encode of the payload (tests/test_messages_cpu.py holds the two equal); a caller-made
    record whose CRC field does not match is encoded from the field it carries, not from a recomputed one."""
    import ft8_spec_refine
    return ft8_spec_refine.tones_of_a91(a91).astype(np.uint8)


def crc_of_payload(a91):
    """the CRC-14 ft8_encode appends to the 77-bit payload of a91 (bits 77..90 of the packed 91)"""
    import oracle_lib
    a = bytearray(bytes(a91)[:12])
    a[9] &= 0xF8
    a[10] = a[11] = 0
    return oracle_lib.crc14(bytes(a), 82)


def crc_in_a91(a91):
    a = bytes(a91)
    return ((a[9] & 0x07) << 11) | (a[10] << 3) | (a[11] >> 5)


def _c_text(raw25):
    b = bytes(raw25)[:25]
    return b.split(b"\0", 1)[0]


def collect(mag, cands, counts, status, min_score=10, msgs=None):
    """the restatement of ft8gpu_collect_messages.  mag [B][94208]; cands [B][cap] CAND_DTYPE; counts [B];
    status: [B][cap] STATUS_DTYPE or raw uint8 [B][cap][48]; msgs: the caller's array before the call (zeros if None).
    Returns (msgs [B][50] MESSAGE_DTYPE, n [B])."""
    import rtlsdr_ft8d_amd as ft8
    mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
    B = mag.shape[0]
    st = np.ascontiguousarray(status)
    if st.dtype != ft8.STATUS_DTYPE:
        st = st.view(np.uint8).reshape(B, -1, 48).view(ft8.STATUS_DTYPE).reshape(B, -1)
    out = np.zeros((B, MAX_MESSAGES), ft8.MESSAGE_DTYPE) if msgs is None else np.array(msgs, copy=True)
    n = np.zeros(B, np.int32)
    base = noise_baseline(mag)
    raw_status = st.view(np.uint8).reshape(B, -1, 48)
    cap = st.shape[1]
    for f in range(B):
        seen = []                                        # (hash, text) of the unique messages, in order
        for i in range(min(max(int(counts[f]), 0), cap)):              # idx < max_candidates && idx < counts[f]
            c = cands[f, i]
            r = st[f, i]
            if int(c["score"]) < min_score or r["ok"] == 0:           # :1467, :1476-1485
                continue
            text_raw = raw_status[f, i, 22:47].tobytes()
            key = (int(r["crc_extracted"]), _c_text(text_raw))
            if key in seen:                                            # :1487-1503
                continue
            seen.append(key)
            if len(seen) > MAX_MESSAGES:                               # table full: dropped (fence)
                continue
            rank = len(seen) - 1
            a91 = raw_status[f, i, 10:22].tobytes()
            S, nsym, nb = snr_parts(mag[f], base[f], c, tones_of(a91))
            rec = np.zeros(1, ft8.MESSAGE_DTYPE)[0]
            rec["text"] = text_raw
            rec["snr_db"] = snr_db(S, nsym, nb)
            rec["score"] = c["score"]
            rec["freq_hz"] = (np.float32(c["freq_offset"]) + np.float32(c["freq_sub"]) / np.float32(2)) * np.float32(6.25)
            rec["dt_s"] = (np.float32(c["time_offset"]) + np.float32(c["time_sub"]) / np.float32(2)) / np.float32(6.25)
            rec["hash"] = r["crc_extracted"]
            rec["cand_index"] = i
            rec["cand"] = c
            rec["a91"] = np.frombuffer(a91, np.uint8)
            out[f, rank] = rec
        n[f] = min(len(seen), MAX_MESSAGES)
    return out, n


def records_bytes(msgs, n):
    """the written part of a record array: bytes of slots [0, n[f]) per frame (for comparisons)"""
    return [msgs[f, :int(n[f])].tobytes() for f in range(len(n))]


def check(got_msgs, got_n, want_msgs, want_n):
    """None when the device's records equal the restatement's in every written byte and count, else a description"""
    got_n, want_n = np.asarray(got_n), np.asarray(want_n)
    if not np.array_equal(got_n, want_n):
        f = int(np.nonzero(got_n != want_n)[0][0])
        return f"frame {f}: n_msgs {int(got_n[f])} != {int(want_n[f])}"
    for f in range(len(want_n)):
        k = int(want_n[f])
        g, w = got_msgs[f, :k], want_msgs[f, :k]
        if g.tobytes() != w.tobytes():
            j = next(j for j in range(k) if g[j].tobytes() != w[j].tobytes())
            return f"frame {f} slot {j}: {g[j]} != {w[j]}"
    return None


def oracle_stages(oracle, iq, max_candidates=120, min_score=10, nthreads=8, iters=20):
    """oracle waterfall / find_sync / decode of B frames [B][2][48000] -> (mag, cands, counts, status uint8 [B][cap][48])"""
    mag = oracle.waterfall_batch(iq, nthreads=nthreads)
    cands, counts = oracle.find_sync_batch(mag, max_candidates, min_score, nthreads=nthreads)
    status = oracle.decode_candidates_batch(mag, cands, counts, iters=iters, nthreads=nthreads)
    return mag, cands, counts, status
