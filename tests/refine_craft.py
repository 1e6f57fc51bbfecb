"""Frames and records for the tests of the refined time and frequency (tests/test_refine_cpu.py, tests/test_gpu_refine.py) and
for tools/refine_accuracy.py: the single-signal frames with known truth, and the constructed records of the stage entry."""
import numpy as np

import ft8_spec_osd as so
import ft8_spec_refine as sr
import synth_util as su

NSAMPLES = 48000
FILL = 0xA5
STRONG_DB, WEAK_DB = 0.0, -18.0               # a strong signal, and one near the threshold of belief propagation
TEXT = "CQ K1ABC FN42"


def a91_of_payload(payload):
    """the 12 bytes a decoded record carries: the 77 payload bits, the encoder's CRC-14, zeros"""
    bits = np.unpackbits(np.frombuffer(bytes(payload)[:10], np.uint8))[:77]
    crc = so.crc14(bits)
    all_bits = np.concatenate([bits, [(crc >> (13 - i)) & 1 for i in range(14)], np.zeros(5, np.int64)]).astype(np.uint8)
    return np.packbits(all_bits).tobytes()


def noisy_frame(rng, tones, f0, start, snr_db):
    """one signal in complex AWGN of unit variance per component, peak-normalised to 0.5 -> float32 [2][48000]"""
    fi, fq = rng.normal(0.0, 1.0, NSAMPLES), rng.normal(0.0, 1.0, NSAMPLES)
    si, sq = su.cpfsk(tones, f0, int(start), su.amplitude_for_snr(snr_db, 1.0))
    i32, q32 = (fi + si).astype(np.float32), (fq + sq).astype(np.float32)
    scale = np.float32(0.5) / max(np.abs(i32).max(), np.abs(q32).max())
    return np.stack([i32 * scale, q32 * scale]).astype(np.float32)


# ---- accuracy against known truth -------------------------------------------------------------------------------------------

def accuracy_frames(oracle, n, snr_db, seed):
    """n frames of one signal each, through the oracle's own synthesiser: f0 and the start sample uniform, off the grid.
    Returns (iq [n][2][48000], f0 [n] Hz, start [n] samples, text)."""
    rng = np.random.default_rng(seed)
    rc, payload = oracle.pack77(TEXT)
    assert rc == 0
    tones = oracle.encode(payload)
    amp = su.amplitude_for_snr(snr_db, 1.0)
    f0 = rng.uniform(200.0, 1400.0, n)
    start = rng.integers(320, 5440, n)                    # 0.1 s .. 1.7 s: every position modulo the grid's 256 samples
    iq = np.zeros((n, 2, NSAMPLES), np.float32)
    for f in range(n):
        si, sq = oracle.synth_cpfsk(tones, [f0[f]], [start[f]], [amp])
        i32 = (rng.normal(0.0, 1.0, NSAMPLES) + si).astype(np.float32)
        q32 = (rng.normal(0.0, 1.0, NSAMPLES) + sq).astype(np.float32)
        iq[f, 0], iq[f, 1] = oracle.normalise(i32, q32)
    return iq, f0, start, TEXT


def accuracy(oracle, iq, f0, start, text, nthreads=8):
    """decode with the oracle, refine with the restatement, estimate with the host helper.  Per decoded frame the absolute
    errors: dict of float arrays coarse_hz, refined_hz, coarse_samples (the record's dt_s, which names the first sample of the
    waterfall row, moved to the symbol's start by the lead of 256 samples), coarse_raw_samples (dt_s as it is), refined_samples,
    and snr_db (the refined estimates); decoded = how many frames carried the message."""
    import ft8_spec_messages as sm
    import rtlsdr_ft8d_amd as ft8
    mag, cands, counts, status = sm.oracle_stages(oracle, iq, nthreads=nthreads)
    msgs, n = sm.collect(mag, cands, counts, status)
    tw = sr.twiddles(oracle)
    out = {k: [] for k in ("coarse_hz", "refined_hz", "coarse_samples", "coarse_raw_samples", "refined_samples", "snr_db")}
    for f in range(len(n)):
        hit = [i for i in range(int(n[f])) if msgs[f, i]["text"].split(b"\0")[0].decode() == text]
        if not hit:
            continue
        m = msgs[f, hit[0]]
        rec = sr.refine_record(iq[f, 0], iq[f, 1], m["cand"], m["a91"].tobytes(), tw)
        dt, hz, snr, ok = ft8.refined_estimate(np.array([m]), np.array([rec]))
        assert ok[0] and (dt[0], hz[0], snr[0]) == sr.estimate(m["cand"], rec)
        out["coarse_hz"].append(abs(float(m["freq_hz"]) - f0[f]))
        out["refined_hz"].append(abs(float(hz[0]) - f0[f]))
        out["coarse_raw_samples"].append(abs(float(m["dt_s"]) * 3200.0 - start[f]))
        out["coarse_samples"].append(abs(float(m["dt_s"]) * 3200.0 + sr.LEAD - start[f]))
        out["refined_samples"].append(abs(float(dt[0]) * 3200.0 - start[f]))
        out["snr_db"].append(float(snr[0]))
    res = {k: np.array(v) for k, v in out.items()}
    res["decoded"] = len(out["coarse_hz"])
    return res


def summary(err):
    """median and 90th percentile of every error of accuracy()"""
    s = {"decoded": int(err["decoded"])}
    for k in ("coarse_hz", "refined_hz", "coarse_samples", "coarse_raw_samples", "refined_samples"):
        s[k] = {"median": round(float(np.median(err[k])), 4), "p90": round(float(np.percentile(err[k], 90)), 4)}
    s["snr_db_median"] = round(float(np.median(err["snr_db"])), 2)
    return s


# ---- constructed records for the stage entry -----------------------------------------------------------------------------------

def constructed(ft8):
    """3 frames and 50 records each, made by hand (a record need not be a decode):
      frame 0  noise and one strong signal, n_msgs = 50: time_offset -12 and 23 (windows leave the frame at both ends) with
               freq_offset 0 and 248 and (time_sub, freq_sub) in all four combinations; the signal's own record shifted so
               that the truth sits at e = +16, at e = -16 and at e = 0; records past every edge; random records
      frame 1  noise and the signal, n_msgs = 0
      frame 2  all zeros, n_msgs = 3
    Returns (iq [3][2][48000], msgs [3][50] MESSAGE_DTYPE, n_msgs [3], where: name -> (frame, slot))."""
    rng = np.random.default_rng(20261019)
    payload = ft8.pack77(TEXT)
    tones = ft8.encode(payload)
    a91 = np.frombuffer(a91_of_payload(payload), np.uint8)
    T_sig, F_sig = 9, 2 * 160 + 1                                     # on the grid: row 9, 1003.125 Hz
    start, f0 = 256 * T_sig + sr.LEAD, 3.125 * F_sig
    iq = np.zeros((3, 2, NSAMPLES), np.float32)
    iq[0] = noisy_frame(rng, tones, f0, start, 3.0)
    iq[1] = noisy_frame(rng, tones, f0, start, 3.0)
    msgs = np.zeros((3, 50), ft8.MESSAGE_DTYPE)
    msgs.view(np.uint8)[:] = rng.integers(0, 256, msgs.nbytes, dtype=np.uint8).reshape(msgs.view(np.uint8).shape)   # text, snr_db, ... are not read
    where = {}

    def put_raw(f, i, name, to, ts, fo, fs, a=a91):
        c = msgs[f, i]["cand"]
        c["score"], c["time_offset"], c["time_sub"], c["freq_offset"], c["freq_sub"] = 20, to, ts, fo, fs
        msgs[f, i]["a91"] = a
        where[name] = (f, i)

    def put(f, i, name, T, F, a=a91):
        put_raw(f, i, name, T >> 1, T & 1, F >> 1, F & 1, a)

    i = 0
    for to in (-12, 23):
        for fo in (0, 248):
            for ts in (0, 1):
                for fs in (0, 1):
                    put(0, i, f"edge_to{to}_fo{fo}_ts{ts}_fs{fs}", 2 * to + ts, 2 * fo + fs)
                    i += 1
    for name, T, F in (("truth_at_plus16", T_sig - 2, F_sig),            # 256 (T - 2) + 256 + 32 * 16 = start
                       ("truth_at_minus16", T_sig + 2, F_sig),
                       ("truth_at_0", T_sig, F_sig),
                       ("truth_one_bin_up", T_sig, F_sig + 1),
                       ("far_before_the_frame", 2 * -200, 40),           # every window before sample 0: all powers +0
                       ("far_behind_the_frame", 2 * 300, 40)):
        put(0, i, name, T, F)
        i += 1
    put_raw(0, i, "field_extremes", 32767, 255, -32768, 255)
    i += 1
    while i < 50:
        a = rng.integers(0, 256, 12, dtype=np.uint8)
        put(0, i, f"random_{i}", int(rng.integers(-24, 48)), int(rng.integers(0, 498)), a)
        i += 1
    for k in range(3):
        put(2, k, f"zeros_{k}", (T_sig, -24, 47)[k], (F_sig, 0, 497)[k])
    return iq, msgs, np.array([50, 0, 3], np.int32), where
