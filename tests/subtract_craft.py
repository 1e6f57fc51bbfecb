"""Frames and records for the tests of the subtraction in the I/Q samples (tests/test_subtract_cpu.py, tests/test_gpu_subtract.py)
and for tools/subtract_gain.py: single-signal frames with the synthesiser's own noiseless waveform beside them, the two-signal
frames of the uncovering test, and the hand-made records of the stage entry."""
import numpy as np

import ft8_spec_refine as sr
import ft8_spec_subtract as ss
import refine_craft as rc
import synth_util as su

NSAMPLES = 48000
FILL = 0xA5
STRONG_TEXT, WEAK_TEXT = "CQ K1ABC FN42", "CQ W9XYZ EN37"
# seeds of uncover_frame for which pass 1 decodes the strong signal only, the restated subtraction path decodes the weak one in
# pass 2 and ft8_spec_multipass.decode_passes at 2 passes does not (the first ten of the 53 such seeds among 0 .. 63)
UNCOVER_SEEDS = (0, 2, 3, 4, 5, 6, 7, 9, 10, 11)


def tones_of_text(oracle, text):
    rc_, payload = oracle.pack77(text)
    assert rc_ == 0
    return oracle.encode(payload), payload


# ---- suppression against the synthesiser's own waveform ---------------------------------------------------------------------

def suppression_frames(oracle, n, snr_db, seed):
    """n frames of one signal each from ft8o_synth_cpfsk, f0 and the start sample uniform and off the grid; snr_db None: no
    noise.  Returns (iq [n][2][48000], s [n][2][48000]: the noiseless waveform at the frame's scale, f0, start)."""
    rng = np.random.default_rng(seed)
    tones, _ = tones_of_text(oracle, STRONG_TEXT)
    f0 = rng.uniform(200.0, 1400.0, n)
    start = rng.integers(320, 5440, n)
    iq = np.zeros((n, 2, NSAMPLES), np.float32)
    s = np.zeros((n, 2, NSAMPLES), np.float32)
    for f in range(n):
        si, sq = oracle.synth_cpfsk(tones, [f0[f]], [start[f]], [1.0 if snr_db is None else su.amplitude_for_snr(snr_db, 1.0)])
        if snr_db is None:
            i32, q32 = si.copy(), sq.copy()
        else:
            i32 = (rng.normal(0.0, 1.0, NSAMPLES) + si).astype(np.float32)
            q32 = (rng.normal(0.0, 1.0, NSAMPLES) + sq).astype(np.float32)
        scale = np.float32(0.5) / max(np.abs(i32).max(), np.abs(q32).max())
        iq[f, 0], iq[f, 1] = i32 * scale, q32 * scale
        s[f, 0], s[f, 1] = si * scale, sq * scale
    return iq, s, f0, start


def suppression_db(oracle, iq, s, nthreads=8):
    """decode with the oracle, refine and subtract with the restatements; per decoded frame 10 log10(|x' - (x - s)|^2 / |s|^2),
    the residual of the cancellation against subtracting the truth.  Returns a float array (one entry per decoded frame)."""
    import ft8_spec_messages as sm
    mag, cands, counts, status = sm.oracle_stages(oracle, iq, nthreads=nthreads)
    msgs, n = sm.collect(mag, cands, counts, status)
    tw, w4 = sr.twiddles(oracle), ss.twiddles()
    out = []
    for f in range(len(n)):
        hit = [i for i in range(int(n[f])) if msgs[f, i]["text"].split(b"\0")[0].decode() == STRONG_TEXT]
        if not hit:
            continue
        i = hit[0]
        ref = np.zeros((1, 50), sr.REFINED_DTYPE)
        ref[0, i] = sr.refine_record(iq[f, 0], iq[f, 1], msgs[f, i]["cand"], msgs[f, i]["a91"].tobytes(), tw)
        x2, _info = ss.subtract(iq[f:f + 1], msgs[f:f + 1], ref, [i], [i + 1], w4)
        err = x2[0].astype(np.float64) - (iq[f].astype(np.float64) - s[f].astype(np.float64))
        out.append(10.0 * np.log10((err ** 2).sum() / (s[f].astype(np.float64) ** 2).sum()))
    return np.array(out)


# ---- uncovering ----------------------------------------------------------------------------------------------------------------

def uncover_frame(oracle, seed):
    """a weak signal 3 to 9 Hz and 2 to 5 symbols away from one that is 15 to 20 dB stronger, in unit noise -> float32 [2][48000]"""
    rng = np.random.default_rng(seed)
    strong, _ = tones_of_text(oracle, STRONG_TEXT)
    weak, _ = tones_of_text(oracle, WEAK_TEXT)
    snr_s = rng.uniform(0.0, 6.0)
    snr_w = snr_s - rng.uniform(15.0, 20.0)
    f_s = rng.uniform(300.0, 1300.0)
    f_w = f_s + rng.choice([-1.0, 1.0]) * rng.uniform(3.0, 9.0)
    st_s = int(rng.integers(1600, 4000))
    st_w = st_s + int(rng.choice([-1, 1])) * int(rng.integers(2 * 512, 5 * 512))
    si, sq = oracle.synth_cpfsk(np.stack([strong, weak]), [f_s, f_w], [st_s, st_w],
                                [su.amplitude_for_snr(snr_s, 1.0), su.amplitude_for_snr(snr_w, 1.0)])
    i32 = (rng.normal(0.0, 1.0, NSAMPLES) + si).astype(np.float32)
    q32 = (rng.normal(0.0, 1.0, NSAMPLES) + sq).astype(np.float32)
    return np.stack(oracle.normalise(i32, q32)).astype(np.float32)


def texts_of(msgs, n):
    return [[r["text"].split(b"\0")[0].decode(errors="replace") for r in msgs[f, :int(n[f])]] for f in range(len(n))]


def uncover_facts(oracle, iq, nthreads=8):
    """per frame (pass 1 decodes the strong signal only, the subtraction path has the weak one after pass 2, masking at 2 passes
    has not), and the subtraction path's (msgs, n, n_by_pass, residual)"""
    import ft8_spec_messages as sm
    import ft8_spec_multipass as mp
    stages = sm.oracle_stages(oracle, iq, nthreads=nthreads)
    sub = ss.decode_passes_subtracted(oracle, iq, 2, nthreads=nthreads, stages=stages)
    msk = mp.decode_passes(oracle, iq, 2, nthreads=nthreads, stages=stages)
    t_sub, t_msk = texts_of(sub[0], sub[1]), texts_of(msk[0], msk[1])
    facts = []
    for f in range(iq.shape[0]):
        first = t_sub[f][:int(sub[2][f, 0])]
        facts.append((first == [STRONG_TEXT], WEAK_TEXT in t_sub[f], WEAK_TEXT not in t_msk[f]))
    return facts, sub


# ---- hand-made records for the stage entry ---------------------------------------------------------------------------------------

def constructed(ft8):
    """6 frames of 50 records each, made by hand (a record need not be a decode), with first / n_msgs as the entry gets them:
      frame 0  noise and one strong signal that starts at sample 2576 on 4 * 321 + 2 quarter steps (1004.6875 Hz);
               first = -3, n_msgs = 70 (clamped to 0 and 50): windows that leave the frame at both ends (time_offset -12 and 23,
               freq_offset 0 and 248, every sub-step, e_best -16 / 0 / 16, u* 1 / 2 / 3), the signal's own record placed so that
               each of d* = +-2 and t* = +-2 is chosen, windows wholly outside the frame, R.valid = 0, random a91 and R
      frame 1  noise and the signal, n_msgs = 0
      frame 2  all zeros, n_msgs = 3
      frame 3  the signal, first = 2, n_msgs = 5: records 0 and 1 are not subtracted
      frame 4  the signal, first = 7 >= n_msgs = 4: nothing is subtracted
      frame 5  the signal, n_msgs = 3: three different records that overlap on the same samples (frames 3 to 5 hold the same five:
               the signal's own, another message in its cell, the signal's three steps up, and its own twice more)
    Returns (iq [6][2][48000], msgs [6][50], refined [6][50], first [6], n_msgs [6], where: name -> (frame, slot))."""
    rng = np.random.default_rng(20261020)
    payload = ft8.pack77(STRONG_TEXT)
    tones = ft8.encode(payload)
    a91 = np.frombuffer(rc.a91_of_payload(payload), np.uint8)
    T_sig, F_sig = 9, 2 * 160 + 1
    start, f0 = 256 * T_sig + sr.LEAD + 16, 0.78125 * (4 * F_sig + 2)
    B = 6
    iq = np.zeros((B, 2, NSAMPLES), np.float32)
    for f in (0, 1, 3, 4, 5):
        iq[f] = rc.noisy_frame(rng, tones, f0, start, 3.0)
    msgs = np.zeros((B, 50), ft8.MESSAGE_DTYPE)
    msgs.view(np.uint8)[:] = rng.integers(0, 256, msgs.nbytes, dtype=np.uint8).reshape(msgs.view(np.uint8).shape)
    refined = np.zeros((B, 50), sr.REFINED_DTYPE)
    refined.view(np.uint8)[:] = rng.integers(0, 256, refined.nbytes, dtype=np.uint8).reshape(refined.view(np.uint8).shape)
    where = {}
    PF = {1: (1.0, 9.0, 5.0, 2.0, 1.0), 2: (1.0, 5.0, 9.0, 5.0, 1.0), 3: (1.0, 2.0, 5.0, 9.0, 1.0)}

    def put(f, i, name, T, F, e_best=0, us=2, valid=1, a=a91):
        c = msgs[f, i]["cand"]
        c["score"], c["time_offset"], c["time_sub"], c["freq_offset"], c["freq_sub"] = 20, T >> 1, T & 1, F >> 1, F & 1
        msgs[f, i]["a91"] = a
        r = refined[f, i]
        r["e_best"], r["valid"], r["pf"] = e_best, valid, PF[us]
        where[name] = (f, i)

    i = 0
    for to in (-12, 23):
        for fo in (0, 248):
            for ts in (0, 1):
                for fs in (0, 1):
                    put(0, i, f"edge_to{to}_fo{fo}_ts{ts}_fs{fs}", 2 * to + ts, 2 * fo + fs, e_best=(-16, 0, 16)[i % 3], us=1 + i % 3)
                    i += 1
    # S_0 = 256 T + 256 + 32 e_best: 16 samples before the signal at e_best = 0, 16 behind it at e_best = 1;
    # k4_0 = 4 (F + u* - 2): 2 quarter steps below the signal at F + u* - 2 = 321, 2 above it at 322
    truth = (("truth_d+2_t+2", F_sig, 2, 0), ("truth_d-2_t-2", F_sig + 1, 2, 1), ("truth_d+2_t-2_u1", F_sig + 1, 1, 1),
             ("truth_d-2_t+2_u3", F_sig, 3, 0))
    for name, F, us, e in truth:
        put(0, i, name, T_sig, F, e_best=e, us=us)
        i += 1
    for name, T in (("far_before_the_frame", 2 * -200), ("far_behind_the_frame", 2 * 300)):
        put(0, i, name, T, 40)
        i += 1
    put(0, i, "not_valid", T_sig, F_sig, valid=0)
    i += 1
    put(0, i, "not_valid_random", 5, 77, valid=0, a=rng.integers(0, 256, 12, dtype=np.uint8))
    i += 1
    c = msgs[0, i]["cand"]
    c["time_offset"], c["time_sub"], c["freq_offset"], c["freq_sub"] = 32767, 255, -32768, 255
    refined[0, i]["e_best"], refined[0, i]["valid"] = 32767, 1
    where["field_extremes"] = (0, i)
    i += 1
    while i < 50:                                                 # random a91; every other one with a random R as well
        a = rng.integers(0, 256, 12, dtype=np.uint8)
        if i % 2:
            put(0, i, f"random_{i}", int(rng.integers(-24, 48)), int(rng.integers(0, 498)), e_best=int(rng.integers(-16, 17)),
                us=int(rng.integers(1, 4)), a=a)
        else:
            c = msgs[0, i]["cand"]
            c["time_offset"], c["time_sub"], c["freq_offset"], c["freq_sub"] = int(rng.integers(-12, 24)), 0, int(rng.integers(0, 249)), 1
            msgs[0, i]["a91"] = a
            refined[0, i]["e_best"] = int(rng.integers(-16, 17))
            where[f"random_R_{i}"] = (0, i)
        i += 1
    for k in range(3):
        put(2, k, f"zeros_{k}", (T_sig, -24, 47)[k], (F_sig, 0, 497)[k])
    other = rng.integers(0, 256, 12, dtype=np.uint8)                # another message in the signal's own cell
    for f in (3, 4, 5):
        put(f, 0, f"f{f}_truth", T_sig, F_sig, e_best=0, us=2)
        put(f, 1, f"f{f}_other_message_same_cell", T_sig, F_sig, e_best=0, us=2, a=other)
        put(f, 2, f"f{f}_three_steps_up", T_sig, F_sig + 3, e_best=1, us=2)
        put(f, 3, f"f{f}_truth_u3", T_sig, F_sig, e_best=0, us=3)
        put(f, 4, f"f{f}_truth_again", T_sig, F_sig, e_best=0, us=2)
    first = np.array([-3, 0, 0, 2, 7, 0], np.int32)
    n_msgs = np.array([70, 0, 3, 5, 4, 3], np.int32)
    return iq, msgs, refined, first, n_msgs, where
