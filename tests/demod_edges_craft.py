"""Constructed signals for the branches and float edges of the second demodulation that radio frames never reach (tests only;
tests/test_demod_cpu.py proves with the restatement that every named case is what it is named for, tests/test_gpu_demod.py
holds the device to the restatement on them).  Everything is built from tests/demod_craft.py's float64 synthesiser and the
codeword of any 91 bits (tests/combine_craft.codeword_of_bits):

  refusals     noiseless signals whose word BP finds and the CRC (result 3) or unpack77 (result 4) refuses, the all-zero word,
               and a good signal behind the first refusal (a record composed and abandoned, then one composed and kept)
  weak         signals in noise on which set 1 finds no codeword and set 2 (or only set 3) is accepted
  tiny         one data symbol's 512 samples scaled down until set 1's smallest nonzero normalised soft bit lies below, or just
               above, the 2^-58 of the division guard
  scaled       one clean signal with every sample times a power of two: subnormal powers, an overflowing variance,
               infinite and NaN powers
  nan          a NaN sample with a sign and a payload inside a Costas symbol; -inf beside +inf
  edges        records with extreme fields and records one step either side of "the search window touches the frame"
  long lists   70 and 7 candidates per frame: the selection kernel's second chunk and the ragged last workgroup

The only searched quantities are WEAK_SEED with WEAK, TINY_EXP and SCALED_EXP; each was chosen from what the restatement
returns on the CPU (the searches are described beside them), and the CPU test asserts what each one is chosen for."""
import numpy as np

import combine_craft as cc
import demod_craft as dc
import ft8_spec_demod as sdm
import ft8_spec_osd as so

NSAMPLES = dc.NSAMPLES
CAP = dc.CAP
DATA_SYMS = tuple(range(7, 36)) + tuple(range(43, 72))


def tones_of_codeword(cw):
    """the 79 tones of any 174-bit codeword: Costas at 0 / 36 / 72, data symbol i of half h from bits 87 h + 3 i .. + 2 (MSB
    first) through the Gray map"""
    cw = np.asarray(cw, np.uint8)
    assert cw.shape == (174,)
    tones = np.zeros(79, np.uint8)
    for first in (0, 36, 72):
        tones[first:first + 7] = sdm.COSTAS
    for m in DATA_SYMS:
        b = 3 * sdm.data_index(m)
        tones[m] = sdm.GRAY[4 * int(cw[b]) + 2 * int(cw[b + 1]) + int(cw[b + 2])]
    return tones


def word_with_crc(bits77, flip=None):
    """the codeword of 77 payload bits and their CRC, bit `flip` of the 14 CRC bits inverted"""
    bits77 = np.asarray(bits77, np.uint8)
    crc = so.crc14(bits77)
    crc_bits = np.array([(crc >> (13 - k)) & 1 for k in range(14)], np.uint8)
    if flip is not None:
        crc_bits[flip] ^= 1
    return cc.codeword_of_bits(np.concatenate([bits77, crc_bits]))


def refused_bits(oracle):
    """77 seeded payload bits with i3 = 3, a message type unpack77 refuses"""
    bits = np.random.default_rng(0x77).integers(0, 2, 77).astype(np.uint8)
    bits[74:77] = (0, 1, 1)
    packed = np.packbits(np.concatenate([bits, np.zeros(3, np.uint8)]))
    assert oracle.unpack77(packed.tobytes())[0] < 0
    return bits


def place_tones(frame, tones, to, ts, fo, fs, amp=1.0, e=0, d=0, dt=0, df=0.0, phase0=0.0):
    T, F = 2 * to + ts, 2 * fo + fs
    I, Q = dc.cpfsk(tones, 0.78125 * (4 * F + d) + df, dc.start_of(T, e, dt), amp, phase0)
    frame[0] += I
    frame[1] += Q


# ---- weak signals ---------------------------------------------------------------------------------------------------------------
# weak_frame(seed) plants WEAK_SIGNALS signals of amplitude 0.30 .. 0.45 in noise of sigma 3.  Seeds 0, 1, 2, ... were analysed
# with the restatement (the library's twiddles, 20 iterations); WEAK_SEED is the first whose frame holds both a signal on which
# sets 1 and 3 find no codeword and set 2 is accepted, and one on which sets 1 and 2 find none and set 3 is accepted.  Its
# other signals are attempted too: set 1 accepts some, one is accepted by set 2 and would be by set 3, the rest end in 7.
WEAK_SIGNALS = 10
WEAK_SEED = 10
WEAK = {"set2_accepts": (2, 21), "set3_accepts": (6, 23)}                    # name: (signal, nhard of the accepted set)


def weak_frame(oracle, seed):
    """(frame float64 [2][48000], [(to, ts, fo, fs)] of its signals)"""
    rng = np.random.default_rng(seed)
    frame = rng.normal(0.0, 3.0, (2, NSAMPLES))
    at = []
    for s in range(WEAK_SIGNALS):
        to, ts, fo, fs = int(rng.integers(2, 10)), int(rng.integers(0, 2)), 10 + 24 * s, int(rng.integers(0, 2))
        dc.place(oracle, frame, dc.TEXTS[s % len(dc.TEXTS)], to, ts, fo, fs, amp=rng.uniform(0.30, 0.45), dt=int(rng.integers(-100, 101)),
                 df=rng.uniform(-1.2, 1.2), phase0=rng.uniform(0.0, 2.0 * np.pi))
        at.append((to, ts, fo, fs))
    return frame, at


# ---- one symbol scaled down -----------------------------------------------------------------------------------------------------
# A noiseless signal on the candidate's own grid point (e* = d* = 0), the 512 samples of data symbol TINY_SYMBOL times 2^k.  k
# was walked down from -50 with the restatement: at -60 set 1's smallest nonzero |x| is still above 2^-58, at -61 it is below,
# at -83 it is nonzero for the last time (from -84 on the symbol's soft bits are exact zeros, as sets 2 and 3 have them always).
# A magnitude whose square underflows is a zero, so the smallest soft bit follows the frame's scale: with every other sample
# times 2^40 or 2^48 (the norm factor shrinks by as much) the symbol at 2^-60 gives an |x| below the 2^-82 of the fast tanh's
# domain, and at 2^-83, the last nonzero one again, a subnormal |x|.
TINY_SYMBOL = 20
TINY_AT = (6, 0, 100, 1)                     # time_offset, time_sub, freq_offset, freq_sub
TINY_EXP = {"soft_bits_just_above": (-60, 0), "tiny_soft_bits": (-61, 0), "tiny_soft_bits_deepest": (-83, 0),
            "tiny_soft_bits_below_tanh_domain": (-60, 40), "subnormal_soft_bit": (-83, 48)}   # name: (k, the other samples' exponent)


def tiny_frame(oracle, k, rest=0):
    frame = np.zeros((2, NSAMPLES))
    to, ts, fo, fs = TINY_AT
    dc.place(oracle, frame, dc.TEXTS[2], to, ts, fo, fs, phase0=0.4)
    f32 = frame.astype(np.float32)
    s0 = dc.start_of(2 * to + ts) + 512 * TINY_SYMBOL
    exps = np.full(NSAMPLES, rest)
    exps[s0:s0 + 512] = k
    return np.ldexp(f32, exps[None, :]).astype(np.float32)


# ---- every sample times a power of two ------------------------------------------------------------------------------------------
# One signal of amplitude 1 in noise of sigma 0.5, as float32, times 2^k (ldexp: exact wherever the product is a normal float).
# k was walked over -91 .. -60 and 30 .. 127 with the restatement.  Downwards: -70 is the last k that is accepted, -75 the first
# with a subnormal psync, -83 the last with a nonzero one.  Upwards: 50 is the last k that is accepted, at 51 the squared sum
# of the soft bits overflows (variance -inf, norm factor -0, every x a zero: BP finds nothing), at 52 the sum of squares does
# too (inf - inf: a NaN variance), at 53 the powers from e = -1 on are infinite, from 54 to 124 all are, from 125 on they are
# NaN though every sample is finite.
SCALED_AT = (5, 1, 120, 0)
SCALED_EXP = {"scaled_accepted_tiny_psync": -70, "scaled_subnormal_psync": -75, "scaled_last_nonzero_psync": -83, "scaled_accepted_top": 50,
              "scaled_variance_overflows": 51, "scaled_not_finite": 52, "scaled_inf_psync": 53, "scaled_nan_psync": 125}


def scaled_base(oracle):
    rng = np.random.default_rng(0x5CA1)
    frame = rng.normal(0.0, 0.5, (2, NSAMPLES))
    to, ts, fo, fs = SCALED_AT
    dc.place(oracle, frame, dc.TEXTS[1], to, ts, fo, fs, e=1, d=-1, dt=5, df=0.1, phase0=2.0)
    return frame.astype(np.float32)


def scaled_frame(base, k):
    with np.errstate(over="ignore"):
        return np.ldexp(base, k).astype(np.float32)


# ---- the inputs -----------------------------------------------------------------------------------------------------------------
NAN_AT = (4, 0, 80, 1)
NAN_BITS = 0xFFC00001                        # a quiet NaN with its sign set and a payload
EXTREMES = ((20, 32767, -32768, 255, 255), (20, -32768, 32767, 255, 255), (-32768, -32768, -32768, 0, 0), (32767, 32767, 32767, 255, 255))
EDGE_T = (-160, -159, 186, 187)              # T = -159 and 186: the first and the last whose search window reaches the frame


def constructed(ft8, oracle):
    """iq float32 [B][2][48000], cands [B][CAP], counts [B], status_in [B][CAP], where {name: (frame, index)} and
    where["nhard"] = {name: nhard of the accepted set} for the weak signals.  Every record below a count qualifies but one."""
    frames, lists, where = [], [], {}

    def frame(iq32, recs):
        """recs: [(name or None, (score, to, fo, ts, fs))]"""
        f = len(frames)
        frames.append(np.asarray(iq32, np.float32))
        lists.append([r for _n, r in recs])
        for i, (name, _r) in enumerate(recs):
            if name is not None:
                assert name not in where
                where[name] = (f, i)
        return f

    def rec(to, ts, fo, fs, score=20):
        return (score, to, fo, ts, fs)

    # refusals: noiseless, 40 tone spacings apart
    rng = np.random.default_rng(0xE6)
    bits = rng.integers(0, 2, 77).astype(np.uint8)
    x = np.zeros((2, NSAMPLES))
    place_tones(x, tones_of_codeword(word_with_crc(bits, flip=5)), 4, 0, 20, 0, phase0=0.3)
    dc.place(oracle, x, dc.TEXTS[1], 5, 1, 60, 1, phase0=1.0)
    place_tones(x, tones_of_codeword(word_with_crc(refused_bits(oracle))), 6, 0, 100, 0, phase0=1.7)
    place_tones(x, np.asarray(tones_of_codeword(np.zeros(174, np.uint8))), 7, 1, 140, 1, phase0=2.4)
    place_tones(x, tones_of_codeword(word_with_crc(bits[::-1], flip=13)), 3, 1, 180, 0, phase0=3.1)
    frame(x, [("crc_refuses", rec(4, 0, 20, 0)), ("good_behind_a_refusal", rec(5, 1, 60, 1)), ("unpack_refuses", rec(6, 0, 100, 0)),
              ("all_zero_word", rec(7, 1, 140, 1)), ("crc_refuses_last", rec(3, 1, 180, 0))])

    # weak signals: the whole list of each seed's frame is attempted
    where["nhard"] = dict((name, nhard) for name, (_signal, nhard) in WEAK.items())
    x, at = weak_frame(oracle, WEAK_SEED)
    names = dict((signal, name) for name, (signal, _nhard) in WEAK.items())
    frame(x, [(names.get(s, f"weak_{s}"), rec(to, ts, fo, fs, score=30 - s)) for s, (to, ts, fo, fs) in enumerate(at)])

    # one symbol scaled down
    for name, (k, rest) in TINY_EXP.items():
        to, ts, fo, fs = TINY_AT
        frame(tiny_frame(oracle, k, rest), [(name, rec(to, ts, fo, fs))])

    # every sample times a power of two
    base = scaled_base(oracle)
    for name, k in SCALED_EXP.items():
        to, ts, fo, fs = SCALED_AT
        frame(scaled_frame(base, k), [(name, rec(to, ts, fo, fs))])

    # a NaN with a sign and a payload inside the first Costas symbol of a good signal; -inf beside +inf inside the last
    to, ts, fo, fs = NAN_AT
    for name, sym in (("nan_payload", 3), ("inf_beside_minus_inf", 75)):
        x = np.zeros((2, NSAMPLES))
        dc.place(oracle, x, dc.TEXTS[4], to, ts, fo, fs, phase0=0.9)
        x = x.astype(np.float32)
        j = dc.start_of(2 * to + ts) + 512 * sym + 200
        if name == "nan_payload":
            x[1, j:j + 1] = np.array([NAN_BITS], np.uint32).view(np.float32)
        else:
            x[0, j], x[0, j + 1] = -np.inf, np.inf
        frame(x, [(name, rec(to, ts, fo, fs))])

    # extreme fields and the frame's edges, on noise; the one record of these inputs that does not qualify
    x = np.random.default_rng(0xED6E).normal(0.0, 3.0, (2, NSAMPLES))
    recs = [(f"field_extremes_{k}", r) for k, r in enumerate(EXTREMES)]
    for T in EDGE_T:
        for fo in (0, 255):
            recs.append((f"edge_T{T}_fo{fo}", rec(T >> 1, T & 1, fo, 0)))
    recs.append(("does_not_qualify", rec(5, 0, 50, 0)))
    frame(x, recs)

    B = len(frames)
    iq = np.stack(frames)
    cands = np.zeros((B, CAP), ft8.CAND_DTYPE)
    counts = np.array([len(l) for l in lists], np.int32)
    status = np.stack([dc.failing_status(ft8, CAP) for _ in range(B)])
    for f, l in enumerate(lists):
        assert len(l) <= CAP
        for i, r in enumerate(l):
            cands[f, i] = r
    f, i = where["does_not_qualify"]
    status[f, i]["ok"], status[f, i]["ldpc_errors"] = 1, 0
    return iq, cands, counts, status, where


# ---- long lists -----------------------------------------------------------------------------------------------------------------
LONG = {70: (70, 65, 64, 3), 7: (7, 5)}      # max_candidates: the counts of its frames
LONG_RECORDS = ((20, 5, 100, 1, 0), (18, -80, 255, 1, 0), (16, 9, 37, 0, 1))


def long_lists(ft8, cap):
    """iq [B][2][48000] (even frames zeros, odd frames noise), cands [B][cap] drawn from LONG_RECORDS, counts LONG[cap], status
    [B][cap]: every third record does not qualify (ok = 1 and ldpc_errors = 0 in turn; one with ok = 1 and errors left), FILL
    behind the counts"""
    counts = np.array(LONG[cap], np.int32)
    B = len(counts)
    rng = np.random.default_rng(0x106 + cap)
    iq = np.zeros((B, 2, NSAMPLES), np.float32)
    iq[1::2] = rng.normal(0.0, 3.0, (len(iq[1::2]), 2, NSAMPLES)).astype(np.float32)
    cands = np.frombuffer(bytes([dc.FILL]) * (8 * B * cap), ft8.CAND_DTYPE).reshape(B, cap).copy()
    status = np.frombuffer(bytes([dc.FILL]) * (48 * B * cap), ft8.STATUS_DTYPE).reshape(B, cap).copy()
    pick = rng.integers(0, len(LONG_RECORDS), (B, cap))
    for f in range(B):
        status[f, :counts[f]] = dc.failing_status(ft8, int(counts[f]), errors=3 + f)
        for i in range(int(counts[f])):
            cands[f, i] = LONG_RECORDS[pick[f, i]]
            if i % 3 == 2:
                if i % 2:
                    status[f, i]["ok"], status[f, i]["ldpc_errors"] = 1, (7 if i == 5 else 0)
                else:
                    status[f, i]["ldpc_errors"] = 0
    return iq, cands, counts, status
