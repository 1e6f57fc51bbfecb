"""Waterfalls, candidate lists and status records made to order for the second output path (tests only): the noise baseline
and message kernels of messages.hip, the mask and append kernels of multipass.hip, and dedup_dev.h / tone_dev.h behind them.
Radio frames never put the SNR decision near a threshold, never fill a noise window with one byte value, never carry a CRC
field that disagrees with its payload and never reach the seams of the dedup; here all of that is dictated.

numpy only, fixed seeds, everything in memory.  family(name) returns a dict {"name", "groups"}; a group is one Decoder
configuration (max_candidates = "cap", "min_score") with at most 16 frames over all groups of a family:
  mags [B][94208] uint8, cands [B][cap], counts [B], status [B][cap]     what collect_messages takes
  cases                                                                 one dict per constructed case (frame, index, ...)
  append = {base, msgs, n_msgs}                                         where the family has an append view of its own
  mask = {base, msgs, first, n_msgs}                                    mask_edges only
Status records are built like _synthetic_status of tests/test_gpu_messages.py, byte by byte so that junk behind a text's
NUL, 25-byte texts and the pad byte can be set.  Candidate slots at and behind counts[f] hold decoys: valid, decoded records
of unique messages with a high score, so that a kernel that ignored the count would write them.

How a case is laid out.  A case owns a SITE: slice fs (freq_sub mod 2) and the 40 columns [fo - 16, fo + 24) of it (fo the
clamped freq_offset), disjoint from every other site of its frame.  The 8 columns [fo, fo + 8) carry its cells, in the rows
of its time_sub; the other 32 (those inside the waterfall) are its noise window, and every window column is built over all
184 rows so that its 47th smallest byte -- what ft8gpu_collect_messages will compute as the baseline -- is the value the
case intends: 46 bytes at or below it, the value itself, 137 at or above it, shuffled.

Families (DESIGN.md "Every decoded message", "Multi-pass decoding"):
  snr_steps     for each of the 80 thresholds T[d] one case with S at or just above (nsym P[nb]) T[d] and one just below, the
                relative distance at most 2^-24 (half a float32 ulp) on each side, S being the sequential double sum of the
                rule.  The last four cells of a case are chosen by meet-in-the-middle over the pair sums of P, the others
                drawn near the target mean, with restarts.  nb is low for the high steps, high for the low ones (a high
                target mean is what makes the four-cell sums dense enough), symbol counts 79 and partial.  Step 0 (-30 dB)
                cannot be observed: snr_db starts there.  Reversing the order of the double sum changes none of these
                snr_db values: the summation ORDER in double is not observable through this family, only the precision.
  snr_range     49 and -30 by a wide margin, cells equal to the baseline, one symbol inside the waterfall (time_offset -78,
                91), none (-79, 92, -32768, 32767: 0 >= 0 holds at every step, so snr_db is 49 -- and the only cases here
                that sit exactly on equality).
  noise_window  every window size 16..32 (freq_offset 0..16 and 232..248), clamping freq_offsets (cells from the clamped
                value, freq_hz from the raw one), two-valued windows whose lower median, upper median and mean give three
                different snr_db, windows of all 0 and all 255 half outside the waterfall, sub-steps 2, 3, 254, 255; it
                carries a foreign base for the append.
  tones         91-bit a91 values (zero, ones, random, a walking one, CRC fields that do not match the payload, junk in the
                low five bits of a91[11]) painted inversely: the cell under the right tone low, the other seven at 255.
  dedup         caps 1, 63, 64, 65, 120, 129; the 50th and 51st unique message on either side of the chunk seam; texts and
                hashes at their edges; first occurrences that do not count; counts of -1 and cap + 5; and an append view.
  mask_edges    waterfall bytes in [0, 127], base in [128, 255]: every masked cell is visible.

variant=... of the functions below restates the rule WRONG in one named way; tests/test_messages_craft_cpu.py shows that every
variant changes at least one record or cell of the family built against it, and that variant=None is tests/ft8_spec_messages.py
and tests/ft8_spec_multipass.py byte for byte."""
import functools

import numpy as np

import ft8_spec_messages as sm
import ft8_spec_osd as so

COSTAS = (3, 1, 4, 0, 6, 5, 2)
GRAY = (0, 1, 3, 2, 5, 6, 4, 7)
GRAY_SWAPPED = (0, 1, 2, 3, 5, 6, 4, 7)                       # entries 2 and 3 exchanged
NBLOCKS, NBIN, MAG_ARRAY, MAX_MESSAGES = 92, 256, 94208, 50
FILL = 0xA5
FAMILIES = ("snr_steps", "snr_range", "noise_window", "tones", "dedup", "mask_edges")
VARIANTS = ("float32", "gt", "upper_median", "sentinel_high", "sentinel_zero", "unclamped", "subs_raw", "payload_tones",
            "gray_swap")
STEP_BOUND = 2.0 ** -24
CLAMPING_FO = (-1, -300, 249, 256, 1000, -32768, 32767)
SUBS = (2, 3, 254, 255)


def _ft8():
    import rtlsdr_ft8d_amd as ft8
    return ft8


# ---- a91 and tones ---------------------------------------------------------------------------------------------------------

def a91_from_bits(bits91):
    b = np.zeros(96, np.uint8)
    b[:91] = np.asarray(bits91, np.uint8)[:91]
    return np.packbits(b)


def bits_of(a91):
    return np.unpackbits(np.frombuffer(bytes(a91)[:12], np.uint8))[:91]


def a91_consistent(bits77):
    """payload + the CRC-14 ft8_encode appends to it"""
    crc = so.crc14(list(bits77))
    return a91_from_bits(list(bits77)[:77] + [(crc >> (13 - k)) & 1 for k in range(14)])


def tones_of(a91, variant=None):
    """the 79 tones of a91: all 91 stored bits through the generator, the Gray map and the Costas arrays"""
    bits = bits_of(a91).astype(np.int64)
    if variant == "payload_tones":                              # what ft8_encode gives for the payload alone
        bits = bits_of(a91_consistent(bits[:77])).astype(np.int64)
    gray = GRAY_SWAPPED if variant == "gray_swap" else GRAY
    cw = (bits @ so.generator_matrix().astype(np.int64)) & 1
    tones = np.zeros(79, np.int64)
    for m in range(79):
        if m < 7 or 36 <= m < 43 or m >= 72:
            tones[m] = COSTAS[m % 36]
        else:
            d = m - 7 if m < 36 else m - 14
            tones[m] = gray[int(cw[3 * d]) << 2 | int(cw[3 * d + 1]) << 1 | int(cw[3 * d + 2])]
    return tones


# ---- the rule, and its wrong variants ---------------------------------------------------------------------------------------

def _clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def window_columns(fo):
    """the noise window of clamped freq_offset fo: the columns inside the waterfall"""
    return [j for j in list(range(fo - 16, fo)) + list(range(fo + 8, fo + 24)) if 0 <= j < NBIN]


def nsym_of(to):
    return sum(1 for k in range(79) if 0 <= to + k < NBLOCKS)


def snr_of(mag, base, cand, a91, variant=None, parts=False):
    """snr_db of one message on frame mag [94208] with base [2][256]; variant None is ft8_spec_messages.snr_parts + snr_db"""
    P, T = sm.power_table(), sm.threshold_table()
    to, fo_raw = int(cand["time_offset"]), int(cand["freq_offset"])
    ts_raw, fs_raw = int(cand["time_sub"]), int(cand["freq_sub"])
    ts, fs = (ts_raw, fs_raw) if variant == "subs_raw" else (ts_raw & 1, fs_raw & 1)
    fo = fo_raw if variant == "unclamped" else _clamp(fo_raw, 0, 248)
    tones = tones_of(a91, variant)
    flat = np.asarray(mag, np.uint8).reshape(-1)
    f32 = variant == "float32"
    S = np.float32(0.0) if f32 else 0.0
    nsym = 0
    for k in range(79):
        blk = to + k
        if 0 <= blk < NBLOCKS:
            p = P[flat[(blk * 1024 + ts * 512 + fs * 256 + fo + int(tones[k])) % MAG_ARRAY]]
            S = S + np.float32(p) if f32 else S + float(p)
            nsym += 1
    brow = np.asarray(base, np.uint8).reshape(-1)
    cols = list(range(fo - 16, fo)) + list(range(fo + 8, fo + 24))
    inside = [int(brow[(fs * 256 + j) % 512]) for j in cols if 0 <= j < NBIN]
    outside = 32 - len(inside)
    if variant == "sentinel_high":
        v = sorted(inside + [256] * outside)
        nb = min(v[(len(v) - 1) // 2], 255)
    elif variant == "sentinel_zero":
        v = sorted(inside + [0] * outside)
        nb = v[(len(v) - 1) // 2]
    elif not inside:
        nb = 0
    elif variant == "upper_median":
        nb = sorted(inside)[len(inside) // 2]
    else:
        nb = sorted(inside)[(len(inside) - 1) // 2]
    if f32:
        floor_sum = np.float32(nsym) * np.float32(P[nb])
        thr = [floor_sum * np.float32(t) for t in T]
    else:
        floor_sum = float(nsym) * float(P[nb])
        thr = [floor_sum * float(t) for t in T]
    snr = sm.SNR_MIN
    for d in range(len(T)):
        if (S > thr[d]) if variant == "gt" else (S >= thr[d]):
            snr = sm.SNR_MIN + d
    return (snr, float(S), nsym, nb) if parts else snr


def collect(group, variant=None, base=None, msgs=None, n_msgs=None):
    """the records of a group under the rule (variant None) or one wrong variant of it; with msgs / n_msgs it is the append"""
    ft8 = _ft8()
    mags, cands, counts, status = group["mags"], group["cands"], group["counts"], group["status"]
    B, cap = cands.shape
    raw = status.view(np.uint8).reshape(B, cap, 48)
    if base is None:
        base = sm.noise_baseline(mags)
    base = np.asarray(base, np.uint8).reshape(B, 2, 256)
    out = np.full((B, MAX_MESSAGES * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(B, MAX_MESSAGES) if msgs is None else np.array(msgs, copy=True)
    n = np.zeros(B, np.int32)
    for f in range(B):
        n0 = 0 if n_msgs is None else _clamp(n_msgs[f], 0, MAX_MESSAGES)
        seen = [(int(out[f, r]["hash"]), sm._c_text(out[f, r].tobytes()[:25])) for r in range(n0)]
        for i in range(_clamp(counts[f], 0, cap)):
            c, r = cands[f, i], status[f, i]
            if int(c["score"]) < group["min_score"] or int(r["ok"]) == 0:
                continue
            text_raw = raw[f, i, 22:47].tobytes()
            key = (int(r["crc_extracted"]), sm._c_text(text_raw))
            if key in seen:
                continue
            seen.append(key)
            if len(seen) > MAX_MESSAGES:
                continue
            a91 = raw[f, i, 10:22].tobytes()
            rec = np.zeros(1, ft8.MESSAGE_DTYPE)
            rb = rec.view(np.uint8).reshape(64)
            rb[:25] = np.frombuffer(text_raw, np.uint8)
            rec = rec[0]
            rec["snr_db"] = snr_of(mags[f], base[f], c, a91, variant)
            rec["score"] = c["score"]
            rec["freq_hz"] = (np.float32(c["freq_offset"]) + np.float32(c["freq_sub"]) / np.float32(2)) * np.float32(6.25)
            rec["dt_s"] = (np.float32(c["time_offset"]) + np.float32(c["time_sub"]) / np.float32(2)) / np.float32(6.25)
            rec["hash"] = r["crc_extracted"]
            rec["cand_index"] = i
            rec["cand"] = c
            rec["a91"] = np.frombuffer(a91, np.uint8)
            out[f, len(seen) - 1] = rec
        n[f] = min(len(seen), MAX_MESSAGES)
    return out, n


def mask_cells(msgs, first, n_msgs, variant=None):
    """the cells the mask rule writes, per frame a sorted list of flat indices into the frame's waterfall.
    variant "no_block_test" drops the test 0 <= time_offset + k < 92 (the index then wraps inside the frame)"""
    out = []
    for f in range(len(first)):
        cells = set()
        for r in range(_clamp(first[f], 0, MAX_MESSAGES), _clamp(n_msgs[f], 0, MAX_MESSAGES)):
            c = msgs[f, r]["cand"]
            to = int(c["time_offset"])
            ts, fs = int(c["time_sub"]), int(c["freq_sub"])
            if variant != "subs_raw":
                ts, fs = ts & 1, fs & 1
            fo = int(c["freq_offset"]) if variant == "unclamped" else _clamp(c["freq_offset"], 0, 248)
            tones = tones_of(msgs[f, r]["a91"], variant)
            for k in range(79):
                if variant == "no_block_test" or 0 <= to + k < NBLOCKS:
                    cells.add(((to + k) * 1024 + ts * 512 + fs * 256 + fo + int(tones[k])) % MAG_ARRAY)
        out.append(sorted(cells))
    return out


# ---- building blocks ---------------------------------------------------------------------------------------------------------

def status_record(text=b"", hash_=0, ok=1, a91=None, pad=0, calculated=None):
    """48 bytes: ldpc_errors, iters, crc_extracted, crc_calculated, unpack_status, ok, a91[12], text[25], pad"""
    raw = np.zeros(48, np.uint8)
    raw[4:6] = np.frombuffer(np.uint16(hash_).tobytes(), np.uint8)
    raw[6:8] = np.frombuffer(np.uint16(hash_ if calculated is None else calculated).tobytes(), np.uint8)
    raw[9] = ok
    if a91 is not None:
        raw[10:22] = np.frombuffer(bytes(a91)[:12], np.uint8)
    t = bytes(text)[:25]
    raw[22:22 + len(t)] = np.frombuffer(t, np.uint8)
    raw[47] = pad
    return raw


def _set_baseline(mag4, fs, j, v, rng):
    """column (fs, j) of mag4 [92][2][2][256] over its 184 rows: the 47th smallest byte becomes v"""
    col = np.concatenate([rng.integers(0, v + 1, 46), [v], rng.integers(v, 256, 137)]).astype(np.uint8)
    rng.shuffle(col)
    mag4[:, :, fs, j] = col.reshape(NBLOCKS, 2)


class _Book:
    """frames under construction: sites are placed in the first frame that has room for them"""

    def __init__(self, seed, lo=0, hi=256, per_frame=48):
        self.rng = np.random.default_rng(seed)
        self.lo, self.hi, self.per_frame = lo, hi, per_frame
        self.frames = []

    def _new(self):
        self.frames.append(dict(mag=self.rng.integers(self.lo, self.hi, (NBLOCKS, 2, 2, NBIN)).astype(np.uint8),
                                used={0: [], 1: []}, cands=[], status=[], cases=[]))

    def place(self, fs, fo):
        span = (max(fo - 16, 0), min(fo + 24, NBIN))
        for k in range(len(self.frames) + 1):
            if k == len(self.frames):
                self._new()
            fr = self.frames[k]
            if len(fr["cands"]) < self.per_frame and all(span[1] <= a or b <= span[0] for a, b in fr["used"][fs]):
                fr["used"][fs].append(span)
                return k, fr

    def site(self, cand, a91, cells, window, other=None, text=None, hash_=None, **info):
        """one case.  cand = (score, time_offset, freq_offset, time_sub, freq_sub); cells: a byte or one byte per symbol inside
        the waterfall, in symbol order; window: a byte or one byte per window column, in column order; other: the byte of
        the seven cells beside each tone (None: the background stays)"""
        score, to, fo_raw, ts_raw, fs_raw = cand
        fo, ts, fs = _clamp(fo_raw, 0, 248), ts_raw & 1, fs_raw & 1
        k, fr = self.place(fs, fo)
        cols = window_columns(fo)
        wv = [int(window)] * len(cols) if np.isscalar(window) else [int(x) for x in window]
        assert len(wv) == len(cols)
        for j, v in zip(cols, wv):
            _set_baseline(fr["mag"], fs, j, v, self.rng)
        tones = tones_of(a91)
        inside = [m for m in range(79) if 0 <= to + m < NBLOCKS]
        cv = [int(cells)] * len(inside) if np.isscalar(cells) else [int(x) for x in cells]
        assert len(cv) == len(inside)
        for m, v in zip(inside, cv):
            if other is not None:
                fr["mag"][to + m, ts, fs, fo:fo + 8] = other
            fr["mag"][to + m, ts, fs, fo + int(tones[m])] = v
        idx = len(fr["cands"])
        text = (b"%s%02d.%03d" % (info.get("tag", b"C"), k, idx)) if text is None else text
        hash_ = sm.crc_in_a91(a91) if hash_ is None else hash_
        fr["cands"].append((score, to, fo_raw, ts_raw, fs_raw))
        fr["status"].append(status_record(text, hash_, 1, a91))
        case = dict(info, frame=k, index=idx, window_size=len(cols), nsym=len(inside))
        fr["cases"].append(case)
        return case

    def group(self, cap=120, min_score=10):
        return _pack([(fr["mag"], fr["cands"], fr["status"], None) for fr in self.frames], cap, min_score,
                     [c for fr in self.frames for c in fr["cases"]], self.rng)


def _pack(frames, cap, min_score, cases, rng):
    """frames: (mag4 or flat, cand tuples, status rows, count or None) -> a group; slots behind the count hold decoys"""
    ft8 = _ft8()
    B = len(frames)
    mags = np.stack([np.asarray(fr[0], np.uint8).reshape(MAG_ARRAY) for fr in frames])
    cands = np.zeros((B, cap), ft8.CAND_DTYPE)
    status = np.zeros((B, cap, 48), np.uint8)
    counts = np.zeros(B, np.int32)
    for f, (_, cl, sl, count) in enumerate(frames):
        assert len(cl) == len(sl) <= cap
        for i in range(cap):
            if i < len(cl):
                cands[f, i], status[f, i] = tuple(cl[i]), sl[i]
            else:
                a = a91_from_bits(rng.integers(0, 2, 91))
                cands[f, i] = (300, int(rng.integers(-12, 24)), int(rng.integers(0, 249)), int(rng.integers(0, 2)), int(rng.integers(0, 2)))
                status[f, i] = status_record(b"DECOY %d" % i, 0x3000 + i, 1, a)
        counts[f] = len(cl) if count is None else count
    return dict(cap=cap, min_score=min_score, mags=mags, cands=cands, counts=counts,
                status=status.view(ft8.STATUS_DTYPE).reshape(B, cap), cases=cases)


def _random_payload(rng):
    return a91_consistent(rng.integers(0, 2, 77))


# ---- snr_steps -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def _pair_sums():
    P = sm.power_table()
    i, j = np.triu_indices(256)
    s = P[i] + P[j]
    o = np.argsort(s, kind="stable")
    return s[o], i[o], j[o]


def _seq_sum(P, cells):
    S = 0.0
    for v in cells:
        S = S + float(P[v])
    return S


def _step_cells(rng, nsym, nb, d, restarts=48, at_least=8):
    """cells (bytes, symbol order) for a case at or above and one below threshold d: ((cells, gap) above, (cells, gap) below),
    gap = |S - X| / X with X = (nsym P[nb]) T[d]; at least `at_least` restarts, then until both gaps are within STEP_BOUND"""
    P, T = sm.power_table(), sm.threshold_table()
    X = (float(nsym) * float(P[nb])) * float(T[d])
    mean = nb + 20.0 * np.log10(float(T[d]))
    ps, pi, pj = _pair_sums()
    best = {True: None, False: None}
    for turn in range(restarts):
        head = [int(v) for v in np.clip(np.rint(mean) + rng.integers(-6, 5, nsym - 4), 0, 255)]
        partial = _seq_sum(P, head)
        R = X - partial
        if R <= 4.0 * float(P[0]) or R > 3.5 * float(P[255]):
            continue
        k = np.searchsorted(ps, R - ps)
        tried = []
        for kk in (np.clip(k, 0, len(ps) - 1), np.clip(k - 1, 0, len(ps) - 1)):
            err = ps + ps[kk] - R
            tried += [(int(a), int(kk[a])) for a in np.argsort(np.abs(err))[:12]]
        for a, b in tried:
            tail = sorted([int(pi[a]), int(pj[a]), int(pi[b]), int(pj[b])])
            cells = head + tail
            S = _seq_sum(P, cells)
            above = S >= X
            gap = abs(S - X) / X
            if best[above] is None or gap < best[above][1]:
                best[above] = (cells, gap)
        if turn + 1 >= at_least and all(best[s] is not None and best[s][1] <= STEP_BOUND for s in (True, False)):
            break
    return best[True], best[False]


def _step_plan(d):
    """(nb, time_offset) of step d: nb low / middle / high as far as the target mean byte stays in [170, 246], where the
    four-cell sums are dense enough for the 2^-24 bound; full and partial symbol counts in turn"""
    lift = 20.0 * np.log10(float(sm.threshold_table()[d]))
    order = [(30, 90, 150, 210), (90, 150, 210, 30), (150, 210, 30, 90), (210, 30, 90, 150)][d % 4]
    ok = [nb for nb in order if 170.0 <= nb + lift <= 246.0]
    nb = ok[0] if ok else _clamp(round(208.0 - lift), 0, 255)
    to = (0, 13, -12, 23, 5, -40, 60, 2)[d % 8]
    return nb, to


def _snr_steps():
    book = _Book(0x5731, lo=0, hi=96)
    rng = np.random.default_rng(0x5732)
    fo_slots = [16 + 40 * i for i in range(6)]
    n = 0
    for d in range(80):
        nb, to = _step_plan(d)
        nsym = nsym_of(to)
        above, below = _step_cells(rng, nsym, nb, d)
        for side, (cells, gap) in (("above", above), ("below", below)):
            fo, fs, ts = fo_slots[n % 6] + (n // 12) % 17, (n // 6) & 1, int(rng.integers(0, 2))
            book.site((20 + d, to, fo, ts, fs), _random_payload(rng), cells, nb, step=d, side=side, gap=gap, nb=nb,
                      want=sm.SNR_MIN + (d if side == "above" else max(d - 1, 0)), tag=b"S")
            n += 1
    return [book.group()]


# ---- snr_range -------------------------------------------------------------------------------------------------------------

def _snr_range():
    book = _Book(0x5241, lo=0, hi=256)
    rng = book.rng
    pl = lambda: _random_payload(rng)
    k = 0

    def add(to, cells, window, want, **kw):
        nonlocal k
        book.site((30, to, 20 + 40 * (k % 6), k & 1, (k // 6) & 1), pl(), cells, window, want=want, tag=b"R", **kw)
        k += 1
    for to in (0, -12, 23):
        add(to, 255, 0, 49, kind="top")
        add(to, 0, 255, -30, kind="bottom")
        add(to, 100, 100, -30, kind="equal")
    add(5, 0, 0, -30, kind="equal")
    add(5, 255, 255, -30, kind="equal")
    for to in (-78, 91):
        add(to, 200, 100, None, kind="one_symbol")
        add(to, 255, 0, 49, kind="one_symbol")
        add(to, 0, 255, -30, kind="one_symbol")
    for to in (-79, 92, -32768, 32767):
        add(to, [], 100, 49, kind="no_symbol")
        add(to, [], 0, 49, kind="no_symbol")
    return [book.group()]


# ---- noise_window ----------------------------------------------------------------------------------------------------------

def _two_valued(n, lo, hi, rng):
    """n window bytes, (n + 1) // 2 of them lo and the rest hi, shuffled: lower median lo; for even n the upper median is hi"""
    w = np.array([lo] * ((n + 1) // 2) + [hi] * (n // 2))
    rng.shuffle(w)
    return w


def _noise_window():
    book = _Book(0x4E57, lo=0, hi=128)
    rng = book.rng
    pl = lambda: _random_payload(rng)
    k = 0

    def add(fo, window, cells=190, ts=None, fs=None, to=None, **kw):
        nonlocal k
        ts = k & 1 if ts is None else ts
        fs = (k >> 1) & 1 if fs is None else fs
        to = (0, -12, 13, 23, 7)[k % 5] if to is None else to
        n = len(window_columns(_clamp(fo, 0, 248)))
        w = window(n) if callable(window) else window
        book.site((25, to, fo, ts, fs), pl(), cells, w, tag=b"W", fo=fo, **kw)
        k += 1
    for fo in list(range(0, 17)) + list(range(232, 249)):                     # window sizes 16..32, both parities
        add(fo, lambda n: rng.integers(90, 150, n), kind="size")
    for fo in CLAMPING_FO:                                                      # cells from the clamped value
        add(fo, lambda n: rng.integers(90, 150, n), kind="clamp")
    for fo in (0, 5, 100, 133, 248):                                           # lower median / upper median / mean all differ
        add(fo, lambda n: _two_valued(n, 100, 140, rng), kind="two_valued")
    for fo in (0, 248):                                                        # half the window outside: never counted
        add(fo, 0, cells=120, kind="all_0")
        add(fo, 255, cells=255, kind="all_255")
    for ts, fs in ((2, 3), (3, 2), (254, 255), (255, 254), (2, 254), (3, 255), (255, 255), (2, 2)):
        add(60 + 8 * (k % 20), lambda n: rng.integers(90, 150, n), ts=ts, fs=fs, kind="subs")
    g = book.group()
    B = len(g["counts"])
    base = np.random.default_rng(0x4E58).integers(0, 256, (B, 2, 256)).astype(np.uint8)         # NOT the waterfall's own baseline
    ft8 = _ft8()
    g["append"] = dict(base=base, msgs=np.full((B, MAX_MESSAGES * 64), FILL, np.uint8).view(ft8.MESSAGE_DTYPE).reshape(B, MAX_MESSAGES),
                       n_msgs=np.zeros(B, np.int32))
    return [g]


# ---- tones -----------------------------------------------------------------------------------------------------------------

def tone_payloads(rng):
    """(kind, a91) of the tones family"""
    out = [("zero", a91_from_bits(np.zeros(91))), ("ones", a91_from_bits(np.ones(91)))]
    out += [("random", a91_from_bits(rng.integers(0, 2, 91))) for _ in range(4)]
    for b in range(91):
        bits = np.zeros(91, np.uint8)
        bits[b] = 1
        out.append(("walking", a91_from_bits(bits)))
    for _ in range(3):                                                        # a consistent record, then its CRC field damaged
        a = _random_payload(rng)
        bad = bits_of(a).copy()
        bad[77 + int(rng.integers(0, 14))] ^= 1
        out += [("crc_match", a), ("crc_mismatch", a91_from_bits(bad))]
    for junk in (0x1F, 0x01, 0x10):                                           # the low five bits are no part of the 91
        a = _random_payload(rng)
        j = a.copy()
        j[11] |= junk
        out += [("junk_clean", a), ("junk", j)]
    return out


def _tones():
    book = _Book(0x544F, lo=0, hi=128, per_frame=12)
    rng = book.rng
    for k, (kind, a91) in enumerate(tone_payloads(rng)):
        to = (0, 13, -12, 23, 4)[k % 5]
        book.site((40, to, 16 + 40 * (k % 6) + (k // 12) % 17, k & 1, (k // 6) & 1), a91, 140, 100, other=255,
                  kind=kind, tag=b"T", hash_=sm.crc_in_a91(a91))
    return [book.group()]


# ---- dedup -----------------------------------------------------------------------------------------------------------------

def _msg(j):
    """message j of the dedup pool: (text, hash, a91)"""
    rng = np.random.default_rng(0xDE00 + j)
    a = _random_payload(rng)
    return b"MSG %03d DE TEST" % j, sm.crc_in_a91(a), a


def _dedup_frame(rng, entries, count=None, lo=0, hi=256):
    """entries: dicts with j (pool message) or text / hash, and ok, score, pad"""
    mag = rng.integers(lo, hi, MAG_ARRAY).astype(np.uint8)
    cl, sl = [], []
    for e in entries:
        text, h, a = _msg(e.get("j", 0))
        text, h = e.get("text", text), e.get("hash", h)
        cl.append((e.get("score", 15), int(rng.integers(-12, 24)), int(rng.integers(0, 249)), int(rng.integers(0, 2)), int(rng.integers(0, 2))))
        sl.append(status_record(text, h, e.get("ok", 1), e.get("a91", a), e.get("pad", 0)))
    return mag, cl, sl, count


def _seam(n_at, total, extra_unique=True):
    """a candidate list whose 50th unique message sits at index n_at and whose 51st follows at n_at + 1; the n_at - 49 other
    places before it are repeats, undecoded candidates and candidates below min_score, spread between the first 49"""
    fillers = n_at - 49
    every = 49 // max(fillers, 1)
    e, j, placed = [], 0, 0
    while j < 49:
        e.append(dict(j=j))
        j += 1
        if placed < fillers and j % every == 0:
            e.append([dict(j=max(j - 3, 0)), dict(j=200 + placed, ok=0), dict(j=300 + placed, score=9)][placed % 3])
            placed += 1
    assert len(e) == n_at
    e.append(dict(j=49))
    if extra_unique:
        e.append(dict(j=50))
    k = 51
    while len(e) < total:
        e.append(dict(j=k if k % 2 else k - 40))
        k += 1
    return e[:total]


def _text_cases():
    t25a, t25b = b"ABCDEFGHIJKLMNOPQRSTUVWX1", b"ABCDEFGHIJKLMNOPQRSTUVWX2"
    return [dict(j=0), dict(j=0, text=b"OTHER TEXT"),                          # the same hash with another text: new
            dict(j=0, hash=0x1234),                                            # the same text with another hash: new
            dict(j=0),                                                         # a repeat
            dict(j=1, text=b"HELLO\0JUNK ONE"), dict(j=1, text=b"HELLO\0OTHER JUNK BEHIND"), dict(j=1, text=b"HELLO"),   # one message
            dict(j=2, text=t25a), dict(j=2, text=t25b), dict(j=2, text=t25a),   # 25 characters, no terminator: two messages
            dict(j=2, text=t25a[:24]),                                         # and the 24-character prefix: a third
            dict(j=3, pad=0xEE), dict(j=3, pad=0x01), dict(j=3),               # the pad byte is no part of the text: one message
            dict(j=4, text=b""), dict(j=4, text=b"\0BEHIND"), dict(j=4, text=b"", hash=0),   # empty text: two messages (two hashes)
            dict(j=5, hash=0x3FFF), dict(j=5, hash=0x4000), dict(j=5, hash=0xFFFF), dict(j=5, hash=0xFFFF),   # three messages
            dict(j=6, text=b"\xff\x80\x7f HIGH BYTES"), dict(j=6, text=b"\xff\x80\x7f HIGH BYTES"), dict(j=6, text=b"\xff\x80\x7e HIGH BYTES")]


def _first_cases():
    return [dict(j=0, score=9), dict(j=1, ok=0), dict(j=2),                    # firsts that do not count ...
            dict(j=0), dict(j=1), dict(j=2),                                   # ... the later occurrence is the first
            dict(j=3, ok=2), dict(j=4, ok=255), dict(j=3, ok=1),               # ok is tested for non-zero
            dict(j=5, score=10), dict(j=6, score=-5), dict(j=6, score=32767), dict(j=7, score=-32768)]


def _seed_records(rng, items):
    """hand-made records for the append: (text, hash) pairs, bytes behind the text's NUL filled with junk"""
    ft8 = _ft8()
    m = np.full(MAX_MESSAGES * 64, FILL, np.uint8)
    for r, (text, h) in enumerate(items):
        rec = rng.integers(1, 256, 64).astype(np.uint8)                        # junk everywhere first
        t = bytes(text)[:25]
        rec[:len(t)] = np.frombuffer(t, np.uint8)
        if len(t) < 25:
            rec[len(t)] = 0
        rec[36:38] = np.frombuffer(np.uint16(h).tobytes(), np.uint8)
        m[64 * r:64 * r + 64] = rec
    return m.view(ft8.MESSAGE_DTYPE)


def _dedup():
    rng = np.random.default_rng(0xDED0)
    groups = []

    def group(cap, frames, seeds, n_in):
        g = _pack(frames, cap, 10, [], rng)
        B = len(frames)
        g["append"] = dict(base=np.random.default_rng(cap).integers(0, 256, (B, 2, 256)).astype(np.uint8),
                           msgs=np.stack([_seed_records(rng, s) for s in seeds]), n_msgs=np.array(n_in, np.int32))
        groups.append(g)
    pool = lambda js: [_msg(j)[:2] for j in js]
    # cap 1: one decoded candidate under a count of cap + 5; a count of -1
    group(1, [_dedup_frame(rng, [dict(j=0)], count=6), _dedup_frame(rng, [dict(j=1)], count=-1)],
          [pool([0]), pool([])], [0, 0])
    # cap 63: the 50th unique message in the last lane the cap leaves; the text cases under a count of cap + 5
    group(63, [_dedup_frame(rng, _seam(62, 63)), _dedup_frame(rng, _text_cases() + _seam(49, 38)[:38], count=68)],
          [pool(range(100, 149)), pool([0, 1])], [49, -3])
    # cap 64: 50th at lane 62, 51st at lane 63; firsts that do not count
    group(64, [_dedup_frame(rng, _seam(62, 64)), _dedup_frame(rng, _first_cases())],
          [pool(range(0, 50)), pool([2, 5])], [50, 77])
    # cap 65: 50th at lane 63, 51st at lane 0 of the next chunk; a count of -1 with a full list
    group(65, [_dedup_frame(rng, _seam(63, 65)), _dedup_frame(rng, _seam(63, 65), count=-1)],
          [pool([10, 20]), pool([3])], [2, 1])
    # cap 120: 50th at lane 0 and 51st at lane 1 of the second chunk; text cases; 50 reached in the middle of the second
    # chunk; a message of the second chunk that repeats one of the first and one that repeats a seed record
    late = [dict(j=j % 20) for j in range(64)] + [dict(j=20 + j) for j in range(20)] + [dict(j=5), dict(j=70)]
    group(120, [_dedup_frame(rng, _seam(64, 120)), _dedup_frame(rng, _text_cases()),
                _dedup_frame(rng, [dict(j=j % 30) for j in range(70)] + [dict(j=30 + j) for j in range(40)]),
                _dedup_frame(rng, late)],
          [pool([]), [(b"HELLO\0SEED JUNK", _msg(1)[1]), (b"ABCDEFGHIJKLMNOPQRSTUVWX2", _msg(2)[1]), (b"", 0)],
           pool(range(200, 210)), pool([70, 21, 150])], [0, 3, 10, 3])
    # cap 129: three chunks, the last one a single lane that carries a new message; a count of cap + 5; more than 50
    sparse = [dict(j=j // 6) for j in range(128)] + [dict(j=99)]
    group(129, [_dedup_frame(rng, sparse), _dedup_frame(rng, sparse, count=134),
                _dedup_frame(rng, [dict(j=j) for j in range(129)]), _dedup_frame(rng, _first_cases() + _text_cases())],
          [pool([]), pool([99]), pool(range(100, 149)), pool([])], [0, 1, 49, 0])
    return groups


# ---- mask_edges ------------------------------------------------------------------------------------------------------------

MASK_TIME_OFFSETS = (-79, -78, -12, 0, 13, 14, 23, 91, 92)


def _mask_edges():
    rng = np.random.default_rng(0x3A5C)
    pay = [a for _, a in tone_payloads(np.random.default_rng(0x544F))]
    frames = []

    def frame(cl, a91s=None):
        a91s = [a91_from_bits(rng.integers(0, 2, 91)) for _ in cl] if a91s is None else a91s
        sl = [status_record(b"MASK %d" % i, 0x100 + i, 1, a) for i, a in enumerate(a91s)]
        frames.append((rng.integers(0, 128, MAG_ARRAY).astype(np.uint8), cl, sl, None))
    frame([(20, to, 30 * k, k & 1, (k >> 1) & 1) for k, to in enumerate(MASK_TIME_OFFSETS)])
    frame([(20, int(rng.integers(-12, 24)), fo, k & 1, (k >> 1) & 1) for k, fo in enumerate(CLAMPING_FO + (0, 248, 1, 247))]
          + [(20, 3, 100, ts, fs) for ts in SUBS for fs in SUBS])
    frame([(20, (0, -12, 23, -78, 91)[k % 5], int(rng.integers(0, 249)), k & 1, (k >> 1) & 1) for k in range(50)], pay[:50])
    frame([(20, int(rng.integers(-12, 24)), int(rng.integers(0, 249)), int(rng.integers(0, 2)), int(rng.integers(0, 2))) for _ in range(50)])
    twice = a91_from_bits(rng.integers(0, 2, 91))
    frame([(20, 1, 50, 0, 0), (21, 5, 120, 1, 0), (22, 5, 120, 3, 2), (23, 9, 200, 1, 1)], [pay[2], twice, twice, pay[3]])
    frame([(20, 2, 10 + 20 * k, 0, 1) for k in range(6)], pay[50:56])
    frame([(20, -5, 10 + 20 * k, 1, 0) for k in range(5)], pay[56:61])
    frame([(20, 17, 10 + 20 * k, 1, 1) for k in range(4)], pay[61:65])
    g = _pack(frames, 120, 10, [], rng)
    base = rng.integers(128, 256, (len(frames), 2, 256)).astype(np.uint8)
    msgs, n = collect(g, base=base)
    n = n.copy()
    assert list(n) == [9, 27, 50, 50, 4, 6, 5, 4]
    #                     0   1   2   3  4      5  6  7
    first = np.array([0, -4, 0, 0, 1, 8, 0, 4], np.int32)                     # -4: from 0; 1: record 0 stays; n + 2 and n: nothing
    n_mask = np.array([9, 27, 77, 50, 3, 6, 0, 4], np.int32)                   # 77: up to 50; 3 of 4: record 3 stays; 0: nothing
    g["mask"] = dict(base=base, msgs=msgs, first=first, n_msgs=n_mask)
    g["append"] = dict(base=base, msgs=msgs, n_msgs=np.array([4, 27, 10, 50, 0, 77, -3, 2], np.int32))
    return [g]


_BUILDERS = dict(snr_steps=_snr_steps, snr_range=_snr_range, noise_window=_noise_window, tones=_tones, dedup=_dedup,
                 mask_edges=_mask_edges)


@functools.lru_cache(None)
def family(name):
    groups = _BUILDERS[name]()
    assert sum(len(g["counts"]) for g in groups) <= 16, name
    for g in groups:
        for k in ("mags", "cands", "counts", "status"):
            g[k].setflags(write=False)
    return dict(name=name, groups=groups)


def report():
    """what the families reach and which wrong variant of the rule each of them catches, by the restatement alone
    (profiles/messages_constructed.json: python tests/messages_craft.py)"""
    def wrong(g, variant):
        a, n = collect(g)
        b, _ = collect(g, variant=variant)
        return [(f, j) for f in range(len(n)) for j in range(int(n[f])) if a[f, j].tobytes() != b[f, j].tobytes()]
    steps = family("snr_steps")["groups"][0]
    f32 = {(f, j) for f, j in wrong(steps, "float32")}
    by_place = {(c["frame"], c["index"]): c for c in steps["cases"]}
    doc = dict(what="constructed inputs of the messages, mask and append kernels (tests/messages_craft.py): what the families reach "
                    "and how many records or frames each wrong variant of the rule changes, by the numpy restatements; "
                    "tests/test_gpu_messages_constructed.py holds the device to the same records byte for byte",
               frames={name: [len(g["counts"]) for g in family(name)["groups"]] for name in FAMILIES},
               snr_steps=dict(cases=len(steps["cases"]), bound=STEP_BOUND,
                              worst_gap_above=max(c["gap"] for c in steps["cases"] if c["side"] == "above"),
                              worst_gap_below=max(c["gap"] for c in steps["cases"] if c["side"] == "below"),
                              float32_wrong_cases=len(f32), float32_wrong_steps=len({by_place[p]["step"] for p in f32})),
               records_wrong_by_variant={name: {v: sum(len(wrong(g, v)) for g in family(name)["groups"]) for v in VARIANTS}
                                         for name in FAMILIES})
    mk = family("mask_edges")["groups"][0]["mask"]
    rule = mask_cells(mk["msgs"], mk["first"], mk["n_msgs"])
    doc["mask_edges"] = dict(cells_by_frame=[len(c) for c in rule],
                             frames_wrong_by_variant={v: sum(a != b for a, b in zip(mask_cells(mk["msgs"], mk["first"], mk["n_msgs"], variant=v), rule))
                                                      for v in ("no_block_test", "unclamped", "subs_raw", "payload_tones", "gray_swap")})
    return doc


if __name__ == "__main__":
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "messages_constructed.json"), "w") as fh:
        json.dump(report(), fh, indent=1)
        fh.write("\n")
