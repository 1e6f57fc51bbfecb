"""Waterfalls made to order for the sync search (tests only).  ft8_sync_score averages neighbour contrasts over the three Costas
blocks of a position; radio frames and random bytes reach a third of its range (|numerator| < 9000 of 19125), so the packed
16-bit arithmetic of sync.hip, its quotient rule, its thresholds on the numerator and the heap's filter are never put under
load by them.  Here the scores are dictated instead.

The building block is a Costas triple: the cells [t0 + 36 m + k][time_sub][freq_sub][f0 + COSTAS[k]] (blocks inside 0..91) at
amplitude a on a background bg.  Every averaged term of the position (t0, f0) is then a - bg, so on background 0 its score is
exactly a at every t0, the time edges included.  Triples whose blocks are a free block apart and whose bins are a free bin
apart do not read each other's cells: on the lattice t0 in (-12, -4, 4, 12) x f0 = 8 i x the four slices, 512 scores can be
dictated independently, in scan order.

Four families (DESIGN.md "Sync search"), all from fixed seeds, each at most 16 frames: full_scale, quotients, thresholds,
heap_orders.  tests/test_sync_craft_cpu.py proves with the oracle and tests/ft8_spec_decode.py alone that every family has the
properties it is named for; tests/test_gpu_sync_extremes.py sends them through the kernels."""
import functools

import numpy as np

COSTAS = (3, 1, 4, 0, 6, 5, 2)
NBLOCKS, NBIN, MAG_ARRAY = 92, 256, 94208
T0_MIN, T0_COUNT, F0_COUNT = -12, 36, 249
SLICES = ((0, 0), (0, 1), (1, 0), (1, 1))                     # (time_sub, freq_sub) in scan order
LATTICE_T0 = (-12, -4, 4, 12)
LATTICE_F0 = tuple(range(0, 256, 8))
HEAP_MIN_SCORE = 100                                           # above every off-site score of a lattice frame (proved on the CPU)
HEAP_CAPS = (1, 7, 64, 120, 128, 480, 1024)


def navg_of(t0):
    """the number of terms ft8_sync_score averages at time offset t0 (the frequency plays no part)"""
    n = 0
    for m in range(3):
        for k in range(7):
            b = t0 + 36 * m + k
            if 0 <= b < NBLOCKS:
                n += (1 if COSTAS[k] > 0 else 0) + 1 + (1 if k > 0 and b > 0 else 0) + (1 if k < 6 and b + 1 < NBLOCKS else 0)
    return n


NAVG = np.array([navg_of(t0) for t0 in range(T0_MIN, T0_MIN + T0_COUNT)], np.int64)
NAVG_SET = tuple(sorted(set(int(n) for n in NAVG)))
MAX_NUM = 255 * max(NAVG_SET)                                  # every term is a difference of two bytes


def seam_scores():
    """the thresholds at which min_score * navg first passes 32767, for the largest and the smallest navg, and the one before
    each: where the kernel's packed threshold saturates for some time offsets of a frame and not for others"""
    out = []
    for n in (max(NAVG_SET), min(NAVG_SET)):
        first = 32767 // n + 1
        out += [first - 1, first]
    return out


def threshold_scores():
    seams = seam_scores()
    below = [-s for s in seams] + [1 - s for s in seams]      # (min_score - 1) * navg + 1 passes -32768 one score later
    return sorted(set([0, 1, -1, 100, 255, 256, -255, -256] + seams + below))


# ---- the restated rule -------------------------------------------------------------------------------------------------------

def numerators(mag):
    """the sums ft8_sync_score divides, int64 [time_sub][freq_sub][36][249]"""
    wf = np.asarray(mag, np.uint8).reshape(NBLOCKS, 2, 2, NBIN).astype(np.int64)
    out = np.zeros((2, 2, T0_COUNT, F0_COUNT), np.int64)
    f0 = np.arange(F0_COUNT)
    for ts, fs in SLICES:
        p = wf[:, ts, fs, :]
        for ti in range(T0_COUNT):
            acc = np.zeros(F0_COUNT, np.int64)
            for m in range(3):
                for k in range(7):
                    b = ti + T0_MIN + 36 * m + k
                    if not 0 <= b < NBLOCKS:
                        continue
                    col = f0 + COSTAS[k]
                    here = p[b, col]
                    if COSTAS[k] > 0:
                        acc += here - p[b, col - 1]
                    acc += here - p[b, col + 1]
                    if k > 0 and b > 0:
                        acc += here - p[b - 1, col]
                    if k < 6 and b + 1 < NBLOCKS:
                        acc += here - p[b + 1, col]
            out[ts, fs, ti] = acc
    return out


def trunc_div(num, n):
    """C integer division"""
    num = np.asarray(num, np.int64)
    return np.sign(num) * (np.abs(num) // n)


def scores_of(num, mutant=None):
    n = NAVG[None, None, :, None]
    return np.floor_divide(num, n) if mutant == "floor" else trunc_div(num, n)


def packed_threshold(min_score, navg):
    """sync.hip's threshold on the numerator: trunc(num / navg) >= min_score  <=>  num >= T, held in a saturating int16"""
    t = min_score * navg if min_score > 0 else (min_score - 1) * navg + 1
    return max(-32768, min(32767, t))


def select(num, cap, min_score, mutant=None, stats=None):
    """ft8_find_sync on the numerators: [(score, time_offset, freq_offset, time_sub, freq_sub)] in the final order.
    mutant: None = the specification; "threshold" = min_score * navg as the numerator's threshold at every min_score;
    "floor" = floor instead of truncation; "replace_ge" = the heap replaces its minimum on >=.
    stats (a dict) receives survivors, replaced (evictions) and tied (survivors equal to the minimum of the full heap)."""
    sc = scores_of(num, mutant)
    if mutant == "threshold":
        keep = num >= min_score * NAVG[None, None, :, None]
    else:
        keep = sc >= min_score
    heap = []
    replaced = tied = 0

    def down(size):
        c = 0
        while True:
            s, l, r = c, 2 * c + 1, 2 * c + 2
            if l < size and heap[l][0] < heap[s][0]:
                s = l
            if r < size and heap[r][0] < heap[s][0]:
                s = r
            if s == c:
                return
            heap[c], heap[s] = heap[s], heap[c]
            c = s

    si, ti, fi = np.nonzero(keep.reshape(4, T0_COUNT, F0_COUNT))          # scan order
    vals = sc.reshape(4, T0_COUNT, F0_COUNT)[si, ti, fi]
    for s, seg, t, f in zip(vals.tolist(), si.tolist(), ti.tolist(), fi.tolist()):
        if len(heap) == cap:
            tied += s == heap[0][0]
            if s > heap[0][0] or (mutant == "replace_ge" and s == heap[0][0]):
                replaced += 1
                heap[0] = heap[-1]
                heap.pop()
                down(len(heap))
        if len(heap) < cap:
            heap.append((s, t + T0_MIN, f, seg >> 1, seg & 1))
            c = len(heap) - 1
            while c > 0:
                q = (c - 1) // 2
                if heap[c][0] >= heap[q][0]:
                    break
                heap[c], heap[q] = heap[q], heap[c]
                c = q
    size = length = len(heap)
    while length > 1:
        heap[0], heap[length - 1] = heap[length - 1], heap[0]
        length -= 1
        down(length)
    if stats is not None:
        stats.update(survivors=len(vals), replaced=replaced, tied=tied)
    return heap[:size]


def as_list(cands):
    """an oracle / GPU candidate array as select()'s list"""
    return [(int(c["score"]), int(c["time_offset"]), int(c["freq_offset"]), int(c["time_sub"]), int(c["freq_sub"])) for c in cands]


# ---- painting ----------------------------------------------------------------------------------------------------------------

def paint(mag, ts, fs, t0, f0, a):
    """a Costas triple at amplitude a; mag uint8 [94208]"""
    wf = mag.reshape(NBLOCKS, 2, 2, NBIN)
    assert 0 <= f0 < F0_COUNT and T0_MIN <= t0 < T0_MIN + T0_COUNT and 0 <= a <= 255
    for m in range(3):
        for k in range(7):
            b = t0 + 36 * m + k
            if 0 <= b < NBLOCKS:
                wf[b, ts, fs, f0 + COSTAS[k]] = a


def lattice_sites():
    """the 512 sites (time_sub, freq_sub, t0, f0) in scan order"""
    return [(ts, fs, t0, f0) for ts, fs in SLICES for t0 in LATTICE_T0 for f0 in LATTICE_F0]


def lattice_frame(amps):
    """background 0; amps [512] in scan order, 0 = the site stays empty"""
    mag = np.zeros(MAG_ARRAY, np.uint8)
    for (ts, fs, t0, f0), a in zip(lattice_sites(), amps):
        if a:
            paint(mag, ts, fs, t0, f0, int(a))
    return mag


def site_index(sites):
    s = np.array(sites)
    return s[:, 0], s[:, 1], s[:, 2] - T0_MIN, s[:, 3]


def rows_of(j):
    """the time offsets of frame j of a 12-frame set that between them hold every t0 of -12..23, one free block apart:
    j < 8: (-12, -4, 4, 12) + j; j >= 8: (-4, 4, 12, 20) + (j - 8)"""
    return tuple(t + j for t in LATTICE_T0) if j < 8 else tuple(t + j - 8 for t in (-4, 4, 12, 20))


def _grid_sites(j):
    """frame j of the 12: its four rows x every slice x f0 = 8 i + (j mod 8), with f0 = 248 where j mod 8 = 0: over the frames
    every f0 mod 8, i.e. every cell of the four a lane of the kernel owns, in even and odd lanes"""
    s = j % 8
    return [(ts, fs, t0, f0 + s) for ts, fs in SLICES for t0 in rows_of(j) for f0 in LATTICE_F0 if f0 + s < F0_COUNT]


# ---- the families ------------------------------------------------------------------------------------------------------------

def _full_scale():
    """255 on 0 in the slices with (slice + frame) even, 0 on 255 in the others: every t0 (so every navg class, both halves of
    the time range, every wave's run), every slice in both signs, f0 = 0 and 248 and every f0 mod 4"""
    mags, sites = [], []
    for j in range(12):
        mag = np.zeros(MAG_ARRAY, np.uint8)
        wf = mag.reshape(NBLOCKS, 2, 2, NBIN)
        fs_ = []
        for si, (ts, fs) in enumerate(SLICES):
            if (si + j) & 1:
                wf[:, ts, fs, :] = 255
        for ts, fs, t0, f0 in _grid_sites(j):
            bright = not ((2 * ts + fs + j) & 1)
            paint(mag, ts, fs, t0, f0, 255 if bright else 0)
            fs_.append((ts, fs, t0, f0, 255 if bright else -255))
        mags.append(mag)
        sites.append(fs_)
    return dict(mags=np.stack(mags), sites=sites, configs=[(120, 100), (480, 255), (1024, -255)])


QUOTIENT_SEED = 0x51C6                                        # the first seed from 0x51C0 on whose frames hold every residue (quotient_coverage)


def _quotients(seed=QUOTIENT_SEED):
    """random amplitudes 170..255 on backgrounds 0..8 (positive numerators) and 0..85 on 247..255 (negative ones), the sites of
    _grid_sites: every |numerator| at a site is above 8192 and lands anywhere modulo navg"""
    rng = np.random.default_rng(seed)
    mags, sites = [], []
    for j in range(12):
        mag = np.zeros(MAG_ARRAY, np.uint8)
        wf = mag.reshape(NBLOCKS, 2, 2, NBIN)
        for si, (ts, fs) in enumerate(SLICES):
            lo = 247 if (si + j) & 1 else 0
            wf[:, ts, fs, :] = rng.integers(lo, lo + 9, (NBLOCKS, NBIN))
        fs_ = []
        for ts, fs, t0, f0 in _grid_sites(j):
            bright = not ((2 * ts + fs + j) & 1)
            paint(mag, ts, fs, t0, f0, int(rng.integers(170, 256)) if bright else int(rng.integers(0, 86)))
            fs_.append((ts, fs, t0, f0))
        mags.append(mag)
        sites.append(fs_)
    return dict(mags=np.stack(mags), sites=sites, configs=[(120, 100), (1024, 0), (1024, -256)])


def quotient_coverage(nums):
    """{(navg, sign, r)}: a numerator with |num| > 8192, that sign and num = r (mod navg), r in (-1, 0, 1), occurs"""
    have = set()
    for num in nums:
        for ti in range(T0_COUNT):
            n = int(NAVG[ti])
            v = num[:, :, ti, :].reshape(-1)
            v = v[np.abs(v) > 8192]
            for r in (-1, 0, 1):
                hit = v[(v - r) % n == 0]
                have |= {(n, int(s), r) for s in np.unique(np.sign(hit))}
    return have


def _thresholds():
    """one lattice frame with every amplitude 1..255 (each twice, and two more), in seeded order"""
    rng = np.random.default_rng(0x7E5)
    amps = rng.permutation(np.concatenate([np.arange(1, 256), np.arange(1, 256), [100, 255]]))
    return dict(mags=lattice_frame(amps)[None], amps=[amps], configs=[(cap, ms) for ms in threshold_scores() for cap in (120, 1024)])


HEAP_FRAMES = ("ascending", "descending", "equal", "falling_plateaus", "rising_plateaus", "sawtooth", "shuffled")


def heap_amps(name):
    """the amplitudes of the 512 lattice sites in scan order (0 = empty site).  Every painted amplitude is >= HEAP_MIN_SCORE,
    so the survivors at that threshold are the painted sites, in this order."""
    i = np.arange(512)
    if name in ("ascending", "descending"):                    # strictly: 156 distinct scores 100..255 on sites spread over the scan
        at = np.sort(np.random.default_rng(0xA5C).choice(512, 156, replace=False))
        amps = np.zeros(512, np.int64)
        amps[at] = np.arange(100, 256) if name == "ascending" else np.arange(255, 99, -1)
        return amps
    if name == "equal":
        return np.full(512, 200)
    if name == "falling_plateaus":                             # ties in runs [16 k - 8, 16 k + 8): across every multiple of 64 and every cap
        return 255 - 4 * ((i + 8) // 16)
    if name == "rising_plateaus":
        return 120 + 4 * ((i + 8) // 16)
    if name == "sawtooth":
        return 100 + 3 * (i % 50)
    if name == "shuffled":
        return np.random.default_rng(0x5AF).integers(100, 256, 512)
    raise KeyError(name)


def _heap_orders():
    amps = [heap_amps(n) for n in HEAP_FRAMES]
    return dict(mags=np.stack([lattice_frame(a) for a in amps]), amps=amps, names=HEAP_FRAMES,
                configs=[(cap, HEAP_MIN_SCORE) for cap in HEAP_CAPS])


FAMILIES = ("full_scale", "quotients", "thresholds", "heap_orders")


@functools.lru_cache(maxsize=None)
def family(name):
    """dict(mags uint8 [B][94208] read-only, configs [(max_candidates, min_score)], and what the CPU test holds the frames to)"""
    d = dict(full_scale=_full_scale, quotients=_quotients, thresholds=_thresholds, heap_orders=_heap_orders)[name]()
    assert len(d["mags"]) <= 16
    d["mags"].setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def family_numerators(name):
    return [numerators(m) for m in family(name)["mags"]]


def random_byte_frames(n=70):
    """the extra frames of test_heap_forms_are_exact (tests/test_gpu_parity.py): what the sync tests reached before"""
    rng = np.random.default_rng(9)
    return [rng.integers(0, 256, MAG_ARRAY, dtype=np.uint8) for _ in range(n)]
