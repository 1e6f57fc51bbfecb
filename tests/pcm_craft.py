"""Constructed captures for the PCM front end (tests only): random samples in the four formats, the channel lists that reach
every branch of the channel arithmetic, the capture lengths at the edges of the kernel's tiles, CPFSK signals at any of the
rates, and a .wav writer for the reader's tests."""
import struct

import numpy as np

import ft8_spec_pcm as sp

FORMATS = (sp.S16, sp.F32FMT, sp.S16 | sp.COMPLEX, sp.F32FMT | sp.COMPLEX)
FORMAT_NAMES = {sp.S16: "s16-real", sp.F32FMT: "f32-real", sp.S16 | sp.COMPLEX: "s16-complex", sp.F32FMT | sp.COMPLEX: "f32-complex"}
# outputs of stage A per workgroup of the planes kernel as built (pcm.hip), by D
TILE_OUTPUTS = {15: 128, 30: 128, 60: 128, 120: 128, 240: 64}
assert sp.channel(-128) == (0, 0) and sp.channel(-48) == (3, -16) and sp.channel(-177) == (-2, 15)
assert sp.channel(0) == (4, 0) and sp.channel(16) == (5, -16) and sp.channel(47) == (5, 15)


def edge_bins(D, fmt):
    """complex: c = 0 with q = 0; q = -16; q = 15 with a negative c; both ends of the range.  Real: freq_bin 0; q = -16; q = 15;
    the upper end"""
    lo, hi = sp.bin_range(D, fmt)
    return (-128, -48, -177, hi, lo) if fmt & sp.COMPLEX else (0, 16, 47, hi)


def sixteen(D, fmt):
    lo, hi = sp.bin_range(D, fmt)
    edge = edge_bins(D, fmt)
    more = (1, 31, 32, 240, 256, 500, 1000, hi - 1, hi - 255, hi // 2, hi // 3, 2047)
    if fmt & sp.COMPLEX:
        more = (0, -1, lo + 1, lo // 2, lo // 3 - 5) + more
    out = (edge + more)[:16]
    assert len(out) == 16 and all(lo <= b <= hi for b in out)
    return out


def channel_lists(D, fmt):
    """1, 2, 3 and 16 channels"""
    e = edge_bins(D, fmt)
    return (e[:1], e[1:3], e[-3:], sixteen(D, fmt))


def lengths(D):
    """1, M, 4 M + 1, one sample either side of the input under one tile of the planes kernel, an odd length near 20 000"""
    M = D // 3
    tile = TILE_OUTPUTS[D] * M
    return (1, M, 4 * M + 1, tile - 1, tile + 1, 19997)


def nelements(fmt, nsamples):
    return nsamples * (2 if fmt & sp.COMPLEX else 1)


def random_capture(fmt, nsamples, seed):
    """elements of one capture: int16 over the whole range with both ends among them, or float32 normal values of either sign"""
    rng = np.random.default_rng(seed)
    n = nelements(fmt, nsamples)
    if fmt & sp.F32FMT:
        return rng.normal(0.0, 0.3, n).astype(np.float32)
    a = rng.integers(-32768, 32768, n, dtype=np.int16)
    if n >= 4:
        a[1], a[-2] = -32768, 32767
    return a


def ends_capture(fmt, nsamples):
    """zero everywhere but the first and the last sample"""
    n = nelements(fmt, nsamples)
    a = np.zeros(n, np.float32 if fmt & sp.F32FMT else np.int16)
    lo, hi = (-0.75, 0.5) if fmt & sp.F32FMT else (-32768, 32767)
    if fmt & sp.COMPLEX:
        a[:2] = (lo, hi)
        a[-2:] = (hi, lo)
    else:
        a[0], a[-1] = lo, hi
    return a


def cpfsk(tones, f_hz, start_s, nsamples, amplitude, rate):
    """amplitude * exp(i phase), the phase the running sum of the tone frequencies, complex128 [nsamples]; f_hz is tone 0 on the
    input's own axis"""
    symbol = rate * 4 // 25                                  # 0.16 s
    f = np.repeat(f_hz + 6.25 * np.asarray(tones, np.float64), symbol)
    s = int(round(start_s * rate))
    n = min(f.size, nsamples - s)
    out = np.zeros(nsamples, np.complex128)
    out[s:s + n] = amplitude * np.exp(1j * np.cumsum(2.0 * np.pi * f[:n] / rate))
    return out


def to_s16(x):
    return np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def text_of(rec):
    return bytes(rec["text"]).split(b"\0")[0].decode()


def wav_bytes(data, rate, channels, tag, bits, extensible=False, extra_chunks=(), declared=None):
    """a RIFF/WAVE image: data as raw bytes; extra_chunks [(id, body)] go in front of the data chunk, padded to even"""
    block = channels * bits // 8
    if extensible:
        sub = struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * block, block, bits, 22, bits, 0) + sub
    else:
        fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    for cid, chunk in extra_chunks:
        body += cid + struct.pack("<I", len(chunk)) + chunk + (b"\0" if len(chunk) & 1 else b"")
    body += b"data" + struct.pack("<I", len(data) if declared is None else declared) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body
