"""Constructed 2.4 Msps captures for the wideband RX front end (tests only): random bytes, the special captures of the stage
tests, the channel lists that reach every branch of the channel arithmetic, and CPFSK signals quantised to bytes over noise."""
import numpy as np

import ft8_spec_wide as sw

SYMBOL = 384000                                             # samples of one FT8 symbol at 2.4 Msps
# freq_bin values: c = 0 with q = 0; q = -32 (c = 100); q = 31 with a negative c (c = -50); the two ends of the range
EDGE_BINS = (-128, 6240, -3297, 176000, -176000)
SIXTEEN = EDGE_BINS + (0, 48000, 48240, -66000, -65760, 1, -1, 63, 64, 175999, -97)
assert len(SIXTEEN) == 16
assert sw.channel(-128) == (0, 0) and sw.channel(6240) == (100, -32) and sw.channel(-3297) == (-50, 31)
assert sw.channel(176000) == (2752, 0) and sw.channel(-176000) == (-2748, 0)
LENGTHS = (8, 752, 48000, 192008)


def random_capture(npairs, seed):
    """uniform bytes that include 0 and 255 -> uint8 [2 npairs]"""
    raw = np.random.default_rng(seed).integers(0, 256, 2 * npairs, dtype=np.uint8)
    raw[1], raw[-2] = 0, 255
    return raw


def ends_capture(npairs):
    """0x80 everywhere except (0x00, 0xFF) in the first pair and (0xFF, 0x00) in the last"""
    raw = np.full(2 * npairs, 0x80, np.uint8)
    raw[:2] = (0x00, 0xFF)
    raw[-2:] = (0xFF, 0x00)
    return raw


def cpfsk(tones, f_hz, start_s, npairs, amplitude):
    """amplitude * exp(i phase), the phase the running sum of the tone frequencies, complex128 [npairs]; f_hz is tone 0 relative
    to the capture's centre"""
    f = np.repeat(f_hz + 6.25 * np.asarray(tones, np.float64), SYMBOL)
    s = int(round(start_s * sw.RATE))
    n = min(f.size, npairs - s)
    out = np.zeros(npairs, np.complex128)
    out[s:s + n] = amplitude * np.exp(1j * np.cumsum(2.0 * np.pi * f[:n] / sw.RATE))
    return out


def to_bytes(x):
    """complex samples -> interleaved unsigned bytes, rounded and clipped"""
    raw = np.empty(2 * x.shape[0], np.uint8)
    raw[0::2] = np.clip(np.rint(x.real) + 128, 0, 255).astype(np.uint8)
    raw[1::2] = np.clip(np.rint(x.imag) + 128, 0, 255).astype(np.uint8)
    return raw


def text_of(rec):
    return bytes(rec["text"]).split(b"\0")[0].decode()
