"""rtlsdr_ft8d_amd -- Python view of libft8gpu.so (include/ft8gpu.h).

The product is the C-ABI shared library built from ``csrc/`` (hand-written HIP kernels for
gfx950 + C host side).  This module only binds it with ctypes for the tests and ``bench.py``;
there is no Python or CPU fallback: if the library is missing, import of the binding raises.
"""
import ctypes as C
import glob
import hashlib
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libft8gpu.so")
AB_LIB_PATH = os.path.join(_HERE, "libft8gpu_ab.so")      # `make -C csrc ab`: product kernels + the alternative kernel forms

NSAMPLES = 48000            # rtlsdr_ft8d.h:34-35
MAG_ARRAY = 94208           # rtlsdr_ft8d.h:56
MAX_MESSAGES = 50           # rtlsdr_ft8d.h:46
SCORES_PER_FRAME = 2 * 2 * 36 * 249
HOST_PTRS, DEVICE_PTRS = 0, 1

RESULT_DTYPE = np.dtype([("call", "S13"), ("loc", "S7"), ("freq", "<i4"), ("snr", "<i4")], align=True)
CAND_DTYPE = np.dtype([("score", "<i2"), ("time_offset", "<i2"), ("freq_offset", "<i2"),
                       ("time_sub", "u1"), ("freq_sub", "u1")])
STATUS_DTYPE = np.dtype([("ldpc_errors", "<i2"), ("iters", "<i2"), ("crc_extracted", "<u2"),
                         ("crc_calculated", "<u2"), ("unpack_status", "i1"), ("ok", "u1"),
                         ("a91", "u1", (12,)), ("text", "S25"), ("pad", "u1")])
SIGNAL_DTYPE = np.dtype([("tones", "u1", (79,)), ("pad", "u1"), ("f0_hz", "<f4"), ("t0_s", "<f4"),
                         ("amplitude", "<f4")])
# ft8gpu_message: every unique message of a frame with SNR estimate, time offset and frequency (ft8gpu_decode_messages)
# ft8gpu_rx_state: the statics of rtlsdr_callback() (rtlsdr_ft8d.c:76-202), 516 bytes without padding
RX_STATE_DTYPE = np.dtype([(n, "<i4") for n in ("Ix1", "Ix2", "Qx1", "Qx2", "Iy1", "It1y", "It1z", "Qy1", "Qt1y", "Qt1z",
                                                "Iy2", "It2y", "It2z", "Qy2", "Qt2y", "Qt2z")]
                          + [("decimationIndex", "<u4"), ("firI", "<f4", (56,)), ("firQ", "<f4", (56,))])
MESSAGE_DTYPE = np.dtype({"names": ["text", "snr_db", "score", "freq_hz", "dt_s", "hash", "cand_index", "cand", "a91", "pad"],
                          "formats": ["S25", "i1", "<i2", "<f4", "<f4", "<u2", "<u2", CAND_DTYPE, ("u1", (12,)), ("u1", (4,))],
                          "offsets": [0, 25, 26, 28, 32, 36, 38, 40, 48, 60], "itemsize": 64})
# ft8gpu_osd_info: what ordered-statistics decoding found for a candidate (ft8gpu_osd_candidates)
OSD_INFO_DTYPE = np.dtype([("result", "u1"), ("nhard", "u1"), ("pattern", "<u2"), ("metric", "<i4")])
OSD_MAX_HARD_ERRORS = 27    # FT8GPU_OSD_MAX_HARD_ERRORS, the recommended gate
# ft8gpu_ap_info / ft8gpu_ap_hypothesis: a-priori decoding (ft8gpu_ap_candidates)
AP_INFO_DTYPE = np.dtype([("result", "u1"), ("nhard", "u1"), ("hyp", "u1"), ("iters", "u1"), ("results", "u1", (4,))])
AP_HYP_DTYPE = np.dtype([("mask", "u1", (10,)), ("bits", "u1", (10,))])
AP_MAX_HYPOTHESES = 4       # FT8GPU_AP_MAX_HYPOTHESES
AP_MAX_HARD_ERRORS = 40     # FT8GPU_AP_MAX_HARD_ERRORS, the recommended gate
assert RESULT_DTYPE.itemsize == 28 and CAND_DTYPE.itemsize == 8 and MESSAGE_DTYPE.itemsize == 64 and OSD_INFO_DTYPE.itemsize == 8
assert AP_INFO_DTYPE.itemsize == 8 and AP_HYP_DTYPE.itemsize == 20
# ft8gpu_callhash_entry / ft8gpu_callhash_state / ft8gpu_resolved: the call hash table of a receiver (ft8gpu_resolve_calls)
CALLHASH_ENTRIES = 4096     # FT8GPU_CALLHASH_ENTRIES
CALLHASH_ENTRY_DTYPE = np.dtype([("call", "S11"), ("len", "u1"), ("h22", "<u4")])
CALLHASH_STATE_DTYPE = np.dtype([("entry", CALLHASH_ENTRY_DTYPE, (CALLHASH_ENTRIES,)), ("stamp", "<u4", (CALLHASH_ENTRIES,)),
                                 ("slot", "<u4"), ("pad", "<u4", (3,))])
RESOLVED_DTYPE = np.dtype([("text", "S40"), ("n_hashed", "u1"), ("n_resolved", "u1"), ("n_inserted", "u1"),
                           ("resolved_mask", "u1"), ("pad", "u1", (4,))])
assert CALLHASH_ENTRY_DTYPE.itemsize == 16 and CALLHASH_STATE_DTYPE.itemsize == 81936 and RESOLVED_DTYPE.itemsize == 48
assert STATUS_DTYPE.itemsize == 48 and SIGNAL_DTYPE.itemsize == 92
# ft8gpu_expect_entry / ft8gpu_expect_state / ft8gpu_match_info: the expected messages of a receiver (ft8gpu_match_candidates)
EXPECT_ENTRIES = 512        # FT8GPU_EXPECT_ENTRIES
EXPECT_ENTRY_DTYPE = np.dtype([("payload", "u1", (10,)), ("used", "u1"), ("kind", "u1"), ("stamp", "<u4")])
EXPECT_STATE_DTYPE = np.dtype([("entry", EXPECT_ENTRY_DTYPE, (EXPECT_ENTRIES,)), ("cursor", "<u4"), ("slot", "<u4"), ("pad", "<u4", (2,))])
MATCH_INFO_DTYPE = np.dtype([("result", "u1"), ("nhard", "u1"), ("index", "<u2"), ("metric", "<i4")])
MATCH_MAX_HARD_ERRORS = 49  # FT8GPU_MATCH_MAX_HARD_ERRORS, the recommended gate
assert EXPECT_ENTRY_DTYPE.itemsize == 16 and EXPECT_STATE_DTYPE.itemsize == 8208 and MATCH_INFO_DTYPE.itemsize == 8
# ft8gpu_hint_entry / ft8gpu_hint_state / ft8gpu_hint_info: the call hints of a receiver (ft8gpu_hint_candidates)
HINT_ENTRIES = 512          # FT8GPU_HINT_ENTRIES
HINT_ENTRY_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("stamp", "<u4"), ("kind", "u1"), ("used", "u1"), ("phase", "u1"), ("pad", "u1")])
HINT_STATE_DTYPE = np.dtype([("entry", HINT_ENTRY_DTYPE, (HINT_ENTRIES,)), ("cursor", "<u4"), ("slot", "<u4"), ("pad", "<u4", (2,))])
HINT_INFO_DTYPE = np.dtype([("result", "u1"), ("nhard", "u1"), ("ntried", "u1"), ("iters", "u1"), ("results", "u1", (4,)),
                            ("index", "<u2", (4,))])
HINT_MAX_BAD_PER_64 = 24    # FT8GPU_HINT_MAX_BAD_PER_64, FT8GPU_HINT_TRIES, FT8GPU_HINT_MAX_HARD_ERRORS: the recommended values
HINT_TRIES = 4
HINT_MAX_HARD_ERRORS = 40
assert HINT_ENTRY_DTYPE.itemsize == 16 and HINT_STATE_DTYPE.itemsize == 8208 and HINT_INFO_DTYPE.itemsize == 16
# ft8gpu_softmem_entry / ft8gpu_softmem_state / ft8gpu_combine_info: the soft-bit memory of a receiver (ft8gpu_combine_candidates)
SOFTMEM_ENTRIES = 128       # FT8GPU_SOFTMEM_ENTRIES
SOFTMEM_ENTRY_DTYPE = np.dtype([("cand", CAND_DTYPE), ("used", "u1"), ("count", "u1"), ("pad", "<u2"), ("stamp", "<u4"),
                                ("llr", "<f4", (176,))])
SOFTMEM_STATE_DTYPE = np.dtype([("entry", SOFTMEM_ENTRY_DTYPE, (SOFTMEM_ENTRIES,)), ("cursor", "<u4"), ("slot", "<u4"),
                                ("pad", "<u4", (2,))])
COMBINE_INFO_DTYPE = np.dtype([("result", "u1"), ("nagree", "u1"), ("index", "u1"), ("count", "u1"), ("nhard", "u1"),
                               ("pad", "u1", (3,))])
COMBINE_MIN_AGREE = 88           # FT8GPU_COMBINE_MIN_AGREE, the recommended gate
COMBINE_STORE_PER_SLOT = 48      # FT8GPU_COMBINE_STORE_PER_SLOT, the recommended number of candidates stored per slot
# refined time and frequency (ft8gpu_refine_messages): the powers around a record's position in the I/Q samples
REFINED_DTYPE = np.dtype([("e_best", "<i2"), ("valid", "u1"), ("pad0", "u1"), ("pt", "<f4", (3,)), ("pf", "<f4", (5,)),
                          ("noise", "<f4"), ("pad", "u1", (8,))])
assert REFINED_DTYPE.itemsize == 48
# subtraction in the I/Q samples (ft8gpu_subtract_messages): what the fine search chose for a record
SUBTRACT_INFO_DTYPE = np.dtype([("k4", "<i4"), ("s_best", "<i4"), ("d_best", "i1"), ("t_best", "i1"), ("valid", "u1"), ("pad0", "u1"),
                                ("pf", "<f4", (5,)), ("pt", "<f4", (5,)), ("pad", "u1", (12,))])
SUBTRACT_TABLE = 4096            # FT8GPU_SUBTRACT_TABLE
SUBTRACT_CPFSK, SUBTRACT_GFSK = 0, 1   # FT8GPU_SUBTRACT_CPFSK / _GFSK: the shape of the reference a record is subtracted with
assert SUBTRACT_INFO_DTYPE.itemsize == 64
assert SOFTMEM_ENTRY_DTYPE.itemsize == 720 and SOFTMEM_STATE_DTYPE.itemsize == 92176 and COMBINE_INFO_DTYPE.itemsize == 8
# demodulation from the I/Q samples (ft8gpu_demod_candidates): what the second demodulation found for a candidate
DEMOD_INFO_DTYPE = np.dtype([("result", "u1"), ("set", "u1"), ("nhard", "u1"), ("e_best", "i1"), ("d_best", "i1"), ("pad0", "u1", (3,)),
                             ("psync", "<f4"), ("pad", "u1", (4,))])
DEMOD_MAX_HARD_ERRORS = 174      # FT8GPU_DEMOD_MAX_HARD_ERRORS, the recommended gate
DEMOD_SETS = 7                   # FT8GPU_DEMOD_SETS, the recommended mask of soft-bit sets
# AP on the demodulated soft bits (ft8gpu_demod_soft, ft8gpu_ap_soft_candidates): soft [B][cap][3][SOFT_STRIDE] float32
SOFT_STRIDE = 176                # FT8GPU_SOFT_STRIDE
APSOFT_INFO_DTYPE = np.dtype([("result", "u1"), ("nhard", "u1"), ("hyp", "u1"), ("iters", "u1"), ("set", "u1"), ("pad", "u1", (3,)),
                              ("results", "u1", (3, 4))])
APSOFT_MAX_HARD_ERRORS = 174     # FT8GPU_APSOFT_MAX_HARD_ERRORS, the recommended gate
assert APSOFT_INFO_DTYPE.itemsize == 20
AUDIO_RATE = 12000               # FT8GPU_AUDIO_RATE
AUDIO_NSAMPLES = 180000          # FT8GPU_AUDIO_NSAMPLES
AUDIO_TAPS = 160                 # FT8GPU_AUDIO_TAPS
AUDIO_MIX = 1920                 # FT8GPU_AUDIO_MIX
AUDIO_MAX_BANDS = 4              # FT8GPU_AUDIO_MAX_BANDS
AUDIO_MAX_BASE = 704             # FT8GPU_AUDIO_MAX_BASE
AUDIO_S16, AUDIO_F32 = 0, 1      # FT8GPU_AUDIO_S16 / _F32
GFSK_IQ, GFSK_AUDIO = 0, 1       # FT8GPU_GFSK_IQ / _AUDIO
WIDE_RATE = 2400000              # FT8GPU_WIDE_RATE
WIDE_MAX_PAIRS = 36000000        # FT8GPU_WIDE_MAX_PAIRS
WIDE_MIX1, WIDE_MIX2 = 6000, 3072    # FT8GPU_WIDE_MIX1 / _MIX2
WIDE_TAPS = 96                   # FT8GPU_WIDE_TAPS
WIDE_MAX_CHANNELS = 16           # FT8GPU_WIDE_MAX_CHANNELS
WIDE_MAX_BIN = 176000            # FT8GPU_WIDE_MAX_BIN
PCM_S16, PCM_F32, PCM_COMPLEX = 0, 1, 2   # FT8GPU_PCM_S16 / _F32 / _COMPLEX (added to either)
PCM_RATES = (48000, 96000, 192000, 384000, 768000)   # 3200 D, D = 15 .. 240
PCM_MIX2 = 1536                  # FT8GPU_PCM_MIX2
PCM_TAPS_B = 48                  # FT8GPU_PCM_TAPS_B
PCM_MAX_CHANNELS = 16            # FT8GPU_PCM_MAX_CHANNELS
PCM_MAX_SAMPLES = 11520000       # FT8GPU_PCM_MAX_SAMPLES
GFSK_SPS_IQ, GFSK_SPS_AUDIO = 512, 1920   # FT8GPU_GFSK_SPS_IQ / _AUDIO
GFSK_TWIDDLES = 4096             # FT8GPU_GFSK_TWIDDLES
GFSK_MAX_SIGNALS = 64            # FT8GPU_GFSK_MAX_SIGNALS
GFSK_TILE = 8192                 # FT8GPU_GFSK_TILE: output samples per workgroup of the kernel as built
# ft8gpu_channel (16 bytes): a signal's fading channel, parallel to SIGNAL_DTYPE records (include/ft8gpu.h "Fading channel")
CHANNEL_DTYPE = np.dtype([("spread_hz", "<f4"), ("delay_ms", "<f4"), ("path2_gain", "<f4"), ("mode", "<u4")])
assert CHANNEL_DTYPE.itemsize == 16
CHANNEL_NONE, CHANNEL_FADED = 0, 1   # FT8GPU_CHANNEL_NONE / _FADED
CHANNEL_TAPS = 16                # FT8GPU_CHANNEL_TAPS
CHANNEL_GRID = 1265              # FT8GPU_CHANNEL_GRID
# FT8GPU_CHANNEL_QUIET / _MODERATE / _DISTURBED / _FLUTTER: (spread_hz, delay_ms, path2_gain, mode)
CHANNEL_PRESETS = {"quiet": (0.1, 0.5, 1.0, 1), "moderate": (0.5, 1.0, 1.0, 1), "disturbed": (1.0, 2.0, 1.0, 1), "flutter": (10.0, 0.5, 1.0, 1)}
assert DEMOD_INFO_DTYPE.itemsize == 16


class Params(C.Structure):
    _fields_ = [("min_score", C.c_int32), ("max_candidates", C.c_int32), ("ldpc_iters", C.c_int32)]


class DeepParams(C.Structure):
    """ft8gpu_deep_params: passes 1..4, osd_order -1 (no OSD) .. 2, osd_max_hard_errors 0..83"""
    _fields_ = [("passes", C.c_int32), ("osd_order", C.c_int32), ("osd_max_hard_errors", C.c_int32)]


class ApHypothesis(C.Structure):
    """ft8gpu_ap_hypothesis: 77 payload bits with a mask, numbered as in a91 (MSB first)"""
    _fields_ = [("mask", C.c_uint8 * 10), ("bits", C.c_uint8 * 10)]


class ApParams(C.Structure):
    """ft8gpu_ap_params: passes 1..4, nhyp 0 (no AP) .. 4, ap_max_hard_errors 0..174, osd_order -1 (no OSD) .. 2,
    osd_max_hard_errors 0..83, hyps[4]"""
    _fields_ = [("passes", C.c_int32), ("nhyp", C.c_int32), ("ap_max_hard_errors", C.c_int32), ("osd_order", C.c_int32),
                ("osd_max_hard_errors", C.c_int32), ("hyps", ApHypothesis * 4)]


class ExpectParams(C.Structure):
    """ft8gpu_expect_params: max_hard_errors 0..174, max_age in slots (0: never expires), derive != 0: RRR / RR73 / 73"""
    _fields_ = [("max_hard_errors", C.c_int32), ("max_age", C.c_uint32), ("derive", C.c_int32)]


class HintParams(C.Structure):
    """ft8gpu_hint_params: tries 1..4, max_bad_per_64 0..64, max_hard_errors 0..174, max_age in slots (0: never expires),
    use_phase != 0: only entries of the slot's parity are live"""
    _fields_ = [("tries", C.c_int32), ("max_bad_per_64", C.c_int32), ("max_hard_errors", C.c_int32), ("max_age", C.c_uint32),
                ("use_phase", C.c_int32)]


class CombineParams(C.Structure):
    """ft8gpu_combine_params: min_agree 0..174, max_age in slots (0: never expires), store_per_slot 0..128"""
    _fields_ = [("min_agree", C.c_int32), ("max_age", C.c_uint32), ("store_per_slot", C.c_int32)]


class DemodParams(C.Structure):
    """ft8gpu_demod_params: sets 1..7 (bit n - 1: set n), max_hard_errors 0..174, max_per_frame 0..max_candidates"""
    _fields_ = [("sets", C.c_int32), ("max_hard_errors", C.c_int32), ("max_per_frame", C.c_int32)]


class DemodApParams(C.Structure):
    """ft8gpu_demod_ap_params: the demodulation's parameters, nhyp 0 (no AP) .. 4, ap_max_hard_errors 0..174, hyps[4]"""
    _fields_ = [("demod", DemodParams), ("nhyp", C.c_int32), ("ap_max_hard_errors", C.c_int32), ("hyps", ApHypothesis * 4)]


class Timings(C.Structure):
    _fields_ = [("waterfall_ms", C.c_float), ("sync_ms", C.c_float), ("heap_ms", C.c_float),
                ("decode_ms", C.c_float), ("spots_ms", C.c_float), ("total_ms", C.c_float),
                ("launches_per_stage", C.c_int32)]


class ReportInfo(C.Structure):
    """ft8gpu_report_info: receiver identity and the per-datagram constants of postSpots() (rtlsdr_ft8d.c:365-590)"""
    _fields_ = [("rcall", C.c_char * 13), ("rloc", C.c_char * 7), ("app_version", C.c_char * 32),
                ("dial_freq", C.c_uint32), ("unixtime", C.c_uint32), ("sequence", C.c_uint32),
                ("random_id", C.c_uint32)]


DATAGRAM_STRIDE = 1408
STREAM_LEGACY = 1                       # FT8GPU_STREAM_LEGACY (= hipStreamLegacy): the legacy null stream, explicitly
DBG_FORCE_IEEE_DIV, DBG_PIPELINE_FORM, DBG_NO_OVERLAP = 1, 2, 4      # FT8GPU_DBG_* test hooks (per context)
# selector bits of the alternative (bit-identical) kernel forms: accepted by the A/B build only (csrc/ft8gpu_internal.h)
AB_WATERFALL_LDS, AB_HEAP_LANE_PER_FRAME, AB_HEAP_WAVE_PER_FRAME = 8, 16, 32
AB_HINT_IN_WAVE = 64                                                 # call hints: the form without the pre-kernel (A/B build)


class Ft8GpuError(RuntimeError):
    pass


ABI_SYMBOLS = [
    "ft8gpu_create", "ft8gpu_destroy", "ft8gpu_set_stream", "ft8gpu_get_stream", "ft8gpu_set_params", "ft8gpu_enable_timing",
    "ft8gpu_get_timings", "ft8gpu_synchronize", "ft8gpu_last_error", "ft8gpu_device_count",
    "ft8gpu_decode_batch", "ft8gpu_waterfall", "ft8gpu_find_sync", "ft8gpu_score_map",
    "ft8gpu_decode_candidates", "ft8gpu_collect_spots", "ft8gpu_pack77_std", "ft8gpu_encode",
    "ft8gpu_synth_frames", "ft8gpu_synth_frames_at", "ft8gpu_rx_decimate", "ft8gpu_pskreporter_datagrams", "ft8gpu_format_spots",
    "ft8gpu_rx_stream", "ft8gpu_rx_state_reset",
    "ft8gpu_dev_alloc", "ft8gpu_dev_free", "ft8gpu_memcpy_h2d", "ft8gpu_memcpy_d2h", "ft8gpu_host_alloc", "ft8gpu_host_free",
    "ft8gpu_overlap_active", "ft8gpu_overlap_reason", "ft8gpu_build_id", "ft8gpu_pack77",
    "ft8gpu_set_debug_flags", "ft8gpu_selftest_bp_math", "ft8gpu_selftest_norm_math", "ft8gpu_selftest_quantiser", "ft8gpu_gather_spots", "ft8gpu_gather_shutdown",
    "ft8gpu_shard_workers", "ft8gpu_decode_batch_multi", "ft8gpu_decode_batch_multi_dev",
    "ft8gpu_decode_messages", "ft8gpu_collect_messages", "ft8gpu_noise_baseline", "ft8gpu_format_messages",
    "ft8gpu_decode_messages_passes", "ft8gpu_mask_messages", "ft8gpu_append_messages",
    "ft8gpu_osd_candidates", "ft8gpu_decode_messages_deep",
    "ft8gpu_ap_candidates", "ft8gpu_ap_from_text", "ft8gpu_decode_messages_ap",
    "ft8gpu_resolve_calls", "ft8gpu_decode_messages_resolved", "ft8gpu_callhash_reset", "ft8gpu_call_hash",
    "ft8gpu_callhash_insert", "ft8gpu_callhash_lookup", "ft8gpu_format_resolved",
    "ft8gpu_match_candidates", "ft8gpu_expect_update", "ft8gpu_decode_messages_expected", "ft8gpu_expect_reset",
    "ft8gpu_expect_insert", "ft8gpu_expect_insert_text",
    "ft8gpu_hint_candidates", "ft8gpu_hint_update", "ft8gpu_decode_messages_hinted", "ft8gpu_hint_reset", "ft8gpu_hint_insert",
    "ft8gpu_hint_insert_text", "ft8gpu_hint_hypothesis",
    "ft8gpu_combine_candidates", "ft8gpu_softmem_update", "ft8gpu_decode_messages_combined", "ft8gpu_softmem_reset",
    "ft8gpu_refine_messages", "ft8gpu_decode_messages_refined", "ft8gpu_refined_estimate", "ft8gpu_format_messages_refined",
    "ft8gpu_subtract_messages", "ft8gpu_decode_messages_subtracted", "ft8gpu_subtract_twiddles",
    "ft8gpu_subtract_messages_shaped", "ft8gpu_decode_messages_subtracted_shaped",
    "ft8gpu_demod_candidates", "ft8gpu_decode_messages_demod",
    "ft8gpu_demod_soft", "ft8gpu_ap_soft_candidates", "ft8gpu_decode_messages_demod_ap",
    "ft8gpu_audio_taps", "ft8gpu_audio_mixer", "ft8gpu_audio_frames", "ft8gpu_decode_audio", "ft8gpu_read_wav",
    "ft8gpu_gfsk_pulse", "ft8gpu_gfsk_ramp", "ft8gpu_gfsk_twiddles", "ft8gpu_synth_gfsk_frames", "ft8gpu_synth_gfsk_audio",
    "ft8gpu_write_wav",
    "ft8gpu_channel_taps", "ft8gpu_channel_check", "ft8gpu_channel_clip", "ft8gpu_synth_gfsk_frames_faded", "ft8gpu_synth_gfsk_audio_faded",
    "ft8gpu_wide_mixer1", "ft8gpu_wide_mixer2", "ft8gpu_wide_taps", "ft8gpu_wide_frames", "ft8gpu_decode_wide",
    "ft8gpu_pcm_decimation", "ft8gpu_pcm_mixer1", "ft8gpu_pcm_mixer2", "ft8gpu_pcm_taps_a", "ft8gpu_pcm_taps_b", "ft8gpu_pcm_frames",
    "ft8gpu_decode_pcm", "ft8gpu_read_wav_pcm",
    "ft8_find_sync", "ft8_decode", "ft8_encode", "pack77",            # ft8_lib level (include/ft8_lib/ft8/*.h)
    "initFFTW", "freeFFTW", "ft8_subsystem", "ft8gpu_read_raw_iq", "ft8gpu_read_c2", "ft8gpu_write_raw_iq",
]

_lib = None


def _hash16(paths):
    h = hashlib.sha256()
    for path in paths:
        with open(path, "rb") as f:
            h.update(os.path.basename(path).encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def source_build_id():
    """what ft8gpu_build_id() of a library built from THIS tree returns (csrc/Makefile computes the same two hashes):
    "<dev>.<all>" -- device sources (csrc/*.hip, *.h), and every source of the library (+ csrc/*.c, Makefile, the linker version script, include/)"""
    d = os.path.join(_HERE, "csrc")
    inc = os.path.join(os.path.dirname(_HERE), "include")
    dev = sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.h")), key=os.path.basename)
    rest = sorted(glob.glob(os.path.join(d, "*.c")), key=os.path.basename) + [os.path.join(d, "Makefile"), os.path.join(d, "libft8gpu.map"), os.path.join(inc, "ft8gpu.h")] + \
        sorted(glob.glob(os.path.join(inc, "ft8_lib", "ft8", "*.h")), key=os.path.basename)
    return f"{_hash16(dev)}.{_hash16(dev + rest)}"


def device_source_id():
    """the first half of the build id: identity of the kernel sources (what committed PMC summaries are gated on)"""
    return source_build_id().split(".")[0]


def build_id(lib=None):
    return (lib or load_library()).ft8gpu_build_id().decode()


def check_build_id(lib=None, suffix=""):
    """raises unless the loaded library was built from the sources beside it"""
    have, want = build_id(lib), source_build_id() + suffix
    if have != want:
        raise Ft8GpuError(f"libft8gpu{'_ab' if suffix else ''}.so is stale or foreign: its build id is {have}, the sources beside it give {want} "
                          "(rebuild: make -C rtlsdr_ft8d_amd/csrc" + (" ab)" if suffix else ")"))
    return have


def load_library():
    """dlopen libft8gpu.so and declare prototypes.  Raises if the HIP extension is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own HIP/HSA runtime under the same SONAME (libamdhip64.so.7) as
    # /opt/rocm's.  A process must hold exactly ONE of them: two copies each open the GPU and the
    # second one finds no devices.  Importing torch first makes the dynamic loader resolve this
    # library's libamdhip64.so.7 dependency to the copy torch already mapped.  (A plain C caller
    # such as rtlsdr_ft8d.c simply gets /opt/rocm's runtime.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise Ft8GpuError(
            f"{LIB_PATH} is missing: build it with `make -C rtlsdr_ft8d_amd/csrc` "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    _lib = _declare(C.CDLL(LIB_PATH))
    return _lib


def load_ab_library():
    """the A/B build (product kernels + alternative kernel forms behind extra debug-flag bits), checked against the tree"""
    if not os.path.exists(AB_LIB_PATH):
        raise Ft8GpuError(f"{AB_LIB_PATH} is missing: build it with `make -C rtlsdr_ft8d_amd/csrc ab`")
    L = load_library_at(AB_LIB_PATH)
    check_build_id(L, "+ab")
    return L


def load_library_at(path):
    """another build of libft8gpu.so beside the product's (tools/ab_libs.py: A/B of two builds in one process)"""
    load_library()                                   # the product library first: it fixes which HIP runtime is mapped
    return _declare(C.CDLL(os.path.abspath(path)))


def _declare(L):
    vp, i32p = C.c_void_p, C.POINTER(C.c_int32)
    L.ft8gpu_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(Params)]
    L.ft8gpu_destroy.argtypes = [vp]
    L.ft8gpu_destroy.restype = None
    L.ft8gpu_set_stream.argtypes = [vp, vp]
    if hasattr(L, "ft8gpu_get_stream"):
        L.ft8gpu_get_stream.argtypes = [vp]
        L.ft8gpu_get_stream.restype = vp
    L.ft8gpu_set_params.argtypes = [vp, C.POINTER(Params)]
    L.ft8gpu_enable_timing.argtypes = [vp, C.c_int]
    L.ft8gpu_get_timings.argtypes = [vp, C.POINTER(Timings), C.POINTER(C.c_int32)]
    L.ft8gpu_synchronize.argtypes = [vp]
    L.ft8gpu_last_error.restype = C.c_char_p
    L.ft8gpu_decode_batch.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int]
    L.ft8gpu_waterfall.argtypes = [vp, vp, C.c_int, vp, C.c_int]
    L.ft8gpu_find_sync.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int]
    L.ft8gpu_score_map.argtypes = [vp, vp, C.c_int, vp, C.c_int]
    L.ft8gpu_decode_candidates.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.c_int]
    L.ft8gpu_collect_spots.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int]
    L.ft8gpu_pack77_std.argtypes = [C.c_char_p, vp]
    if hasattr(L, "ft8gpu_pack77"):                       # absent from older builds loaded by load_library_at
        L.ft8gpu_pack77.argtypes = [C.c_char_p, vp]
        L.ft8gpu_build_id.restype = C.c_char_p
    if hasattr(L, "ft8gpu_selftest_norm_math"):
        L.ft8gpu_selftest_norm_math.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.ft8gpu_overlap_reason.argtypes = [vp, C.c_char_p, C.c_size_t]
    if hasattr(L, "ft8gpu_selftest_quantiser"):           # absent from older builds loaded by load_library_at
        L.ft8gpu_selftest_quantiser.argtypes = [vp, vp, vp, vp, C.c_int32, vp]
    L.ft8gpu_encode.argtypes = [vp, vp]
    L.ft8gpu_encode.restype = None
    L.ft8gpu_synth_frames.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, C.c_uint64, vp]
    L.ft8gpu_synth_frames_at.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, vp]
    L.ft8gpu_set_debug_flags.argtypes = [vp, C.c_uint]
    if hasattr(L, "ft8gpu_selftest_bp_math"):             # absent from older builds loaded by load_library_at
        L.ft8gpu_selftest_bp_math.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.ft8gpu_decode_batch_multi.argtypes = [C.POINTER(vp), C.c_int, vp, C.c_int, vp, vp]
    L.ft8gpu_decode_batch_multi_dev.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp), C.POINTER(C.c_int), vp, vp]
    if hasattr(L, "ft8gpu_gather_spots"):
        L.ft8gpu_gather_spots.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.POINTER(vp), C.POINTER(vp)]
        L.ft8gpu_gather_shutdown.restype = None
    if hasattr(L, "ft8gpu_decode_messages"):              # absent from older builds loaded by load_library_at
        L.ft8gpu_decode_messages.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int]
        L.ft8gpu_collect_messages.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int]
        L.ft8gpu_noise_baseline.argtypes = [vp, vp, C.c_int, vp, C.c_int]
        L.ft8gpu_format_messages.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    if hasattr(L, "ft8gpu_decode_messages_passes"):       # absent from older builds loaded by load_library_at
        L.ft8gpu_decode_messages_passes.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int]
        L.ft8gpu_mask_messages.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int]
        L.ft8gpu_append_messages.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int]
    if hasattr(L, "ft8gpu_osd_candidates"):               # absent from older builds loaded by load_library_at
        L.ft8gpu_osd_candidates.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int]
        L.ft8gpu_decode_messages_deep.argtypes = [vp, vp, C.c_int, C.POINTER(DeepParams), vp, vp, vp, C.c_int]
    if hasattr(L, "ft8gpu_ap_candidates"):                # absent from older builds loaded by load_library_at
        L.ft8gpu_ap_candidates.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int]
        L.ft8gpu_ap_from_text.argtypes = [C.c_char_p, vp]
        L.ft8gpu_decode_messages_ap.argtypes = [vp, vp, C.c_int, C.POINTER(ApParams), vp, vp, vp, C.c_int]
    if hasattr(L, "ft8gpu_resolve_calls"):                # absent from older builds loaded by load_library_at
        L.ft8gpu_resolve_calls.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_uint32, vp, C.c_int]
        L.ft8gpu_decode_messages_resolved.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(ApParams), vp, C.c_uint32, vp, vp, vp, C.c_int]
        L.ft8gpu_callhash_reset.argtypes = [vp]
        L.ft8gpu_callhash_reset.restype = None
        L.ft8gpu_call_hash.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_uint32)]
        L.ft8gpu_callhash_insert.argtypes = [vp, C.c_char_p]
        L.ft8gpu_callhash_lookup.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, vp]
        L.ft8gpu_format_resolved.argtypes = [vp, vp, C.c_int32, vp, C.c_size_t]
    if hasattr(L, "ft8gpu_match_candidates"):             # absent from older builds loaded by load_library_at
        L.ft8gpu_match_candidates.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_uint32, C.c_int, vp, vp, C.c_int]
        L.ft8gpu_expect_update.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int]
        L.ft8gpu_decode_messages_expected.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(ExpectParams), vp, vp, vp, C.c_int]
        L.ft8gpu_expect_reset.argtypes = [vp]
        L.ft8gpu_expect_reset.restype = None
        L.ft8gpu_expect_insert.argtypes = [vp, vp, C.c_int]
        L.ft8gpu_expect_insert_text.argtypes = [vp, C.c_char_p]
    if hasattr(L, "ft8gpu_hint_candidates"):
        L.ft8gpu_hint_candidates.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.POINTER(HintParams), vp, vp, C.c_int]
        L.ft8gpu_hint_update.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int]
        L.ft8gpu_decode_messages_hinted.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(HintParams), vp, vp, vp, C.c_int]
        L.ft8gpu_hint_reset.argtypes = [vp]
        L.ft8gpu_hint_reset.restype = None
        L.ft8gpu_hint_insert.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_int]
        L.ft8gpu_hint_insert_text.argtypes = [vp, C.c_char_p, C.c_int]
        L.ft8gpu_hint_hypothesis.argtypes = [vp, vp]
    if hasattr(L, "ft8gpu_combine_candidates"):           # absent from older builds loaded by load_library_at
        L.ft8gpu_combine_candidates.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_uint32, C.c_int, vp, vp, C.c_int]
        L.ft8gpu_softmem_update.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int]
        L.ft8gpu_decode_messages_combined.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(CombineParams), vp, vp, vp, C.c_int]
        L.ft8gpu_softmem_reset.argtypes = [vp]
        L.ft8gpu_softmem_reset.restype = None
    if hasattr(L, "ft8gpu_demod_candidates"):             # absent from older builds loaded by load_library_at
        L.ft8gpu_demod_candidates.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.POINTER(DemodParams), vp, vp, C.c_int]
        L.ft8gpu_decode_messages_demod.argtypes = [vp, vp, C.c_int, C.POINTER(DemodParams), vp, vp, vp, C.c_int]
    if hasattr(L, "ft8gpu_demod_soft"):                   # absent from older builds loaded by load_library_at
        L.ft8gpu_demod_soft.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.POINTER(DemodParams), vp, vp, vp, C.c_int]
        L.ft8gpu_ap_soft_candidates.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int]
        L.ft8gpu_decode_messages_demod_ap.argtypes = [vp, vp, C.c_int, C.POINTER(DemodApParams), vp, vp, vp, C.c_int]
    if hasattr(L, "ft8gpu_refine_messages"):              # absent from older builds loaded by load_library_at
        L.ft8gpu_refine_messages.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.c_int]
        L.ft8gpu_decode_messages_refined.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int]
        L.ft8gpu_refined_estimate.argtypes = [vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.ft8gpu_format_messages_refined.argtypes = [vp, vp, C.c_int32, vp, C.c_size_t]
    if hasattr(L, "ft8gpu_subtract_messages"):
        L.ft8gpu_subtract_messages.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int]
        L.ft8gpu_decode_messages_subtracted.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int]
        L.ft8gpu_subtract_twiddles.argtypes = [vp]
        L.ft8gpu_subtract_twiddles.restype = None
    if hasattr(L, "ft8gpu_subtract_messages_shaped"):     # absent from older builds loaded by load_library_at
        L.ft8gpu_subtract_messages_shaped.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int]
        L.ft8gpu_decode_messages_subtracted_shaped.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int]
    if hasattr(L, "ft8gpu_audio_frames"):                 # absent from older builds loaded by load_library_at
        L.ft8gpu_audio_taps.argtypes = [vp]
        L.ft8gpu_audio_taps.restype = None
        L.ft8gpu_audio_mixer.argtypes = [vp]
        L.ft8gpu_audio_mixer.restype = None
        L.ft8gpu_audio_frames.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int]
        L.ft8gpu_decode_audio.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int]
        L.ft8gpu_read_wav.argtypes = [C.c_char_p, vp, C.c_int32, i32p]
    if hasattr(L, "ft8gpu_synth_gfsk_frames"):            # absent from older builds loaded by load_library_at
        L.ft8gpu_gfsk_pulse.argtypes = [C.c_int, vp]
        L.ft8gpu_gfsk_ramp.argtypes = [C.c_int, vp]
        L.ft8gpu_gfsk_twiddles.argtypes = [vp, vp]
        L.ft8gpu_gfsk_twiddles.restype = None
        L.ft8gpu_synth_gfsk_frames.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_float, vp, C.c_int]
        L.ft8gpu_synth_gfsk_audio.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_float, C.c_int,
                                              vp, C.c_int]
        L.ft8gpu_write_wav.argtypes = [C.c_char_p, vp, C.c_int32]
    if hasattr(L, "ft8gpu_synth_gfsk_frames_faded"):      # absent from older builds loaded by load_library_at
        L.ft8gpu_channel_taps.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_float, vp, vp]
        L.ft8gpu_channel_check.argtypes = [vp]
        L.ft8gpu_channel_clip.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp]
        L.ft8gpu_synth_gfsk_frames_faded.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_float, vp, C.c_int]
        L.ft8gpu_synth_gfsk_audio_faded.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_float,
                                                    C.c_int, vp, C.c_int]
    if hasattr(L, "ft8gpu_wide_frames"):                  # absent from older builds loaded by load_library_at
        for f in (L.ft8gpu_wide_mixer1, L.ft8gpu_wide_mixer2, L.ft8gpu_wide_taps):
            f.argtypes = [vp]
            f.restype = None
        L.ft8gpu_wide_frames.argtypes = [vp, vp, C.c_int, C.c_size_t, vp, C.c_int, vp, C.c_int, C.c_int]
        L.ft8gpu_decode_wide.argtypes = [vp, vp, C.c_int, C.c_size_t, vp, C.c_int, vp, vp, C.c_int]
    if hasattr(L, "ft8gpu_pcm_frames"):                   # absent from older builds loaded by load_library_at
        L.ft8gpu_pcm_decimation.argtypes = [C.c_int]
        L.ft8gpu_pcm_mixer1.argtypes = [C.c_int, vp]
        L.ft8gpu_pcm_mixer1.restype = None
        L.ft8gpu_pcm_taps_a.argtypes = [C.c_int, vp]
        for f in (L.ft8gpu_pcm_mixer2, L.ft8gpu_pcm_taps_b):
            f.argtypes = [vp]
            f.restype = None
        L.ft8gpu_pcm_frames.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int]
        L.ft8gpu_decode_pcm.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int]
        L.ft8gpu_read_wav_pcm.argtypes = [C.c_char_p, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), i32p]
    L.ft8gpu_rx_decimate.argtypes = [vp, vp, C.c_int, C.c_size_t, vp, C.c_int, C.c_int]
    if hasattr(L, "ft8gpu_rx_stream"):                    # absent from older builds loaded by load_library_at
        L.ft8gpu_rx_stream.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, vp, vp, C.c_int, C.c_int]
        L.ft8gpu_rx_state_reset.argtypes = [vp]
        L.ft8gpu_rx_state_reset.restype = None
    L.ft8gpu_pskreporter_datagrams.argtypes = [vp, vp, vp, C.c_int, C.POINTER(ReportInfo), vp, vp, vp, C.c_int]
    L.ft8gpu_format_spots.argtypes = [vp, C.c_int32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t]
    L.ft8gpu_dev_alloc.argtypes = [vp, C.c_size_t]
    L.ft8gpu_dev_alloc.restype = vp
    L.ft8gpu_dev_free.argtypes = [vp, vp]
    L.ft8gpu_dev_free.restype = None
    if hasattr(L, "ft8gpu_host_alloc"):                   # absent from older builds loaded by load_library_at
        L.ft8gpu_host_alloc.argtypes = [C.c_size_t]
        L.ft8gpu_host_alloc.restype = vp
        L.ft8gpu_host_free.argtypes = [vp]
        L.ft8gpu_host_free.restype = None
        L.ft8gpu_overlap_active.argtypes = [vp]
    L.ft8gpu_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.ft8gpu_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    L.initFFTW.restype = None
    L.freeFFTW.restype = None
    L.ft8_subsystem.argtypes = [vp, vp, C.c_uint32, vp, i32p]
    L.ft8_subsystem.restype = None
    L.ft8gpu_read_raw_iq.argtypes = [vp, vp, C.c_char_p]
    L.ft8gpu_read_raw_iq.restype = C.c_int32
    L.ft8gpu_read_c2.argtypes = [vp, vp, C.c_char_p, C.POINTER(C.c_double)]
    L.ft8gpu_read_c2.restype = C.c_int32
    L.ft8gpu_write_raw_iq.argtypes = [vp, vp, C.c_char_p]
    L.ft8gpu_write_raw_iq.restype = C.c_int32
    return L


def _check(rc, lib=None):
    if rc != 0:
        raise Ft8GpuError((lib or load_library()).ft8gpu_last_error().decode(errors="replace"))


def _ptr(a):
    """host numpy array or device pointer (int / torch tensor) -> integer address"""
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return int(a)


def pack77_std(msg):
    out = np.zeros(10, np.uint8)
    rc = load_library().ft8gpu_pack77_std(msg.encode(), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"cannot pack {msg!r} as a standard FT8 message")
    return out


def pack77(msg):
    """ft8gpu_pack77: any message type the packer knows (type 1 / 2 with grid, report, RRR / RR73 / 73, /R /P, CQ modifiers,
    <hashed> calls; type 4; telemetry; free text) -> 10 bytes"""
    out = np.zeros(10, np.uint8)
    rc = load_library().ft8gpu_pack77(msg.encode(), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"cannot pack {msg!r} as an FT8 message")
    return out


def ap_from_text(pattern):
    """ft8gpu_ap_from_text: a type 1 message with `?` for the unknown tokens ("CQ ? ?", "CQ DX ? ?", "K1ABC W9XYZ ?") -> one
    AP_HYP_DTYPE record"""
    out = np.zeros(1, AP_HYP_DTYPE)
    rc = load_library().ft8gpu_ap_from_text(pattern.encode(), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"{pattern!r} is no a-priori pattern of a standard message")
    return out[0]


def call_hash(call, bits=22):
    """ft8gpu_call_hash: the bits-bit hash of a call of 1 .. 11 characters of " 0-9A-Z/" """
    out = C.c_uint32(0)
    if load_library().ft8gpu_call_hash(call.encode(), int(bits), C.byref(out)) != 0:
        raise ValueError(f"{call!r} is no call the hash table takes, or bits {bits} is outside 1 .. 32")
    return out.value


def callhash_state(n=1):
    """n reset call hash tables (CALLHASH_STATE_DTYPE [n], all zero: what ft8gpu_callhash_reset leaves)"""
    return np.zeros(n, CALLHASH_STATE_DTYPE)


def _one_state(state):
    assert isinstance(state, np.ndarray) and state.dtype == CALLHASH_STATE_DTYPE and state.size == 1 and state.flags["C_CONTIGUOUS"]
    return state


def callhash_reset(state):
    """ft8gpu_callhash_reset on one state (a CALLHASH_STATE_DTYPE array of one element, in place)"""
    load_library().ft8gpu_callhash_reset(_one_state(state).ctypes.data)


def callhash_insert(state, call):
    """ft8gpu_callhash_insert: e.g. the operator's own call, before the first slot (in place)"""
    if load_library().ft8gpu_callhash_insert(_one_state(state).ctypes.data, call.encode()) != 0:
        raise ValueError(f"{call!r} is no call the hash table takes")


def callhash_lookup(state, bits, hash_value, max_age=0):
    """ft8gpu_callhash_lookup: the call a 12- or 22-bit hash resolves to at the state's slot, or None"""
    buf = C.create_string_buffer(12)
    rc = load_library().ft8gpu_callhash_lookup(_one_state(state).ctypes.data, int(bits), int(hash_value), int(max_age), buf)
    if rc < 0:
        raise ValueError(f"bits {bits} / hash {hash_value}: not a 12- or 22-bit hash")
    return buf.value.decode() if rc else None


def expect_state(n=1):
    """n reset tables of expected messages (EXPECT_STATE_DTYPE [n], all zero: what ft8gpu_expect_reset leaves)"""
    return np.zeros(n, EXPECT_STATE_DTYPE)


def softmem_state(n=1):
    """n reset soft-bit memories (SOFTMEM_STATE_DTYPE [n], all zero: what ft8gpu_softmem_reset leaves)"""
    return np.zeros(n, SOFTMEM_STATE_DTYPE)


def softmem_reset(state):
    """ft8gpu_softmem_reset on one state (a SOFTMEM_STATE_DTYPE array of one element, in place)"""
    assert isinstance(state, np.ndarray) and state.dtype == SOFTMEM_STATE_DTYPE and state.size == 1 and state.flags["C_CONTIGUOUS"]
    load_library().ft8gpu_softmem_reset(state.ctypes.data)


def _one_expect_state(state):
    assert isinstance(state, np.ndarray) and state.dtype == EXPECT_STATE_DTYPE and state.size == 1 and state.flags["C_CONTIGUOUS"]
    return state


def expect_reset(state):
    """ft8gpu_expect_reset on one state (an EXPECT_STATE_DTYPE array of one element, in place)"""
    load_library().ft8gpu_expect_reset(_one_expect_state(state).ctypes.data)


def expect_insert(state, payload, kind=0):
    """ft8gpu_expect_insert: insert(payload, kind) of the update rule at the state's slot (in place); payload: 10 bytes"""
    payload = np.ascontiguousarray(payload, np.uint8)
    assert payload.shape == (10,)
    if load_library().ft8gpu_expect_insert(_one_expect_state(state).ctypes.data, payload.ctypes.data, int(kind)) != 0:
        raise ValueError(f"kind {kind} is neither 0 (heard) nor 1 (derived)")


def expect_insert_text(state, text):
    """ft8gpu_expect_insert_text: the message as ft8gpu_pack77 packs it, as a heard entry (in place)"""
    if load_library().ft8gpu_expect_insert_text(_one_expect_state(state).ctypes.data, text.encode()) != 0:
        raise ValueError(f"cannot pack {text!r} as an FT8 message")


def hint_state(n=1):
    """n reset tables of call hints (HINT_STATE_DTYPE [n], all zero: what ft8gpu_hint_reset leaves)"""
    return np.zeros(n, HINT_STATE_DTYPE)


def _one_hint_state(state):
    assert isinstance(state, np.ndarray) and state.dtype == HINT_STATE_DTYPE and state.size == 1 and state.flags["C_CONTIGUOUS"]
    return state


def hint_reset(state):
    """ft8gpu_hint_reset on one state (a HINT_STATE_DTYPE array of one element, in place)"""
    load_library().ft8gpu_hint_reset(_one_hint_state(state).ctypes.data)


def hint_insert(state, kind, a, b, phase):
    """ft8gpu_hint_insert: insert(kind, a, b, phase) of the update rule at the state's slot (in place)"""
    if load_library().ft8gpu_hint_insert(_one_hint_state(state).ctypes.data, int(kind), int(a) & 0xFFFFFFFF, int(b) & 0xFFFFFFFF,
                                         int(phase)) != 0:
        raise ValueError(f"kind {kind} is not 1, 2 or 3")


def hint_insert_text(state, pattern, phase):
    """ft8gpu_hint_insert_text: "K1ABC ? ?", "? W9XYZ ?" or "K1ABC W9XYZ ?" as an entry expected at slot parity `phase`"""
    if load_library().ft8gpu_hint_insert_text(_one_hint_state(state).ctypes.data, pattern.encode(), int(phase)) != 0:
        raise ValueError(f"not a call hint pattern: {pattern!r}")


def hint_hypothesis(entry):
    """ft8gpu_hint_hypothesis: the AP_HYP_DTYPE record of one HINT_ENTRY_DTYPE entry, or None if its kind is not 1, 2 or 3"""
    e = np.array(entry, HINT_ENTRY_DTYPE, ndmin=1)
    out = np.zeros(1, AP_HYP_DTYPE)
    return out[0] if load_library().ft8gpu_hint_hypothesis(e.ctypes.data, out.ctypes.data) == 0 else None


def format_resolved(msgs, resolved, n):
    """ft8gpu_format_resolved: the lines of format_messages with the resolved text"""
    L = load_library()
    msgs, resolved = np.ascontiguousarray(msgs), np.ascontiguousarray(resolved)
    assert msgs.dtype == MESSAGE_DTYPE and resolved.dtype == RESOLVED_DTYPE
    n = int(min(n, msgs.size, resolved.size))
    need = L.ft8gpu_format_resolved(msgs.ctypes.data, resolved.ctypes.data, n, None, 0)
    if need < 0:
        raise Ft8GpuError("ft8gpu_format_resolved failed")
    buf = C.create_string_buffer(need + 1)
    L.ft8gpu_format_resolved(msgs.ctypes.data, resolved.ctypes.data, n, buf, len(buf))
    return buf.value.decode()


def _ap_hyps(hyps):
    """patterns (str) or AP_HYP_DTYPE records -> a contiguous AP_HYP_DTYPE array"""
    hyps = [hyps] if isinstance(hyps, (str, np.void)) else hyps
    out = np.zeros(len(hyps), AP_HYP_DTYPE)
    for k, h in enumerate(hyps):
        out[k] = ap_from_text(h) if isinstance(h, str) else h
    return out


def _ap_params(passes, hyps, ap_max_hard_errors, osd_order, osd_max_hard_errors):
    hyps = _ap_hyps(hyps)
    p = ApParams(int(passes), len(hyps), int(ap_max_hard_errors), int(osd_order), int(osd_max_hard_errors))
    C.memmove(C.addressof(p.hyps), hyps.ctypes.data, min(hyps.nbytes, C.sizeof(p.hyps)))
    return p


def encode(payload):
    payload = np.ascontiguousarray(payload, np.uint8)
    tones = np.zeros(79, np.uint8)
    load_library().ft8gpu_encode(payload.ctypes.data, tones.ctypes.data)
    return tones


class Decoder:
    """One GPU decoder context (ft8gpu_ctx).  Host arrays are numpy; device arrays are anything
    with ``data_ptr()`` (torch tensors) or raw integer addresses."""

    def __init__(self, device=0, max_frames=64, min_score=10, max_candidates=120, ldpc_iters=20, lib=None):
        self.lib = lib or load_library()
        self.params = Params(min_score, max_candidates, ldpc_iters)
        self.max_frames = max_frames
        h = C.c_void_p()
        self._ck(self.lib.ft8gpu_create(C.byref(h), device, max_frames, C.byref(self.params)))
        self.h = h

    def _ck(self, rc):
        _check(rc, self.lib)            # the error text lives in the library that failed (the A/B build is a second library)

    def close(self):
        if getattr(self, "h", None):
            self.lib.ft8gpu_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def max_candidates(self):
        return self.params.max_candidates

    def set_params(self, min_score=None, max_candidates=None, ldpc_iters=None):
        p = Params(self.params.min_score if min_score is None else min_score,
                   self.params.max_candidates if max_candidates is None else max_candidates,
                   self.params.ldpc_iters if ldpc_iters is None else ldpc_iters)
        self._ck(self.lib.ft8gpu_set_params(self.h, C.byref(p)))
        self.params = p

    def set_stream(self, stream_handle):
        """None: the context creates its own stream.  An integer is a hipStream_t; 0 (what torch reports for its
        default stream) is passed as hipStreamLegacy, the explicit name of the null stream."""
        if stream_handle is None:
            h = None
        else:
            h = int(stream_handle) or STREAM_LEGACY
        self._ck(self.lib.ft8gpu_set_stream(self.h, C.c_void_p(h)))

    def stream_handle(self):
        """the hipStream_t of the context as an integer (e.g. for torch.cuda.ExternalStream)"""
        return int(self.lib.ft8gpu_get_stream(self.h) or 0)

    def set_debug_flags(self, flags):
        self._ck(self.lib.ft8gpu_set_debug_flags(self.h, int(flags)))

    def overlap_active(self):
        """True: the two-part pipeline with the serial kernels on side streams is in use for large batches (the
        context has SEEN its streams run kernels concurrently); False: plain pipeline (overlap_reason() says why)"""
        return bool(self.lib.ft8gpu_overlap_active(self.h))

    def overlap_reason(self):
        buf = C.create_string_buffer(256)
        self._ck(self.lib.ft8gpu_overlap_reason(self.h, buf, len(buf)))
        return buf.value.decode()

    def selftest_bp_math(self):
        """exhaustive (2^32 inputs) comparison of the BP kernel's short division chains with the IEEE quotient"""
        out = (C.c_uint64 * 7)()
        self._ck(self.lib.ft8gpu_selftest_bp_math(self.h, out))
        keys = ("tanh_inputs", "tanh_mismatch", "atanh_inputs", "atanh_mismatch", "pair_mismatch", "tanh_max_bits", "first_bad")
        d = dict(zip(keys, [int(v) for v in out]))
        d["tanh_max"] = float(np.array([d["tanh_max_bits"]], np.uint32).view(np.float32)[0])
        return d

    def selftest_norm_math(self):
        """sqrtf(24.0f / v), the LLR scale factor, against exact arithmetic for every float v in [2^-60, 2^60]"""
        out = (C.c_uint64 * 7)()
        self._ck(self.lib.ft8gpu_selftest_norm_math(self.h, out))
        return dict(zip(("inputs", "div_bad", "sqrt_bad", "compose_bad", "first_bad", "rational_inputs", "rational_div_bad"), [int(v) for v in out]))

    def selftest_quantiser(self, cap=4096):
        """the waterfall kernel's dB quantiser on every float (0 .. +inf and every NaN) with this context's uploaded thresholds:
        its step function (steps_bits[k] = k-th bit pattern b with q(b) != q(b - 1), steps_val[k] = q(b); n_steps is the true
        count, also beyond cap), q(0), the counts the proof rests on, and qthr[0..255] as they lie on the device"""
        out = np.zeros(7, np.uint64)
        bits, val, thr = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(256, np.float32)
        self._ck(self.lib.ft8gpu_selftest_quantiser(self.h, out.ctypes.data, bits.ctypes.data, val.ctypes.data, cap, thr.ctypes.data))
        d = dict(zip(("n_steps", "q0", "nan_nonzero", "disagree", "from_guess", "from_guess_plus_1", "first_bad"), [int(v) for v in out]))
        n = min(d["n_steps"], cap, 4096)
        d.update(steps_bits=bits[:n], steps_val=val[:n], qthr=thr)
        return d

    def enable_timing(self, on=True):
        self._ck(self.lib.ft8gpu_enable_timing(self.h, int(on)))

    def timings(self):
        """mean per-stage milliseconds over the runs recorded since enable_timing(True)"""
        t, n = Timings(), C.c_int32(0)
        self._ck(self.lib.ft8gpu_get_timings(self.h, C.byref(t), C.byref(n)))
        d = {k: getattr(t, k) for k, _ in Timings._fields_}
        d["runs"] = n.value
        return d

    def synchronize(self):
        self._ck(self.lib.ft8gpu_synchronize(self.h))

    # ---- host (numpy) API ------------------------------------------------------------------
    def decode_batch(self, iq, decodes=None):
        iq = np.ascontiguousarray(iq, np.float32)
        B = iq.shape[0]
        assert iq.shape[1:] == (2, NSAMPLES)
        if decodes is None:
            decodes = np.zeros((B, MAX_MESSAGES), RESULT_DTYPE)
        n = np.zeros(B, np.int32)
        self._ck(self.lib.ft8gpu_decode_batch(self.h, iq.ctypes.data, B, decodes.ctypes.data, n.ctypes.data, HOST_PTRS))
        return decodes, n

    def waterfall(self, iq):
        iq = np.ascontiguousarray(iq, np.float32)
        B = iq.shape[0]
        assert iq.shape[1:] == (2, NSAMPLES)
        mag = np.zeros((B, MAG_ARRAY), np.uint8)
        self._ck(self.lib.ft8gpu_waterfall(self.h, iq.ctypes.data, B, mag.ctypes.data, HOST_PTRS))
        return mag

    def find_sync(self, mag):
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        cands = np.zeros((B, self.max_candidates), CAND_DTYPE)
        counts = np.zeros(B, np.int32)
        self._ck(self.lib.ft8gpu_find_sync(self.h, mag.ctypes.data, B, cands.ctypes.data, counts.ctypes.data, HOST_PTRS))
        return cands, counts

    def score_map(self, mag):
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        s = np.zeros((B, 2, 2, 36, 249), np.int16)
        self._ck(self.lib.ft8gpu_score_map(self.h, mag.ctypes.data, B, s.ctypes.data, HOST_PTRS))
        return s

    def decode_candidates(self, mag, cands, counts):
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        cands = np.ascontiguousarray(cands)
        counts = np.ascontiguousarray(counts, np.int32)
        assert cands.shape == (B, self.max_candidates) and cands.dtype == CAND_DTYPE
        st = np.zeros((B, self.max_candidates), STATUS_DTYPE)
        self._ck(self.lib.ft8gpu_decode_candidates(self.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data,
                                                 B, st.ctypes.data, HOST_PTRS))
        return st

    def collect_spots(self, cands, counts, status, decodes=None):
        cands = np.ascontiguousarray(cands)
        counts = np.ascontiguousarray(counts, np.int32)
        status = np.ascontiguousarray(status)
        B = counts.shape[0]
        if decodes is None:
            decodes = np.zeros((B, MAX_MESSAGES), RESULT_DTYPE)
        n = np.zeros(B, np.int32)
        self._ck(self.lib.ft8gpu_collect_spots(self.h, cands.ctypes.data, counts.ctypes.data, status.ctypes.data, B,
                                             decodes.ctypes.data, n.ctypes.data, HOST_PTRS))
        return decodes, n

    def decode_messages(self, iq, msgs=None):
        """every unique message of every frame -> (msgs [B][50] MESSAGE_DTYPE, n_msgs [B]); slots past n_msgs[f] keep
        what `msgs` held (zeros when None)"""
        iq = np.ascontiguousarray(iq, np.float32)
        B = iq.shape[0]
        assert iq.shape[1:] == (2, NSAMPLES)
        if msgs is None:
            msgs = np.zeros((B, MAX_MESSAGES), MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros(B, np.int32)
        self._ck(self.lib.ft8gpu_decode_messages(self.h, iq.ctypes.data, B, msgs.ctypes.data, n.ctypes.data, HOST_PTRS))
        return msgs, n

    def collect_messages(self, mag, cands, counts, status, msgs=None):
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        cands = np.ascontiguousarray(cands)
        counts = np.ascontiguousarray(counts, np.int32)
        status = np.ascontiguousarray(status)
        B = counts.shape[0]
        assert mag.shape[0] == B and cands.shape == (B, self.max_candidates) and status.shape == (B, self.max_candidates)
        if msgs is None:
            msgs = np.zeros((B, MAX_MESSAGES), MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros(B, np.int32)
        self._ck(self.lib.ft8gpu_collect_messages(self.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status.ctypes.data,
                                                B, msgs.ctypes.data, n.ctypes.data, HOST_PTRS))
        return msgs, n

    def noise_baseline(self, mag):
        """the per-frame noise floor of the SNR estimate: uint8 [B][2][256], the 47th smallest of each column"""
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        base = np.zeros((B, 2, 256), np.uint8)
        self._ck(self.lib.ft8gpu_noise_baseline(self.h, mag.ctypes.data, B, base.ctypes.data, HOST_PTRS))
        return base

    def decode_messages_passes(self, iq, passes=2, msgs=None):
        """multi-pass decoding (ft8gpu_decode_messages_passes) -> (msgs [B][50] MESSAGE_DTYPE, n_msgs [B],
        n_by_pass [B][passes], the count after each pass); slots past n_msgs[f] keep what `msgs` held (zeros when None)"""
        iq = np.ascontiguousarray(iq, np.float32)
        B = iq.shape[0]
        assert iq.shape[1:] == (2, NSAMPLES)
        if msgs is None:
            msgs = np.zeros((B, MAX_MESSAGES), MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros(B, np.int32)
        nbp = np.zeros((B, max(int(passes), 1)), np.int32)
        self._ck(self.lib.ft8gpu_decode_messages_passes(self.h, iq.ctypes.data, B, int(passes), msgs.ctypes.data, n.ctypes.data,
                                                      nbp.ctypes.data, HOST_PTRS))
        return msgs, n, nbp

    def mask_messages(self, mag, base, msgs, first, n_msgs):
        """ft8gpu_mask_messages: mag [B][94208] with the cells of records [first[f], n_msgs[f]) set to the baseline"""
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        base = np.ascontiguousarray(base, np.uint8)
        msgs = np.ascontiguousarray(msgs)
        first = np.ascontiguousarray(first, np.int32)
        n_msgs = np.ascontiguousarray(n_msgs, np.int32)
        assert base.size == B * 512 and msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES)
        assert first.shape == (B,) and n_msgs.shape == (B,)
        out = np.zeros((B, MAG_ARRAY), np.uint8)
        self._ck(self.lib.ft8gpu_mask_messages(self.h, mag.ctypes.data, base.ctypes.data, msgs.ctypes.data, first.ctypes.data,
                                             n_msgs.ctypes.data, B, out.ctypes.data, HOST_PTRS))
        return out

    def append_messages(self, mag, base, cands, counts, status, msgs, n_msgs):
        """ft8gpu_append_messages: the pass's new messages appended behind the records so far -> (msgs, n_msgs), new arrays"""
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        base = np.ascontiguousarray(base, np.uint8)
        cands = np.ascontiguousarray(cands)
        counts = np.ascontiguousarray(counts, np.int32)
        status = np.ascontiguousarray(status)
        assert base.size == B * 512 and cands.shape == (B, self.max_candidates) and status.shape == (B, self.max_candidates)
        assert counts.shape == (B,) and cands.dtype == CAND_DTYPE and status.dtype == STATUS_DTYPE
        msgs = np.array(msgs, dtype=MESSAGE_DTYPE, copy=True, order="C")
        n = np.array(n_msgs, dtype=np.int32, copy=True, order="C")
        assert msgs.shape == (B, MAX_MESSAGES) and n.shape == (B,)
        self._ck(self.lib.ft8gpu_append_messages(self.h, mag.ctypes.data, base.ctypes.data, cands.ctypes.data, counts.ctypes.data,
                                               status.ctypes.data, B, msgs.ctypes.data, n.ctypes.data, HOST_PTRS))
        return msgs, n

    def _cand_arrays(self, B, cands, counts, status_in, status_out, info, info_dtype):
        """the arrays every *_candidates method shares, shaped for B frames: cands, counts, status_in as bytes, and new
        status_out (bytes) and info arrays that start from what the caller handed in (zeros when None)"""
        cands = np.ascontiguousarray(cands)
        counts = np.ascontiguousarray(counts, np.int32)
        status_in = np.ascontiguousarray(status_in).view(np.uint8).reshape(B, self.max_candidates, 48)
        assert cands.shape == (B, self.max_candidates) and cands.dtype == CAND_DTYPE and counts.shape == (B,)
        out = np.zeros((B, self.max_candidates, 48), np.uint8) if status_out is None else \
            np.array(status_out, copy=True, order="C").view(np.uint8).reshape(B, self.max_candidates, 48)
        inf = np.zeros((B, self.max_candidates), info_dtype) if info is None else \
            np.array(info, copy=True, order="C").view(info_dtype).reshape(B, self.max_candidates)
        return cands, counts, status_in, out, inf

    def osd_candidates(self, mag, cands, counts, status_in, order=1, max_hard_errors=OSD_MAX_HARD_ERRORS, status_out=None, info=None):
        """ft8gpu_osd_candidates -> (status_out [B][cap] STATUS_DTYPE, info [B][cap] OSD_INFO_DTYPE), new arrays; records at and
        behind counts[f] keep what status_out / info held (zeros when None)"""
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        cands, counts, status_in, out, inf = self._cand_arrays(B, cands, counts, status_in, status_out, info, OSD_INFO_DTYPE)
        self._ck(self.lib.ft8gpu_osd_candidates(self.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status_in.ctypes.data,
                                              B, int(order), int(max_hard_errors), out.ctypes.data, inf.ctypes.data, HOST_PTRS))
        return out.view(STATUS_DTYPE).reshape(B, self.max_candidates), inf

    def decode_messages_deep(self, iq, passes=1, osd_order=1, osd_max_hard_errors=OSD_MAX_HARD_ERRORS, msgs=None):
        """ft8gpu_decode_messages_deep -> (msgs [B][50] MESSAGE_DTYPE, n_msgs [B], n_by_stage [B][passes][2]: the count after BP
        and after OSD of each pass); slots past n_msgs[f] keep what `msgs` held (zeros when None)"""
        iq = np.ascontiguousarray(iq, np.float32)
        B = iq.shape[0]
        assert iq.shape[1:] == (2, NSAMPLES)
        if msgs is None:
            msgs = np.zeros((B, MAX_MESSAGES), MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros(B, np.int32)
        nbs = np.zeros((B, max(int(passes), 1), 2), np.int32)
        p = DeepParams(int(passes), int(osd_order), int(osd_max_hard_errors))
        self._ck(self.lib.ft8gpu_decode_messages_deep(self.h, iq.ctypes.data, B, C.byref(p), msgs.ctypes.data, n.ctypes.data,
                                                    nbs.ctypes.data, HOST_PTRS))
        return msgs, n, nbs

    def ap_candidates(self, mag, cands, counts, status_in, hyps=("CQ ? ?",), max_hard_errors=AP_MAX_HARD_ERRORS, status_out=None,
                      info=None):
        """ft8gpu_ap_candidates -> (status_out [B][cap] STATUS_DTYPE, info [B][cap] AP_INFO_DTYPE), new arrays; records at and
        behind counts[f] keep what status_out / info held (zeros when None).  hyps: patterns or AP_HYP_DTYPE records"""
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        cands, counts, status_in, out, inf = self._cand_arrays(B, cands, counts, status_in, status_out, info, AP_INFO_DTYPE)
        hyps = _ap_hyps(hyps)
        self._ck(self.lib.ft8gpu_ap_candidates(self.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status_in.ctypes.data,
                                               B, hyps.ctypes.data, len(hyps), int(max_hard_errors), out.ctypes.data, inf.ctypes.data,
                                               HOST_PTRS))
        return out.view(STATUS_DTYPE).reshape(B, self.max_candidates), inf

    def decode_messages_ap(self, iq, passes=1, hyps=("CQ ? ?",), ap_max_hard_errors=AP_MAX_HARD_ERRORS, osd_order=-1,
                           osd_max_hard_errors=OSD_MAX_HARD_ERRORS, msgs=None):
        """ft8gpu_decode_messages_ap -> (msgs [B][50] MESSAGE_DTYPE, n_msgs [B], n_by_stage [B][passes][3]: the count after BP,
        after AP and after OSD of each pass); slots past n_msgs[f] keep what `msgs` held (zeros when None).  hyps = (): no AP"""
        iq = np.ascontiguousarray(iq, np.float32)
        B = iq.shape[0]
        assert iq.shape[1:] == (2, NSAMPLES)
        if msgs is None:
            msgs = np.zeros((B, MAX_MESSAGES), MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros(B, np.int32)
        nbs = np.zeros((B, max(int(passes), 1), 3), np.int32)
        p = _ap_params(passes, hyps, ap_max_hard_errors, osd_order, osd_max_hard_errors)
        self._ck(self.lib.ft8gpu_decode_messages_ap(self.h, iq.ctypes.data, B, C.byref(p), msgs.ctypes.data, n.ctypes.data,
                                                    nbs.ctypes.data, HOST_PTRS))
        return msgs, n, nbs

    def resolve_calls(self, msgs, n_msgs, state=None, max_age=0, resolved=None):
        """ft8gpu_resolve_calls.  msgs: MESSAGE_DTYPE [nstreams][nslots][50], n_msgs: int32 [nstreams][nslots]; state:
        CALLHASH_STATE_DTYPE [nstreams] as a previous call returned it, or None for reset tables (the caller's array stays as it
        is); resolved: an array to write into (records at and above a frame's count keep its bytes; zeros when None)
        -> (resolved RESOLVED_DTYPE [nstreams][nslots][50], the exit state [nstreams])"""
        msgs = np.ascontiguousarray(msgs)
        n_msgs = np.ascontiguousarray(n_msgs, np.int32)
        nstreams, nslots = n_msgs.shape
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (nstreams, nslots, MAX_MESSAGES)
        state = np.zeros(nstreams, CALLHASH_STATE_DTYPE) if state is None else np.array(state, CALLHASH_STATE_DTYPE, copy=True, ndmin=1)
        assert state.shape == (nstreams,)
        if resolved is None:
            resolved = np.zeros((nstreams, nslots, MAX_MESSAGES), RESOLVED_DTYPE)
        assert resolved.dtype == RESOLVED_DTYPE and resolved.shape == (nstreams, nslots, MAX_MESSAGES) and resolved.flags["C_CONTIGUOUS"]
        self._ck(self.lib.ft8gpu_resolve_calls(self.h, msgs.ctypes.data, n_msgs.ctypes.data, nstreams, nslots, state.ctypes.data,
                                               int(max_age), resolved.ctypes.data, HOST_PTRS))
        return resolved, state

    def resolve_calls_dev(self, msgs_dev, n_msgs_dev, nstreams, nslots, state_dev, max_age, resolved_dev):
        """all arrays in HBM, 16-byte aligned: msgs [nstreams][nslots][50] 64-byte records, n_msgs [nstreams][nslots] int32,
        state [nstreams] 81 936-byte tables (updated in place), resolved [nstreams][nslots][50] 48-byte records"""
        self._ck(self.lib.ft8gpu_resolve_calls(self.h, _ptr(msgs_dev), _ptr(n_msgs_dev), nstreams, nslots, _ptr(state_dev),
                                               int(max_age), _ptr(resolved_dev), DEVICE_PTRS))

    def decode_messages_resolved(self, iq, state=None, max_age=0, ap=None, msgs=None, resolved=None):
        """ft8gpu_decode_messages_resolved.  iq: float32 [nstreams][nslots][2][48000]; ap: None (ft8gpu_decode_messages) or the
        keyword arguments of decode_messages_ap as a dict (passes, hyps, ap_max_hard_errors, osd_order, osd_max_hard_errors)
        -> (msgs [nstreams][nslots][50], n_msgs [nstreams][nslots], resolved [nstreams][nslots][50], the exit state [nstreams])"""
        iq = np.ascontiguousarray(iq, np.float32)
        nstreams, nslots = iq.shape[:2]
        assert iq.shape[2:] == (2, NSAMPLES)
        state = np.zeros(nstreams, CALLHASH_STATE_DTYPE) if state is None else np.array(state, CALLHASH_STATE_DTYPE, copy=True, ndmin=1)
        assert state.shape == (nstreams,)
        if msgs is None:
            msgs = np.zeros((nstreams, nslots, MAX_MESSAGES), MESSAGE_DTYPE)
        if resolved is None:
            resolved = np.zeros((nstreams, nslots, MAX_MESSAGES), RESOLVED_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (nstreams, nslots, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        assert resolved.dtype == RESOLVED_DTYPE and resolved.shape == (nstreams, nslots, MAX_MESSAGES) and resolved.flags["C_CONTIGUOUS"]
        n = np.zeros((nstreams, nslots), np.int32)
        p = None if ap is None else C.byref(_ap_params(ap.get("passes", 1), ap.get("hyps", ("CQ ? ?",)),
                                                       ap.get("ap_max_hard_errors", AP_MAX_HARD_ERRORS), ap.get("osd_order", -1),
                                                       ap.get("osd_max_hard_errors", OSD_MAX_HARD_ERRORS)))
        self._ck(self.lib.ft8gpu_decode_messages_resolved(self.h, iq.ctypes.data, nstreams, nslots, p, state.ctypes.data, int(max_age),
                                                          msgs.ctypes.data, n.ctypes.data, resolved.ctypes.data, HOST_PTRS))
        return msgs, n, resolved, state

    def decode_messages_resolved_dev(self, iq_dev, nstreams, nslots, state_dev, max_age, msgs_dev, n_msgs_dev, resolved_dev, ap=None):
        """the same with every array in HBM; ap as in decode_messages_resolved"""
        p = None if ap is None else C.byref(_ap_params(ap.get("passes", 1), ap.get("hyps", ("CQ ? ?",)),
                                                       ap.get("ap_max_hard_errors", AP_MAX_HARD_ERRORS), ap.get("osd_order", -1),
                                                       ap.get("osd_max_hard_errors", OSD_MAX_HARD_ERRORS)))
        self._ck(self.lib.ft8gpu_decode_messages_resolved(self.h, _ptr(iq_dev), nstreams, nslots, p, _ptr(state_dev), int(max_age),
                                                          _ptr(msgs_dev), _ptr(n_msgs_dev), _ptr(resolved_dev), DEVICE_PTRS))

    def match_candidates(self, mag, cands, counts, status_in, states, max_age=0, max_hard_errors=MATCH_MAX_HARD_ERRORS,
                         status_out=None, info=None):
        """ft8gpu_match_candidates.  states: EXPECT_STATE_DTYPE [B], the table of the receiver each frame belongs to (read only)
        -> (status_out [B][cap] STATUS_DTYPE, info [B][cap] MATCH_INFO_DTYPE), new arrays; records at and behind counts[f] keep
        what status_out / info held (zeros when None)"""
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        cands, counts, status_in, out, inf = self._cand_arrays(B, cands, counts, status_in, status_out, info, MATCH_INFO_DTYPE)
        states = np.ascontiguousarray(states)
        assert states.dtype == EXPECT_STATE_DTYPE and states.shape == (B,)
        self._ck(self.lib.ft8gpu_match_candidates(self.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status_in.ctypes.data,
                                                  B, states.ctypes.data, int(max_age), int(max_hard_errors), out.ctypes.data,
                                                  inf.ctypes.data, HOST_PTRS))
        return out.view(STATUS_DTYPE).reshape(B, self.max_candidates), inf

    def match_candidates_dev(self, mag_dev, cands_dev, counts_dev, status_in_dev, nframes, states_dev, max_age, max_hard_errors,
                             status_out_dev, info_dev):
        """status_out_dev may be status_in_dev; states_dev: [nframes] 8208-byte tables, 16-byte aligned; info_dev: 8-byte records"""
        self._ck(self.lib.ft8gpu_match_candidates(self.h, _ptr(mag_dev), _ptr(cands_dev), _ptr(counts_dev), _ptr(status_in_dev), nframes,
                                                  _ptr(states_dev), int(max_age), int(max_hard_errors), _ptr(status_out_dev),
                                                  _ptr(info_dev), DEVICE_PTRS))

    def expect_update(self, msgs, n_msgs, state=None, derive=True):
        """ft8gpu_expect_update.  msgs: MESSAGE_DTYPE [nstreams][nslots][50], n_msgs: int32 [nstreams][nslots]; state:
        EXPECT_STATE_DTYPE [nstreams] as a previous call returned it, or None for reset tables (the caller's array stays as it
        is) -> the exit state [nstreams]"""
        msgs = np.ascontiguousarray(msgs)
        n_msgs = np.ascontiguousarray(n_msgs, np.int32)
        nstreams, nslots = n_msgs.shape
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (nstreams, nslots, MAX_MESSAGES)
        state = np.zeros(nstreams, EXPECT_STATE_DTYPE) if state is None else np.array(state, EXPECT_STATE_DTYPE, copy=True, ndmin=1)
        assert state.shape == (nstreams,)
        self._ck(self.lib.ft8gpu_expect_update(self.h, msgs.ctypes.data, n_msgs.ctypes.data, nstreams, nslots, state.ctypes.data,
                                               int(bool(derive)), HOST_PTRS))
        return state

    def expect_update_dev(self, msgs_dev, n_msgs_dev, nstreams, nslots, state_dev, derive=True):
        """all arrays in HBM; msgs and state 16-byte aligned; the states are updated in place"""
        self._ck(self.lib.ft8gpu_expect_update(self.h, _ptr(msgs_dev), _ptr(n_msgs_dev), nstreams, nslots, _ptr(state_dev),
                                               int(bool(derive)), DEVICE_PTRS))

    def decode_messages_expected(self, iq, state=None, max_hard_errors=MATCH_MAX_HARD_ERRORS, max_age=0, derive=True, msgs=None):
        """ft8gpu_decode_messages_expected.  iq: float32 [nstreams][nslots][2][48000]; state as in expect_update
        -> (msgs [nstreams][nslots][50], n_msgs [nstreams][nslots], n_by_stage [nstreams][nslots][2]: the count after BP and
        after matching, the exit state [nstreams]); pad[2] of a record gained by matching is 1"""
        iq = np.ascontiguousarray(iq, np.float32)
        nstreams, nslots = iq.shape[:2]
        assert iq.shape[2:] == (2, NSAMPLES)
        state = np.zeros(nstreams, EXPECT_STATE_DTYPE) if state is None else np.array(state, EXPECT_STATE_DTYPE, copy=True, ndmin=1)
        assert state.shape == (nstreams,)
        if msgs is None:
            msgs = np.zeros((nstreams, nslots, MAX_MESSAGES), MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (nstreams, nslots, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros((nstreams, nslots), np.int32)
        nbs = np.zeros((nstreams, nslots, 2), np.int32)
        p = ExpectParams(int(max_hard_errors), int(max_age), int(bool(derive)))
        self._ck(self.lib.ft8gpu_decode_messages_expected(self.h, iq.ctypes.data, nstreams, nslots, state.ctypes.data, C.byref(p),
                                                          msgs.ctypes.data, n.ctypes.data, nbs.ctypes.data, HOST_PTRS))
        return msgs, n, nbs, state

    def decode_messages_expected_dev(self, iq_dev, nstreams, nslots, state_dev, max_hard_errors, max_age, derive, msgs_dev, n_msgs_dev,
                                     n_by_stage_dev=None):
        """the same with every array in HBM (iq, msgs and state 16-byte aligned); n_by_stage_dev: [nstreams][nslots][2] or None"""
        p = ExpectParams(int(max_hard_errors), int(max_age), int(bool(derive)))
        self._ck(self.lib.ft8gpu_decode_messages_expected(self.h, _ptr(iq_dev), nstreams, nslots, _ptr(state_dev), C.byref(p),
                                                          _ptr(msgs_dev), _ptr(n_msgs_dev),
                                                          None if n_by_stage_dev is None else _ptr(n_by_stage_dev), DEVICE_PTRS))

    def hint_candidates(self, mag, cands, counts, status_in, states, tries=HINT_TRIES, max_bad_per_64=HINT_MAX_BAD_PER_64,
                        max_hard_errors=HINT_MAX_HARD_ERRORS, max_age=0, use_phase=True,
                        status_out=None, info=None):
        """ft8gpu_hint_candidates.  states: HINT_STATE_DTYPE [B], the table of the receiver each frame belongs to (read only)
        -> (status_out [B][cap] STATUS_DTYPE, info [B][cap] HINT_INFO_DTYPE), new arrays; records at and behind counts[f] keep
        what status_out / info held (zeros when None)"""
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        cands, counts, status_in, out, inf = self._cand_arrays(B, cands, counts, status_in, status_out, info, HINT_INFO_DTYPE)
        states = np.ascontiguousarray(states)
        assert states.dtype == HINT_STATE_DTYPE and states.shape == (B,)
        p = HintParams(int(tries), int(max_bad_per_64), int(max_hard_errors), int(max_age), int(bool(use_phase)))
        self._ck(self.lib.ft8gpu_hint_candidates(self.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status_in.ctypes.data,
                                                 B, states.ctypes.data, C.byref(p), out.ctypes.data, inf.ctypes.data, HOST_PTRS))
        return out.view(STATUS_DTYPE).reshape(B, self.max_candidates), inf

    def hint_candidates_dev(self, mag_dev, cands_dev, counts_dev, status_in_dev, nframes, states_dev, tries, max_bad_per_64,
                            max_hard_errors, max_age, use_phase, status_out_dev, info_dev):
        """status_out_dev may be status_in_dev; states_dev: [nframes] 8208-byte tables, 16-byte aligned; info_dev: 16-byte records"""
        p = HintParams(int(tries), int(max_bad_per_64), int(max_hard_errors), int(max_age), int(bool(use_phase)))
        self._ck(self.lib.ft8gpu_hint_candidates(self.h, _ptr(mag_dev), _ptr(cands_dev), _ptr(counts_dev), _ptr(status_in_dev), nframes,
                                                 _ptr(states_dev), C.byref(p), _ptr(status_out_dev), _ptr(info_dev), DEVICE_PTRS))

    def hint_update(self, msgs, n_msgs, state=None):
        """ft8gpu_hint_update.  msgs: MESSAGE_DTYPE [nstreams][nslots][50], n_msgs: int32 [nstreams][nslots]; state:
        HINT_STATE_DTYPE [nstreams] as a previous call returned it, or None for reset tables (the caller's array stays as it
        is) -> the exit state [nstreams]"""
        msgs = np.ascontiguousarray(msgs)
        n_msgs = np.ascontiguousarray(n_msgs, np.int32)
        nstreams, nslots = n_msgs.shape
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (nstreams, nslots, MAX_MESSAGES)
        state = np.zeros(nstreams, HINT_STATE_DTYPE) if state is None else np.array(state, HINT_STATE_DTYPE, copy=True, ndmin=1)
        assert state.shape == (nstreams,)
        self._ck(self.lib.ft8gpu_hint_update(self.h, msgs.ctypes.data, n_msgs.ctypes.data, nstreams, nslots, state.ctypes.data, HOST_PTRS))
        return state

    def hint_update_dev(self, msgs_dev, n_msgs_dev, nstreams, nslots, state_dev):
        """all arrays in HBM; msgs and state 16-byte aligned; the states are updated in place"""
        self._ck(self.lib.ft8gpu_hint_update(self.h, _ptr(msgs_dev), _ptr(n_msgs_dev), nstreams, nslots, _ptr(state_dev), DEVICE_PTRS))

    def decode_messages_hinted(self, iq, tries=HINT_TRIES, max_bad_per_64=HINT_MAX_BAD_PER_64, max_hard_errors=HINT_MAX_HARD_ERRORS, state=None,
                               max_age=0, use_phase=True, msgs=None):
        """ft8gpu_decode_messages_hinted.  iq: float32 [nstreams][nslots][2][48000]; state as in hint_update
        -> (msgs [nstreams][nslots][50], n_msgs [nstreams][nslots], n_by_stage [nstreams][nslots][2]: the count after BP and
        after the hint stage, the exit state [nstreams]); pad[2] of a record gained by a call hint is 3"""
        iq = np.ascontiguousarray(iq, np.float32)
        nstreams, nslots = iq.shape[:2]
        assert iq.shape[2:] == (2, NSAMPLES)
        state = np.zeros(nstreams, HINT_STATE_DTYPE) if state is None else np.array(state, HINT_STATE_DTYPE, copy=True, ndmin=1)
        assert state.shape == (nstreams,)
        if msgs is None:
            msgs = np.zeros((nstreams, nslots, MAX_MESSAGES), MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (nstreams, nslots, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros((nstreams, nslots), np.int32)
        nbs = np.zeros((nstreams, nslots, 2), np.int32)
        p = HintParams(int(tries), int(max_bad_per_64), int(max_hard_errors), int(max_age), int(bool(use_phase)))
        self._ck(self.lib.ft8gpu_decode_messages_hinted(self.h, iq.ctypes.data, nstreams, nslots, state.ctypes.data, C.byref(p),
                                                        msgs.ctypes.data, n.ctypes.data, nbs.ctypes.data, HOST_PTRS))
        return msgs, n, nbs, state

    def decode_messages_hinted_dev(self, iq_dev, nstreams, nslots, state_dev, tries, max_bad_per_64, max_hard_errors, max_age, use_phase,
                                   msgs_dev, n_msgs_dev, n_by_stage_dev=None):
        """the same with every array in HBM (iq, msgs and state 16-byte aligned); n_by_stage_dev: [nstreams][nslots][2] or None"""
        p = HintParams(int(tries), int(max_bad_per_64), int(max_hard_errors), int(max_age), int(bool(use_phase)))
        self._ck(self.lib.ft8gpu_decode_messages_hinted(self.h, _ptr(iq_dev), nstreams, nslots, _ptr(state_dev), C.byref(p),
                                                        _ptr(msgs_dev), _ptr(n_msgs_dev),
                                                        None if n_by_stage_dev is None else _ptr(n_by_stage_dev), DEVICE_PTRS))

    def combine_candidates(self, mag, cands, counts, status_in, states, max_age=0, min_agree=COMBINE_MIN_AGREE,
                           status_out=None, info=None):
        """ft8gpu_combine_candidates.  states: SOFTMEM_STATE_DTYPE [B], the memory of the receiver each frame belongs to (read
        only) -> (status_out [B][cap] STATUS_DTYPE, info [B][cap] COMBINE_INFO_DTYPE), new arrays; records at and behind
        counts[f] keep what status_out / info held (zeros when None)"""
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        cands, counts, status_in, out, inf = self._cand_arrays(B, cands, counts, status_in, status_out, info, COMBINE_INFO_DTYPE)
        states = np.ascontiguousarray(states)
        assert states.dtype == SOFTMEM_STATE_DTYPE and states.shape == (B,)
        self._ck(self.lib.ft8gpu_combine_candidates(self.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status_in.ctypes.data,
                                                    B, states.ctypes.data, int(max_age), int(min_agree), out.ctypes.data,
                                                    inf.ctypes.data, HOST_PTRS))
        return out.view(STATUS_DTYPE).reshape(B, self.max_candidates), inf

    def combine_candidates_dev(self, mag_dev, cands_dev, counts_dev, status_in_dev, nframes, states_dev, max_age, min_agree,
                               status_out_dev, info_dev):
        """status_out_dev may be status_in_dev; states_dev: [nframes] 92176-byte memories, 16-byte aligned; info_dev: 8-byte records"""
        self._ck(self.lib.ft8gpu_combine_candidates(self.h, _ptr(mag_dev), _ptr(cands_dev), _ptr(counts_dev), _ptr(status_in_dev), nframes,
                                                    _ptr(states_dev), int(max_age), int(min_agree), _ptr(status_out_dev),
                                                    _ptr(info_dev), DEVICE_PTRS))

    def softmem_update(self, mag, cands, counts, status, info, states, store_per_slot=COMBINE_STORE_PER_SLOT):
        """ft8gpu_softmem_update, one slot.  status: the final status records [B][cap], info: COMBINE_INFO_DTYPE [B][cap] as
        combine_candidates returned it for the same frames and states; states: SOFTMEM_STATE_DTYPE [B] (the caller's array stays
        as it is) -> the exit states [B]"""
        mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
        B = mag.shape[0]
        cands = np.ascontiguousarray(cands)
        counts = np.ascontiguousarray(counts, np.int32)
        status = np.ascontiguousarray(status).view(np.uint8).reshape(B, self.max_candidates, 48)
        info = np.ascontiguousarray(info).view(COMBINE_INFO_DTYPE).reshape(B, self.max_candidates)
        states = np.array(states, SOFTMEM_STATE_DTYPE, copy=True, ndmin=1)
        assert cands.shape == (B, self.max_candidates) and cands.dtype == CAND_DTYPE and counts.shape == (B,) and states.shape == (B,)
        self._ck(self.lib.ft8gpu_softmem_update(self.h, mag.ctypes.data, cands.ctypes.data, counts.ctypes.data, status.ctypes.data,
                                                info.ctypes.data, B, states.ctypes.data, int(store_per_slot), HOST_PTRS))
        return states

    def softmem_update_dev(self, mag_dev, cands_dev, counts_dev, status_dev, info_dev, nframes, states_dev, store_per_slot):
        """all arrays in HBM; the states (16-byte aligned) are updated in place"""
        self._ck(self.lib.ft8gpu_softmem_update(self.h, _ptr(mag_dev), _ptr(cands_dev), _ptr(counts_dev), _ptr(status_dev),
                                                _ptr(info_dev), nframes, _ptr(states_dev), int(store_per_slot), DEVICE_PTRS))

    def decode_messages_combined(self, iq, state=None, min_agree=COMBINE_MIN_AGREE, max_age=0, store_per_slot=COMBINE_STORE_PER_SLOT,
                                 msgs=None):
        """ft8gpu_decode_messages_combined.  iq: float32 [nstreams][nslots][2][48000]; state: SOFTMEM_STATE_DTYPE [nstreams] as
        a previous call returned it, or None for reset memories (the caller's array stays as it is)
        -> (msgs [nstreams][nslots][50], n_msgs [nstreams][nslots], n_by_stage [nstreams][nslots][2]: the count after BP and
        after combining, the exit state [nstreams]); pad[2] of a record gained by combining is 2"""
        iq = np.ascontiguousarray(iq, np.float32)
        nstreams, nslots = iq.shape[:2]
        assert iq.shape[2:] == (2, NSAMPLES)
        state = np.zeros(nstreams, SOFTMEM_STATE_DTYPE) if state is None else np.array(state, SOFTMEM_STATE_DTYPE, copy=True, ndmin=1)
        assert state.shape == (nstreams,)
        if msgs is None:
            msgs = np.zeros((nstreams, nslots, MAX_MESSAGES), MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (nstreams, nslots, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros((nstreams, nslots), np.int32)
        nbs = np.zeros((nstreams, nslots, 2), np.int32)
        p = CombineParams(int(min_agree), int(max_age), int(store_per_slot))
        self._ck(self.lib.ft8gpu_decode_messages_combined(self.h, iq.ctypes.data, nstreams, nslots, state.ctypes.data, C.byref(p),
                                                          msgs.ctypes.data, n.ctypes.data, nbs.ctypes.data, HOST_PTRS))
        return msgs, n, nbs, state

    def decode_messages_combined_dev(self, iq_dev, nstreams, nslots, state_dev, min_agree, max_age, store_per_slot, msgs_dev,
                                     n_msgs_dev, n_by_stage_dev=None):
        """the same with every array in HBM (iq, msgs and state 16-byte aligned); n_by_stage_dev: [nstreams][nslots][2] or None"""
        p = CombineParams(int(min_agree), int(max_age), int(store_per_slot))
        self._ck(self.lib.ft8gpu_decode_messages_combined(self.h, _ptr(iq_dev), nstreams, nslots, _ptr(state_dev), C.byref(p),
                                                          _ptr(msgs_dev), _ptr(n_msgs_dev),
                                                          None if n_by_stage_dev is None else _ptr(n_by_stage_dev), DEVICE_PTRS))

    def demod_candidates(self, iq, cands, counts, status_in, sets=DEMOD_SETS, max_hard_errors=DEMOD_MAX_HARD_ERRORS,
                         max_per_frame=None, status_out=None, info=None):
        """ft8gpu_demod_candidates -> (status_out [B][cap] STATUS_DTYPE, info [B][cap] DEMOD_INFO_DTYPE), new arrays; records at
        and behind counts[f] keep what status_out / info held (zeros when None).  max_per_frame None: max_candidates"""
        iq = np.ascontiguousarray(iq, np.float32).reshape(-1, 2, NSAMPLES)
        B = iq.shape[0]
        cands, counts, status_in, out, inf = self._cand_arrays(B, cands, counts, status_in, status_out, info, DEMOD_INFO_DTYPE)
        p = DemodParams(int(sets), int(max_hard_errors), int(self.max_candidates if max_per_frame is None else max_per_frame))
        self._ck(self.lib.ft8gpu_demod_candidates(self.h, iq.ctypes.data, cands.ctypes.data, counts.ctypes.data, status_in.ctypes.data,
                                                  B, C.byref(p), out.ctypes.data, inf.ctypes.data, HOST_PTRS))
        return out.view(STATUS_DTYPE).reshape(B, self.max_candidates), inf

    def demod_candidates_dev(self, iq_dev, cands_dev, counts_dev, status_in_dev, nframes, sets, max_hard_errors, max_per_frame,
                             status_out_dev, info_dev):
        """status_out_dev may be status_in_dev; iq_dev 16-byte aligned; info_dev: 16-byte records"""
        p = DemodParams(int(sets), int(max_hard_errors), int(max_per_frame))
        self._ck(self.lib.ft8gpu_demod_candidates(self.h, _ptr(iq_dev), _ptr(cands_dev), _ptr(counts_dev), _ptr(status_in_dev), int(nframes),
                                                  C.byref(p), _ptr(status_out_dev), _ptr(info_dev), DEVICE_PTRS))

    def decode_messages_demod(self, iq, sets=DEMOD_SETS, max_hard_errors=DEMOD_MAX_HARD_ERRORS, max_per_frame=None, msgs=None):
        """ft8gpu_decode_messages_demod -> (msgs [B][50], n_msgs [B], n_by_stage [B][2]: the count after BP and after the second
        demodulation); pad[3] of a record the stage gained is the accepted set"""
        iq = np.ascontiguousarray(iq, np.float32).reshape(-1, 2, NSAMPLES)
        B = iq.shape[0]
        if msgs is None:
            msgs = np.zeros((B, MAX_MESSAGES), MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros(B, np.int32)
        nbs = np.zeros((B, 2), np.int32)
        p = DemodParams(int(sets), int(max_hard_errors), int(self.max_candidates if max_per_frame is None else max_per_frame))
        self._ck(self.lib.ft8gpu_decode_messages_demod(self.h, iq.ctypes.data, B, C.byref(p), msgs.ctypes.data, n.ctypes.data,
                                                       nbs.ctypes.data, HOST_PTRS))
        return msgs, n, nbs

    def decode_messages_demod_dev(self, iq_dev, nframes, sets, max_hard_errors, max_per_frame, msgs_dev, n_msgs_dev, n_by_stage_dev=None):
        """the same with every array in HBM (iq and msgs 16-byte aligned); n_by_stage_dev: [nframes][2] or None"""
        p = DemodParams(int(sets), int(max_hard_errors), int(max_per_frame))
        self._ck(self.lib.ft8gpu_decode_messages_demod(self.h, _ptr(iq_dev), int(nframes), C.byref(p), _ptr(msgs_dev), _ptr(n_msgs_dev),
                                                       None if n_by_stage_dev is None else _ptr(n_by_stage_dev), DEVICE_PTRS))

    def demod_soft(self, iq, cands, counts, status_in, sets=DEMOD_SETS, max_hard_errors=DEMOD_MAX_HARD_ERRORS, max_per_frame=None,
                   status_out=None, info=None, soft=None):
        """ft8gpu_demod_soft -> (status_out, info as demod_candidates, soft [B][cap][3][176] float32: the normalised soft bits of
        the sets bp_decode ran on, zero rows elsewhere), new arrays; records at and behind counts[f] keep what the arrays held"""
        iq = np.ascontiguousarray(iq, np.float32).reshape(-1, 2, NSAMPLES)
        B = iq.shape[0]
        cands, counts, status_in, out, inf = self._cand_arrays(B, cands, counts, status_in, status_out, info, DEMOD_INFO_DTYPE)
        shape = (B, self.max_candidates, 3, SOFT_STRIDE)
        soft = np.zeros(shape, np.float32) if soft is None else np.array(soft, np.float32, copy=True, order="C").reshape(shape)
        p = DemodParams(int(sets), int(max_hard_errors), int(self.max_candidates if max_per_frame is None else max_per_frame))
        self._ck(self.lib.ft8gpu_demod_soft(self.h, iq.ctypes.data, cands.ctypes.data, counts.ctypes.data, status_in.ctypes.data,
                                            B, C.byref(p), out.ctypes.data, inf.ctypes.data, soft.ctypes.data, HOST_PTRS))
        return out.view(STATUS_DTYPE).reshape(B, self.max_candidates), inf, soft

    def demod_soft_dev(self, iq_dev, cands_dev, counts_dev, status_in_dev, nframes, sets, max_hard_errors, max_per_frame,
                       status_out_dev, info_dev, soft_dev):
        """status_out_dev may be status_in_dev; iq_dev and soft_dev 16-byte aligned"""
        p = DemodParams(int(sets), int(max_hard_errors), int(max_per_frame))
        self._ck(self.lib.ft8gpu_demod_soft(self.h, _ptr(iq_dev), _ptr(cands_dev), _ptr(counts_dev), _ptr(status_in_dev), int(nframes),
                                            C.byref(p), _ptr(status_out_dev), _ptr(info_dev), _ptr(soft_dev), DEVICE_PTRS))

    def ap_soft_candidates(self, soft, counts, status_in, sets=DEMOD_SETS, hyps=("CQ ? ?",), max_hard_errors=APSOFT_MAX_HARD_ERRORS,
                           status_out=None, info=None):
        """ft8gpu_ap_soft_candidates -> (status_out [B][cap] STATUS_DTYPE, info [B][cap] APSOFT_INFO_DTYPE), new arrays; records
        at and behind counts[f] keep what status_out / info held (zeros when None).  hyps: patterns or AP_HYP_DTYPE records"""
        soft = np.ascontiguousarray(soft, np.float32).reshape(-1, self.max_candidates, 3, SOFT_STRIDE)
        B = soft.shape[0]
        counts = np.ascontiguousarray(counts, np.int32)
        status_in = np.ascontiguousarray(status_in).view(np.uint8).reshape(B, self.max_candidates, 48)
        assert counts.shape == (B,)
        out = np.zeros((B, self.max_candidates, 48), np.uint8) if status_out is None else \
            np.array(status_out, copy=True, order="C").view(np.uint8).reshape(B, self.max_candidates, 48)
        inf = np.zeros((B, self.max_candidates), APSOFT_INFO_DTYPE) if info is None else \
            np.array(info, copy=True, order="C").view(APSOFT_INFO_DTYPE).reshape(B, self.max_candidates)
        hyps = _ap_hyps(hyps)
        self._ck(self.lib.ft8gpu_ap_soft_candidates(self.h, soft.ctypes.data, counts.ctypes.data, status_in.ctypes.data, B, int(sets),
                                                    hyps.ctypes.data, len(hyps), int(max_hard_errors), out.ctypes.data, inf.ctypes.data,
                                                    HOST_PTRS))
        return out.view(STATUS_DTYPE).reshape(B, self.max_candidates), inf

    def ap_soft_candidates_dev(self, soft_dev, counts_dev, status_in_dev, nframes, sets, hyps, max_hard_errors, status_out_dev, info_dev):
        """status_out_dev may be status_in_dev; soft_dev 16-byte aligned; info_dev: 20-byte records; hyps stay on the host"""
        hyps = _ap_hyps(hyps)
        self._ck(self.lib.ft8gpu_ap_soft_candidates(self.h, _ptr(soft_dev), _ptr(counts_dev), _ptr(status_in_dev), int(nframes), int(sets),
                                                    hyps.ctypes.data, len(hyps), int(max_hard_errors), _ptr(status_out_dev),
                                                    _ptr(info_dev), DEVICE_PTRS))

    def _demod_ap_params(self, sets, max_hard_errors, max_per_frame, hyps, ap_max_hard_errors):
        hyps = _ap_hyps(hyps)
        p = DemodApParams(DemodParams(int(sets), int(max_hard_errors), int(self.max_candidates if max_per_frame is None else max_per_frame)),
                          len(hyps), int(ap_max_hard_errors))
        C.memmove(C.addressof(p.hyps), hyps.ctypes.data, min(hyps.nbytes, C.sizeof(p.hyps)))
        return p

    def decode_messages_demod_ap(self, iq, sets=DEMOD_SETS, max_hard_errors=DEMOD_MAX_HARD_ERRORS, max_per_frame=None,
                                 hyps=("CQ ? ?",), ap_max_hard_errors=APSOFT_MAX_HARD_ERRORS, msgs=None):
        """ft8gpu_decode_messages_demod_ap -> (msgs [B][50], n_msgs [B], n_by_stage [B][3]: the count after BP, after the second
        demodulation and after AP on its soft bits); pad[1] = 1 + hypothesis and pad[3] = set on a record AP gained.  hyps = (): no AP"""
        iq = np.ascontiguousarray(iq, np.float32).reshape(-1, 2, NSAMPLES)
        B = iq.shape[0]
        if msgs is None:
            msgs = np.zeros((B, MAX_MESSAGES), MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros(B, np.int32)
        nbs = np.zeros((B, 3), np.int32)
        p = self._demod_ap_params(sets, max_hard_errors, max_per_frame, hyps, ap_max_hard_errors)
        self._ck(self.lib.ft8gpu_decode_messages_demod_ap(self.h, iq.ctypes.data, B, C.byref(p), msgs.ctypes.data, n.ctypes.data,
                                                          nbs.ctypes.data, HOST_PTRS))
        return msgs, n, nbs

    def decode_messages_demod_ap_dev(self, iq_dev, nframes, sets, max_hard_errors, max_per_frame, hyps, ap_max_hard_errors, msgs_dev,
                                     n_msgs_dev, n_by_stage_dev=None):
        """the same with every array in HBM (iq and msgs 16-byte aligned); n_by_stage_dev: [nframes][3] or None"""
        p = self._demod_ap_params(sets, max_hard_errors, max_per_frame, hyps, ap_max_hard_errors)
        self._ck(self.lib.ft8gpu_decode_messages_demod_ap(self.h, _ptr(iq_dev), int(nframes), C.byref(p), _ptr(msgs_dev), _ptr(n_msgs_dev),
                                                          None if n_by_stage_dev is None else _ptr(n_by_stage_dev), DEVICE_PTRS))

    # ---- device-pointer API (inputs and outputs resident in HBM) --------------------------------
    def refine_messages(self, iq, msgs, n_msgs, refined=None):
        """the refine stage (ft8gpu_refine_messages) -> refined [B][50] REFINED_DTYPE; records at and behind n_msgs[f] keep what
        `refined` held (zeros when None)"""
        iq = np.ascontiguousarray(iq, np.float32)
        msgs = np.ascontiguousarray(msgs)
        n_msgs = np.ascontiguousarray(n_msgs, np.int32)
        B = iq.shape[0]
        assert iq.shape[1:] == (2, NSAMPLES) and msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES) and n_msgs.shape == (B,)
        if refined is None:
            refined = np.zeros((B, MAX_MESSAGES), REFINED_DTYPE)
        assert refined.dtype == REFINED_DTYPE and refined.shape == (B, MAX_MESSAGES) and refined.flags["C_CONTIGUOUS"]
        self._ck(self.lib.ft8gpu_refine_messages(self.h, iq.ctypes.data, msgs.ctypes.data, n_msgs.ctypes.data, B, refined.ctypes.data,
                                               HOST_PTRS))
        return refined

    def refine_messages_dev(self, iq_dev, msgs_dev, n_msgs_dev, nframes, refined_dev):
        self._ck(self.lib.ft8gpu_refine_messages(self.h, _ptr(iq_dev), _ptr(msgs_dev), _ptr(n_msgs_dev), int(nframes), _ptr(refined_dev),
                                               DEVICE_PTRS))

    def decode_messages_refined(self, iq, msgs=None, refined=None):
        """ft8gpu_decode_messages and the refine stage on its records -> (msgs [B][50], n_msgs [B], refined [B][50])"""
        iq = np.ascontiguousarray(iq, np.float32)
        B = iq.shape[0]
        assert iq.shape[1:] == (2, NSAMPLES)
        if msgs is None:
            msgs = np.zeros((B, MAX_MESSAGES), MESSAGE_DTYPE)
        if refined is None:
            refined = np.zeros((B, MAX_MESSAGES), REFINED_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        assert refined.dtype == REFINED_DTYPE and refined.shape == (B, MAX_MESSAGES) and refined.flags["C_CONTIGUOUS"]
        n = np.zeros(B, np.int32)
        self._ck(self.lib.ft8gpu_decode_messages_refined(self.h, iq.ctypes.data, B, msgs.ctypes.data, n.ctypes.data, refined.ctypes.data,
                                                       HOST_PTRS))
        return msgs, n, refined

    def decode_messages_refined_dev(self, iq_dev, nframes, msgs_dev, n_msgs_dev, refined_dev):
        self._ck(self.lib.ft8gpu_decode_messages_refined(self.h, _ptr(iq_dev), int(nframes), _ptr(msgs_dev), _ptr(n_msgs_dev),
                                                       _ptr(refined_dev), DEVICE_PTRS))

    def _subtract_entry(self, name, shape):
        """(the entry `name` or its shaped form, the arguments that go in front of the flags): shape None is the older entry,
        SUBTRACT_CPFSK / SUBTRACT_GFSK the shaped one (ft8gpu_subtract_messages_shaped, ft8gpu_decode_messages_subtracted_shaped)"""
        return (getattr(self.lib, name), ()) if shape is None else (getattr(self.lib, name + "_shaped"), (int(shape),))

    def subtract_messages(self, iq, msgs, refined, first, n_msgs, info=None, want_info=True, shape=None):
        """the subtraction stage (ft8gpu_subtract_messages) -> (iq_out [B][2][48000], info [B][50] SUBTRACT_INFO_DTYPE): the frames
        with the records [first[f], n_msgs[f]) subtracted; info records outside that range keep what `info` held (zeros when None).
        want_info = False passes NULL and returns (iq_out, None).  shape: None for that entry, or the reference's shape through
        ft8gpu_subtract_messages_shaped: SUBTRACT_CPFSK (the same bytes) or SUBTRACT_GFSK, the waveform a station sends."""
        iq = np.ascontiguousarray(iq, np.float32)
        msgs = np.ascontiguousarray(msgs)
        refined = np.ascontiguousarray(refined)
        first = np.ascontiguousarray(first, np.int32)
        n_msgs = np.ascontiguousarray(n_msgs, np.int32)
        B = iq.shape[0]
        assert iq.shape[1:] == (2, NSAMPLES) and msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES)
        assert refined.dtype == REFINED_DTYPE and refined.shape == (B, MAX_MESSAGES) and first.shape == (B,) and n_msgs.shape == (B,)
        if not want_info:
            info = None
        elif info is None:
            info = np.zeros((B, MAX_MESSAGES), SUBTRACT_INFO_DTYPE)
        assert info is None or (info.dtype == SUBTRACT_INFO_DTYPE and info.shape == (B, MAX_MESSAGES) and info.flags["C_CONTIGUOUS"])
        out = np.zeros((B, 2, NSAMPLES), np.float32)
        entry, shaped = self._subtract_entry("ft8gpu_subtract_messages", shape)
        self._ck(entry(self.h, iq.ctypes.data, msgs.ctypes.data, refined.ctypes.data, first.ctypes.data, n_msgs.ctypes.data, B,
                       out.ctypes.data, None if info is None else info.ctypes.data, *shaped, HOST_PTRS))
        return out, info

    def subtract_messages_dev(self, iq_dev, msgs_dev, refined_dev, first_dev, n_msgs_dev, nframes, iq_out_dev, info_dev=None, shape=None):
        """every array in HBM (iq_dev and iq_out_dev 16-byte aligned; iq_out_dev may be iq_dev); info_dev: [nframes][50] 64-byte
        records or None; shape as in subtract_messages"""
        entry, shaped = self._subtract_entry("ft8gpu_subtract_messages", shape)
        self._ck(entry(self.h, _ptr(iq_dev), _ptr(msgs_dev), _ptr(refined_dev), _ptr(first_dev), _ptr(n_msgs_dev), int(nframes),
                       _ptr(iq_out_dev), None if info_dev is None else _ptr(info_dev), *shaped, DEVICE_PTRS))

    def decode_messages_subtracted(self, iq, passes=2, msgs=None, want_residual=True, shape=None):
        """multi-pass decoding with subtraction in the I/Q samples (ft8gpu_decode_messages_subtracted) -> (msgs [B][50], n_msgs [B],
        n_by_pass [B][passes], residual [B][2][48000] or None): every frame's last x_p.  shape: None for that entry, or the
        reference's shape through ft8gpu_decode_messages_subtracted_shaped: SUBTRACT_CPFSK (the same bytes) or SUBTRACT_GFSK, which
        cancels signals from the air deeper (profiles/subtract_gfsk_accuracy.json)."""
        iq = np.ascontiguousarray(iq, np.float32)
        B = iq.shape[0]
        assert iq.shape[1:] == (2, NSAMPLES)
        if msgs is None:
            msgs = np.zeros((B, MAX_MESSAGES), MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == (B, MAX_MESSAGES) and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros(B, np.int32)
        nbp = np.zeros((B, max(int(passes), 1)), np.int32)
        res = np.zeros((B, 2, NSAMPLES), np.float32) if want_residual else None
        entry, shaped = self._subtract_entry("ft8gpu_decode_messages_subtracted", shape)
        self._ck(entry(self.h, iq.ctypes.data, B, int(passes), msgs.ctypes.data, n.ctypes.data, nbp.ctypes.data,
                       None if res is None else res.ctypes.data, *shaped, HOST_PTRS))
        return msgs, n, nbp, res

    def decode_messages_subtracted_dev(self, iq_dev, nframes, passes, msgs_dev, n_msgs_dev, n_by_pass_dev=None, residual_dev=None,
                                       shape=None):
        """n_by_pass_dev: [nframes][passes] int32 or None; residual_dev: [nframes][2][48000] float32 (16-byte aligned) or None;
        shape as in decode_messages_subtracted"""
        entry, shaped = self._subtract_entry("ft8gpu_decode_messages_subtracted", shape)
        self._ck(entry(self.h, _ptr(iq_dev), int(nframes), int(passes), _ptr(msgs_dev), _ptr(n_msgs_dev),
                       None if n_by_pass_dev is None else _ptr(n_by_pass_dev), None if residual_dev is None else _ptr(residual_dev),
                       *shaped, DEVICE_PTRS))

    @staticmethod
    def _audio_clips(pcm):
        """pcm [nclips][nsamples] int16 or float32 (anything else becomes float32) -> (array, format)"""
        pcm = np.asarray(pcm)
        pcm = np.ascontiguousarray(pcm, np.int16 if pcm.dtype == np.int16 else np.float32)
        assert pcm.ndim == 2
        return pcm, AUDIO_S16 if pcm.dtype == np.int16 else AUDIO_F32

    def audio_frames(self, pcm, base_bins=(0, 240)):
        """the audio front end (ft8gpu_audio_frames): 12 kHz clips [nclips][nsamples], int16 or float32 -> iq
        [nclips][nbands][2][48000], the band of 1600 Hz above 6.25 * base_bin Hz of every clip as a frame of the decoder"""
        pcm, fmt = self._audio_clips(pcm)
        bases = np.ascontiguousarray(base_bins, np.int32).reshape(-1)
        out = np.zeros((pcm.shape[0], len(bases), 2, NSAMPLES), np.float32)
        self._ck(self.lib.ft8gpu_audio_frames(self.h, pcm.ctypes.data, fmt, pcm.shape[0], pcm.shape[1], bases.ctypes.data, len(bases),
                                            out.ctypes.data, HOST_PTRS))
        return out

    def audio_frames_dev(self, pcm_dev, fmt, nclips, nsamples, base_bins, iq_out_dev):
        """pcm_dev [nclips][nsamples] and iq_out_dev [nclips][nbands][2][48000] (16-byte aligned) in HBM; base_bins stay on the host"""
        bases = np.ascontiguousarray(base_bins, np.int32).reshape(-1)
        self._ck(self.lib.ft8gpu_audio_frames(self.h, _ptr(pcm_dev), int(fmt), int(nclips), int(nsamples), bases.ctypes.data, len(bases),
                                            _ptr(iq_out_dev), DEVICE_PTRS))

    def decode_audio(self, pcm, base_bins=(0, 240), msgs=None):
        """the whole path from 12 kHz audio (ft8gpu_decode_audio) -> (msgs [nclips][50 * nbands], n_msgs [nclips]): every band's
        messages, a message heard in two bands once, freq_hz on the clip's audio axis, pad[0] the band it was taken from"""
        pcm, fmt = self._audio_clips(pcm)
        bases = np.ascontiguousarray(base_bins, np.int32).reshape(-1)
        shape = (pcm.shape[0], MAX_MESSAGES * max(len(bases), 1))
        if msgs is None:
            msgs = np.zeros(shape, MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == shape and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros(pcm.shape[0], np.int32)
        self._ck(self.lib.ft8gpu_decode_audio(self.h, pcm.ctypes.data, fmt, pcm.shape[0], pcm.shape[1], bases.ctypes.data, len(bases),
                                            msgs.ctypes.data, n.ctypes.data, HOST_PTRS))
        return msgs, n

    def decode_audio_dev(self, pcm_dev, fmt, nclips, nsamples, base_bins, msgs_dev, n_msgs_dev):
        """pcm_dev, msgs_dev [nclips][50 * nbands] and n_msgs_dev [nclips] in HBM; base_bins stay on the host"""
        bases = np.ascontiguousarray(base_bins, np.int32).reshape(-1)
        self._ck(self.lib.ft8gpu_decode_audio(self.h, _ptr(pcm_dev), int(fmt), int(nclips), int(nsamples), bases.ctypes.data, len(bases),
                                            _ptr(msgs_dev), _ptr(n_msgs_dev), DEVICE_PTRS))

    def wide_frames(self, raw, freq_bins, normalise=False):
        """the wideband RX front end (ft8gpu_wide_frames): 2.4 Msps captures, uint8 [ncaptures][2 * npairs] -> iq
        [ncaptures][nchannels][2][48000], the 1600 Hz above the capture's centre + 6.25 * freq_bin Hz as a frame of the decoder"""
        raw = np.ascontiguousarray(raw, np.uint8)
        assert raw.ndim == 2
        bins = np.ascontiguousarray(freq_bins, np.int32).reshape(-1)
        out = np.zeros((raw.shape[0], len(bins), 2, NSAMPLES), np.float32)
        self._ck(self.lib.ft8gpu_wide_frames(self.h, raw.ctypes.data, raw.shape[0], raw.shape[1] // 2, bins.ctypes.data, len(bins),
                                           out.ctypes.data, int(normalise), HOST_PTRS))
        return out

    def wide_frames_dev(self, raw_dev, ncaptures, npairs, freq_bins, iq_dev, normalise=False):
        """raw_dev [ncaptures][2 * npairs] and iq_dev [ncaptures][nchannels][2][48000] (both 16-byte aligned) in HBM; freq_bins
        stay on the host"""
        bins = np.ascontiguousarray(freq_bins, np.int32).reshape(-1)
        self._ck(self.lib.ft8gpu_wide_frames(self.h, _ptr(raw_dev), int(ncaptures), int(npairs), bins.ctypes.data, len(bins),
                                           _ptr(iq_dev), int(normalise), DEVICE_PTRS))

    def decode_wide(self, raw, freq_bins, msgs=None):
        """the whole path from 2.4 Msps captures (ft8gpu_decode_wide) -> (msgs [ncaptures][50 * nchannels], n_msgs [ncaptures]):
        every channel's messages, a message heard in two overlapping channels once, freq_hz relative to the capture's centre,
        pad[0] the channel it was taken from"""
        raw = np.ascontiguousarray(raw, np.uint8)
        assert raw.ndim == 2
        bins = np.ascontiguousarray(freq_bins, np.int32).reshape(-1)
        shape = (raw.shape[0], MAX_MESSAGES * max(len(bins), 1))
        if msgs is None:
            msgs = np.zeros(shape, MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == shape and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros(raw.shape[0], np.int32)
        self._ck(self.lib.ft8gpu_decode_wide(self.h, raw.ctypes.data, raw.shape[0], raw.shape[1] // 2, bins.ctypes.data, len(bins),
                                           msgs.ctypes.data, n.ctypes.data, HOST_PTRS))
        return msgs, n

    def decode_wide_dev(self, raw_dev, ncaptures, npairs, freq_bins, msgs_dev, n_msgs_dev):
        """raw_dev, msgs_dev [ncaptures][50 * nchannels] and n_msgs_dev [ncaptures] in HBM; freq_bins stay on the host"""
        bins = np.ascontiguousarray(freq_bins, np.int32).reshape(-1)
        self._ck(self.lib.ft8gpu_decode_wide(self.h, _ptr(raw_dev), int(ncaptures), int(npairs), bins.ctypes.data, len(bins),
                                           _ptr(msgs_dev), _ptr(n_msgs_dev), DEVICE_PTRS))

    @staticmethod
    def _pcm_captures(pcm, complex_iq):
        """[ncaptures][nsamples] (complex: [ncaptures][2 * nsamples], I and Q interleaved, or a complex64 array), int16 or float32
        -> (array, format, nsamples)"""
        pcm = np.asarray(pcm)
        if pcm.dtype == np.complex64:
            pcm, complex_iq = np.ascontiguousarray(pcm).view(np.float32), True
        pcm = np.ascontiguousarray(pcm, np.int16 if pcm.dtype == np.int16 else np.float32)
        assert pcm.ndim == 2 and (not complex_iq or pcm.shape[1] % 2 == 0)
        fmt = (PCM_S16 if pcm.dtype == np.int16 else PCM_F32) | (PCM_COMPLEX if complex_iq else 0)
        return pcm, fmt, pcm.shape[1] // (2 if complex_iq else 1)

    def pcm_frames(self, pcm, rate, freq_bins, complex_iq=False, normalise=False):
        """the PCM front end (ft8gpu_pcm_frames): captures at 48 .. 768 ksps, real [ncaptures][nsamples] or complex [ncaptures][2 *
        nsamples], int16 or float32 -> iq [ncaptures][nchannels][2][48000], the 1600 Hz above 6.25 * freq_bin Hz of the input's
        0 Hz as a frame of the decoder"""
        pcm, fmt, nsamples = self._pcm_captures(pcm, complex_iq)
        bins = np.ascontiguousarray(freq_bins, np.int32).reshape(-1)
        out = np.zeros((pcm.shape[0], len(bins), 2, NSAMPLES), np.float32)
        self._ck(self.lib.ft8gpu_pcm_frames(self.h, pcm.ctypes.data, fmt, int(rate), pcm.shape[0], nsamples, bins.ctypes.data, len(bins),
                                          out.ctypes.data, int(normalise), HOST_PTRS))
        return out

    def pcm_frames_dev(self, pcm_dev, fmt, rate, ncaptures, nsamples, freq_bins, iq_dev, normalise=False):
        """pcm_dev [ncaptures][nsamples] samples of fmt (aligned to the sample type) and iq_dev [ncaptures][nchannels][2][48000]
        (16-byte aligned) in HBM; freq_bins stay on the host"""
        bins = np.ascontiguousarray(freq_bins, np.int32).reshape(-1)
        self._ck(self.lib.ft8gpu_pcm_frames(self.h, _ptr(pcm_dev), int(fmt), int(rate), int(ncaptures), int(nsamples), bins.ctypes.data,
                                          len(bins), _ptr(iq_dev), int(normalise), DEVICE_PTRS))

    def decode_pcm(self, pcm, rate, freq_bins, complex_iq=False, msgs=None):
        """the whole path from PCM captures (ft8gpu_decode_pcm) -> (msgs [ncaptures][50 * nchannels], n_msgs [ncaptures]): every
        channel's messages, a message heard in two overlapping channels once, freq_hz on the input's own axis, pad[0] the channel
        it was taken from"""
        pcm, fmt, nsamples = self._pcm_captures(pcm, complex_iq)
        bins = np.ascontiguousarray(freq_bins, np.int32).reshape(-1)
        shape = (pcm.shape[0], MAX_MESSAGES * max(len(bins), 1))
        if msgs is None:
            msgs = np.zeros(shape, MESSAGE_DTYPE)
        assert msgs.dtype == MESSAGE_DTYPE and msgs.shape == shape and msgs.flags["C_CONTIGUOUS"]
        n = np.zeros(pcm.shape[0], np.int32)
        self._ck(self.lib.ft8gpu_decode_pcm(self.h, pcm.ctypes.data, fmt, int(rate), pcm.shape[0], nsamples, bins.ctypes.data, len(bins),
                                          msgs.ctypes.data, n.ctypes.data, HOST_PTRS))
        return msgs, n

    def decode_pcm_dev(self, pcm_dev, fmt, rate, ncaptures, nsamples, freq_bins, msgs_dev, n_msgs_dev):
        """pcm_dev, msgs_dev [ncaptures][50 * nchannels] and n_msgs_dev [ncaptures] in HBM; freq_bins stay on the host"""
        bins = np.ascontiguousarray(freq_bins, np.int32).reshape(-1)
        self._ck(self.lib.ft8gpu_decode_pcm(self.h, _ptr(pcm_dev), int(fmt), int(rate), int(ncaptures), int(nsamples), bins.ctypes.data,
                                          len(bins), _ptr(msgs_dev), _ptr(n_msgs_dev), DEVICE_PTRS))

    def ap_candidates_dev(self, mag_dev, cands_dev, counts_dev, status_in_dev, nframes, hyps, max_hard_errors, status_out_dev, info_dev):
        """status_out_dev may be status_in_dev; info_dev: [nframes][max_candidates] 8-byte records; hyps stay on the host"""
        hyps = _ap_hyps(hyps)
        self._ck(self.lib.ft8gpu_ap_candidates(self.h, _ptr(mag_dev), _ptr(cands_dev), _ptr(counts_dev), _ptr(status_in_dev), nframes,
                                               hyps.ctypes.data, len(hyps), int(max_hard_errors), _ptr(status_out_dev), _ptr(info_dev),
                                               DEVICE_PTRS))

    def decode_messages_ap_dev(self, iq_dev, nframes, passes, hyps, ap_max_hard_errors, osd_order, osd_max_hard_errors, msgs_dev,
                               n_msgs_dev, n_by_stage_dev=None):
        """n_by_stage_dev: [nframes][passes][3] int32, or None"""
        p = _ap_params(passes, hyps, ap_max_hard_errors, osd_order, osd_max_hard_errors)
        self._ck(self.lib.ft8gpu_decode_messages_ap(self.h, _ptr(iq_dev), nframes, C.byref(p), _ptr(msgs_dev), _ptr(n_msgs_dev),
                                                    None if n_by_stage_dev is None else _ptr(n_by_stage_dev), DEVICE_PTRS))

    def osd_candidates_dev(self, mag_dev, cands_dev, counts_dev, status_in_dev, nframes, order, max_hard_errors, status_out_dev, info_dev):
        """status_out_dev may be status_in_dev; info_dev: [nframes][max_candidates] 8-byte records"""
        self._ck(self.lib.ft8gpu_osd_candidates(self.h, _ptr(mag_dev), _ptr(cands_dev), _ptr(counts_dev), _ptr(status_in_dev), nframes,
                                              int(order), int(max_hard_errors), _ptr(status_out_dev), _ptr(info_dev), DEVICE_PTRS))

    def decode_messages_deep_dev(self, iq_dev, nframes, passes, osd_order, osd_max_hard_errors, msgs_dev, n_msgs_dev, n_by_stage_dev=None):
        """n_by_stage_dev: [nframes][passes][2] int32, or None"""
        p = DeepParams(int(passes), int(osd_order), int(osd_max_hard_errors))
        self._ck(self.lib.ft8gpu_decode_messages_deep(self.h, _ptr(iq_dev), nframes, C.byref(p), _ptr(msgs_dev), _ptr(n_msgs_dev),
                                                    None if n_by_stage_dev is None else _ptr(n_by_stage_dev), DEVICE_PTRS))

    def decode_messages_passes_dev(self, iq_dev, nframes, passes, msgs_dev, n_msgs_dev, n_by_pass_dev=None):
        """n_by_pass_dev: [nframes][passes] int32, or None"""
        self._ck(self.lib.ft8gpu_decode_messages_passes(self.h, _ptr(iq_dev), nframes, int(passes), _ptr(msgs_dev), _ptr(n_msgs_dev),
                                                      None if n_by_pass_dev is None else _ptr(n_by_pass_dev), DEVICE_PTRS))

    def mask_messages_dev(self, mag_dev, base_dev, msgs_dev, first_dev, n_msgs_dev, nframes, mag_out_dev):
        self._ck(self.lib.ft8gpu_mask_messages(self.h, _ptr(mag_dev), _ptr(base_dev), _ptr(msgs_dev), _ptr(first_dev), _ptr(n_msgs_dev),
                                             nframes, _ptr(mag_out_dev), DEVICE_PTRS))

    def append_messages_dev(self, mag_dev, base_dev, cands_dev, counts_dev, status_dev, nframes, msgs_dev, n_msgs_dev):
        self._ck(self.lib.ft8gpu_append_messages(self.h, _ptr(mag_dev), _ptr(base_dev), _ptr(cands_dev), _ptr(counts_dev),
                                               _ptr(status_dev), nframes, _ptr(msgs_dev), _ptr(n_msgs_dev), DEVICE_PTRS))

    def decode_messages_dev(self, iq_dev, nframes, msgs_dev, n_msgs_dev):
        self._ck(self.lib.ft8gpu_decode_messages(self.h, _ptr(iq_dev), nframes, _ptr(msgs_dev), _ptr(n_msgs_dev), DEVICE_PTRS))

    def collect_messages_dev(self, mag_dev, cands_dev, counts_dev, status_dev, nframes, msgs_dev, n_msgs_dev):
        self._ck(self.lib.ft8gpu_collect_messages(self.h, _ptr(mag_dev), _ptr(cands_dev), _ptr(counts_dev), _ptr(status_dev), nframes,
                                                _ptr(msgs_dev), _ptr(n_msgs_dev), DEVICE_PTRS))

    def noise_baseline_dev(self, mag_dev, nframes, base_dev):
        self._ck(self.lib.ft8gpu_noise_baseline(self.h, _ptr(mag_dev), nframes, _ptr(base_dev), DEVICE_PTRS))

    def decode_batch_dev(self, iq_dev, nframes, decodes_dev, n_results_dev):
        self._ck(self.lib.ft8gpu_decode_batch(self.h, _ptr(iq_dev), nframes, _ptr(decodes_dev), _ptr(n_results_dev),
                                            DEVICE_PTRS))

    def find_sync_dev(self, mag_dev, nframes, cands_dev, counts_dev):
        """cands_dev: [nframes][max_candidates] 8-byte records, counts_dev: [nframes] int32 (all in HBM)"""
        self._ck(self.lib.ft8gpu_find_sync(self.h, _ptr(mag_dev), nframes, _ptr(cands_dev), _ptr(counts_dev), DEVICE_PTRS))

    def decode_candidates_dev(self, mag_dev, cands_dev, counts_dev, nframes, status_dev):
        """status_dev: [nframes][max_candidates] 48-byte records in HBM; only records below counts are written"""
        self._ck(self.lib.ft8gpu_decode_candidates(self.h, _ptr(mag_dev), _ptr(cands_dev), _ptr(counts_dev), nframes, _ptr(status_dev), DEVICE_PTRS))

    def waterfall_dev(self, iq_dev, nframes, mag_dev):
        self._ck(self.lib.ft8gpu_waterfall(self.h, _ptr(iq_dev), nframes, _ptr(mag_dev), DEVICE_PTRS))

    def rx_decimate(self, raw, normalise=True):
        """raw: uint8 [ncaptures][2*npairs] host array -> float32 [ncaptures][2][48000]"""
        raw = np.ascontiguousarray(raw, np.uint8)
        ncap, nbytes = raw.shape
        iq = np.zeros((ncap, 2, NSAMPLES), np.float32)
        self._ck(self.lib.ft8gpu_rx_decimate(self.h, raw.ctypes.data, ncap, nbytes // 2, iq.ctypes.data, int(normalise), HOST_PTRS))
        return iq

    def rx_decimate_dev(self, raw_dev, ncaptures, npairs, iq_dev, normalise=True):
        self._ck(self.lib.ft8gpu_rx_decimate(self.h, _ptr(raw_dev), ncaptures, npairs, _ptr(iq_dev), int(normalise), DEVICE_PTRS))

    def rx_stream(self, raw, state=None, normalise=True, iq=None, n_out=None):
        """The RX front end with the filter state carried from slot to slot, as the reference's daemon runs it.
        raw: uint8 [nstreams][nslots][2*npairs] host array (consecutive buffers of each receiver); state: RX_STATE_DTYPE
        [nstreams] as a previous call returned it, or None for the reset state; iq / n_out: arrays to write into.
        -> (float32 [nstreams][nslots][2][48000], uint32 [nstreams][nslots] stored counts, the exit state [nstreams])"""
        raw = np.ascontiguousarray(raw, np.uint8)
        nstreams, nslots, nbytes = raw.shape
        if state is None:
            state = np.zeros(nstreams, RX_STATE_DTYPE)
        else:
            state = np.array(state, RX_STATE_DTYPE, copy=True, ndmin=1)   # the caller's entry state stays as it is
            assert state.shape == (nstreams,)
        if iq is None:
            iq = np.zeros((nstreams, nslots, 2, NSAMPLES), np.float32)
        if n_out is None:
            n_out = np.zeros((nstreams, nslots), np.uint32)
        assert iq.dtype == np.float32 and iq.shape == (nstreams, nslots, 2, NSAMPLES) and iq.flags.c_contiguous
        assert n_out.dtype == np.uint32 and n_out.shape == (nstreams, nslots) and n_out.flags.c_contiguous
        self._ck(self.lib.ft8gpu_rx_stream(self.h, raw.ctypes.data, nstreams, nslots, nbytes // 2, state.ctypes.data,
                                           iq.ctypes.data, n_out.ctypes.data, int(normalise), HOST_PTRS))
        return iq, n_out, state

    def rx_stream_dev(self, raw_dev, nstreams, nslots, npairs, state_dev, iq_dev, n_out_dev=None, normalise=True):
        """all arrays in HBM: raw [nstreams][nslots][2*npairs] uint8, state [nstreams] 516-byte records (updated in place),
        iq [nstreams][nslots][2][48000] float32, n_out [nstreams][nslots] uint32 or None"""
        self._ck(self.lib.ft8gpu_rx_stream(self.h, _ptr(raw_dev), nstreams, nslots, npairs, _ptr(state_dev), _ptr(iq_dev),
                                           _ptr(n_out_dev) if n_out_dev is not None else None, int(normalise), DEVICE_PTRS))

    def pskreporter_datagrams(self, decodes, n_results, info, unixtimes=None):
        """decodes: [n][50] RESULT_DTYPE, n_results: [n] -> (uint8 [n][DATAGRAM_STRIDE], int32 [n] lengths)"""
        decodes = np.ascontiguousarray(decodes)
        n_results = np.ascontiguousarray(n_results, np.int32)
        n = n_results.shape[0]
        assert decodes.dtype == RESULT_DTYPE and decodes.size == n * MAX_MESSAGES
        out = np.zeros((n, DATAGRAM_STRIDE), np.uint8)
        lengths = np.zeros(n, np.int32)
        t = None if unixtimes is None else np.ascontiguousarray(unixtimes, np.uint32)
        self._ck(self.lib.ft8gpu_pskreporter_datagrams(self.h, decodes.ctypes.data, n_results.ctypes.data, n, C.byref(info),
                                                     None if t is None else t.ctypes.data, out.ctypes.data,
                                                     lengths.ctypes.data, HOST_PTRS))
        return out, lengths

    def pskreporter_datagrams_dev(self, decodes_dev, n_results_dev, nframes, info, unixtimes_dev, datagrams_dev, lengths_dev):
        self._ck(self.lib.ft8gpu_pskreporter_datagrams(self.h, _ptr(decodes_dev), _ptr(n_results_dev), nframes, C.byref(info),
                                                     None if unixtimes_dev is None else _ptr(unixtimes_dev),
                                                     _ptr(datagrams_dev), _ptr(lengths_dev), DEVICE_PTRS))

    def synth_frames(self, signals, nframes, nsig, noise_sigma, seed, iq_dev, first_frame=0):
        """frame k of the call is global frame first_frame + k; its noise depends on (seed, global index) only"""
        signals = np.ascontiguousarray(signals)
        assert signals.dtype == SIGNAL_DTYPE and signals.size == nframes * nsig
        self._ck(self.lib.ft8gpu_synth_frames_at(self.h, signals.ctypes.data, nframes, nsig, float(noise_sigma),
                                               int(seed), int(first_frame), _ptr(iq_dev)))

    @staticmethod
    def _gfsk_signals(signals, nclips, nsig):
        signals = np.ascontiguousarray(signals)
        assert signals.dtype == SIGNAL_DTYPE and signals.size == nclips * nsig
        return signals

    def synth_gfsk_frames(self, signals, nframes, nsig, noise_sigma=0.0, seed=0, first_frame=0, peak=0.0):
        """ft8gpu_synth_gfsk_frames: signals [nframes][nsig] of SIGNAL_DTYPE -> iq float32 [nframes][2][48000], GFSK at 3200 sps;
        frame k is global frame first_frame + k for the noise; peak > 0 normalises every frame's largest sample to it"""
        signals = self._gfsk_signals(signals, nframes, nsig)
        out = np.zeros((nframes, 2, NSAMPLES), np.float32)
        self._ck(self.lib.ft8gpu_synth_gfsk_frames(self.h, signals.ctypes.data, int(nframes), int(nsig), float(noise_sigma), int(seed),
                                                 int(first_frame), float(peak), out.ctypes.data, HOST_PTRS))
        return out

    def synth_gfsk_frames_dev(self, signals, nframes, nsig, noise_sigma, seed, first_frame, peak, iq_out_dev):
        """iq_out_dev [nframes][2][48000] float32 in HBM; signals stay on the host"""
        signals = self._gfsk_signals(signals, nframes, nsig)
        self._ck(self.lib.ft8gpu_synth_gfsk_frames(self.h, signals.ctypes.data, int(nframes), int(nsig), float(noise_sigma), int(seed),
                                                 int(first_frame), float(peak), _ptr(iq_out_dev), DEVICE_PTRS))

    def synth_gfsk_audio(self, signals, nclips, nsig, nsamples=AUDIO_NSAMPLES, noise_sigma=0.0, seed=0, first_clip=0, peak=0.0,
                         fmt=AUDIO_F32):
        """ft8gpu_synth_gfsk_audio: signals [nclips][nsig] -> pcm [nclips][nsamples], int16 (AUDIO_S16) or float32, GFSK at 12 kHz"""
        signals = self._gfsk_signals(signals, nclips, nsig)
        out = np.zeros((nclips, max(int(nsamples), 0)), np.int16 if fmt == AUDIO_S16 else np.float32)
        self._ck(self.lib.ft8gpu_synth_gfsk_audio(self.h, signals.ctypes.data, int(nclips), int(nsig), int(nsamples), float(noise_sigma),
                                                int(seed), int(first_clip), float(peak), int(fmt), out.ctypes.data, HOST_PTRS))
        return out

    def synth_gfsk_audio_dev(self, signals, nclips, nsig, nsamples, noise_sigma, seed, first_clip, peak, fmt, pcm_out_dev):
        """pcm_out_dev [nclips][nsamples] of fmt in HBM; signals stay on the host"""
        signals = self._gfsk_signals(signals, nclips, nsig)
        self._ck(self.lib.ft8gpu_synth_gfsk_audio(self.h, signals.ctypes.data, int(nclips), int(nsig), int(nsamples), float(noise_sigma),
                                                int(seed), int(first_clip), float(peak), int(fmt), _ptr(pcm_out_dev), DEVICE_PTRS))

    @staticmethod
    def _gfsk_channels(channels, nclips, nsig):
        """None (the unfaded entries) or CHANNEL_DTYPE [nclips][nsig] -> the pointer the faded entries take"""
        if channels is None:
            return None, None
        channels = np.ascontiguousarray(channels)
        assert channels.dtype == CHANNEL_DTYPE and channels.size == nclips * nsig
        return channels, channels.ctypes.data

    def synth_gfsk_frames_faded(self, signals, channels, nframes, nsig, noise_sigma=0.0, seed=0, first_frame=0, peak=0.0):
        """ft8gpu_synth_gfsk_frames_faded: synth_gfsk_frames with channels [nframes][nsig] of CHANNEL_DTYPE (None: unfaded); the
        taps are keyed by seed and the global frame index"""
        signals = self._gfsk_signals(signals, nframes, nsig)
        channels, cp = self._gfsk_channels(channels, nframes, nsig)
        out = np.zeros((nframes, 2, NSAMPLES), np.float32)
        self._ck(self.lib.ft8gpu_synth_gfsk_frames_faded(self.h, signals.ctypes.data, cp, int(nframes), int(nsig), float(noise_sigma),
                                                       int(seed), int(first_frame), float(peak), out.ctypes.data, HOST_PTRS))
        return out

    def synth_gfsk_frames_faded_dev(self, signals, channels, nframes, nsig, noise_sigma, seed, first_frame, peak, iq_out_dev):
        """iq_out_dev [nframes][2][48000] float32 in HBM; signals and channels stay on the host"""
        signals = self._gfsk_signals(signals, nframes, nsig)
        channels, cp = self._gfsk_channels(channels, nframes, nsig)
        self._ck(self.lib.ft8gpu_synth_gfsk_frames_faded(self.h, signals.ctypes.data, cp, int(nframes), int(nsig), float(noise_sigma),
                                                       int(seed), int(first_frame), float(peak), _ptr(iq_out_dev), DEVICE_PTRS))

    def synth_gfsk_audio_faded(self, signals, channels, nclips, nsig, nsamples=AUDIO_NSAMPLES, noise_sigma=0.0, seed=0, first_clip=0,
                               peak=0.0, fmt=AUDIO_F32):
        """ft8gpu_synth_gfsk_audio_faded: synth_gfsk_audio with channels [nclips][nsig] of CHANNEL_DTYPE (None: unfaded)"""
        signals = self._gfsk_signals(signals, nclips, nsig)
        channels, cp = self._gfsk_channels(channels, nclips, nsig)
        out = np.zeros((nclips, max(int(nsamples), 0)), np.int16 if fmt == AUDIO_S16 else np.float32)
        self._ck(self.lib.ft8gpu_synth_gfsk_audio_faded(self.h, signals.ctypes.data, cp, int(nclips), int(nsig), int(nsamples),
                                                      float(noise_sigma), int(seed), int(first_clip), float(peak), int(fmt),
                                                      out.ctypes.data, HOST_PTRS))
        return out

    def synth_gfsk_audio_faded_dev(self, signals, channels, nclips, nsig, nsamples, noise_sigma, seed, first_clip, peak, fmt, pcm_out_dev):
        """pcm_out_dev [nclips][nsamples] of fmt in HBM; signals and channels stay on the host"""
        signals = self._gfsk_signals(signals, nclips, nsig)
        channels, cp = self._gfsk_channels(channels, nclips, nsig)
        self._ck(self.lib.ft8gpu_synth_gfsk_audio_faded(self.h, signals.ctypes.data, cp, int(nclips), int(nsig), int(nsamples),
                                                      float(noise_sigma), int(seed), int(first_clip), float(peak), int(fmt),
                                                      _ptr(pcm_out_dev), DEVICE_PTRS))

    # ---- device memory helpers of the C ABI (a plain C caller has no HIP headers) ---------------
    def dev_alloc(self, nbytes):
        p = self.lib.ft8gpu_dev_alloc(self.h, nbytes)
        if not p:
            raise Ft8GpuError(self.lib.ft8gpu_last_error().decode(errors="replace"))
        return p

    def dev_free(self, p):
        self.lib.ft8gpu_dev_free(self.h, C.c_void_p(p))

    def memcpy_h2d(self, dst_dev, src):
        src = np.ascontiguousarray(src)
        self._ck(self.lib.ft8gpu_memcpy_h2d(self.h, C.c_void_p(_ptr(dst_dev)), src.ctypes.data, src.nbytes))

    def memcpy_d2h(self, dst, src_dev):
        assert dst.flags["C_CONTIGUOUS"]
        self._ck(self.lib.ft8gpu_memcpy_d2h(self.h, dst.ctypes.data, C.c_void_p(_ptr(src_dev)), dst.nbytes))


def decode_batch_multi(decoders, iq, decodes=None):
    """ft8gpu_decode_batch_multi: host frames [B][2][48000] cut into len(decoders) contiguous shards, one host
    thread and one context (normally one GPU) per shard, records gathered in the caller's host arrays"""
    iq = np.ascontiguousarray(iq, np.float32)
    B = iq.shape[0]
    assert iq.shape[1:] == (2, NSAMPLES)
    if decodes is None:
        decodes = np.zeros((B, MAX_MESSAGES), RESULT_DTYPE)
    n = np.zeros(B, np.int32)
    hs = (C.c_void_p * len(decoders))(*[d.h for d in decoders])
    _check(load_library().ft8gpu_decode_batch_multi(hs, len(decoders), iq.ctypes.data, B, decodes.ctypes.data, n.ctypes.data))
    return decodes, n


class PinnedArray:
    """numpy view of page-locked host memory from ft8gpu_host_alloc.  The memory is freed by close() or at garbage
    collection -- and close() REFUSES while other references to `array` (or views of it) are alive: a view that outlived
    the allocation would be a use-after-free of unmapped pinned memory."""

    def __init__(self, shape, dtype=np.float32):
        lib = load_library()
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = lib.ft8gpu_host_alloc(self.nbytes)
        if not self.ptr:
            raise Ft8GpuError(lib.ft8gpu_last_error().decode(errors="replace"))
        self._buf = (C.c_char * self.nbytes).from_address(self.ptr)
        self._base = np.frombuffer(self._buf, dtype=dtype)          # every view of `array` keeps a reference to this object
        self.array = self._base.reshape(shape)
        self._quiet = self._refs()              # the counts with no outside reference, measured (not assumed per CPython version)

    def _refs(self):
        import sys
        return sys.getrefcount(self._base), sys.getrefcount(self.array)

    def close(self):
        """frees the pinned memory; raises -- and changes NOTHING, `array` stays usable -- while outside references to
        `array` or views of it are alive"""
        if self.ptr:
            now = self._refs()
            extra = (now[0] - self._quiet[0]) + (now[1] - self._quiet[1])
            if extra > 0:
                raise Ft8GpuError(f"PinnedArray.close(): {extra} reference(s) to the pinned buffer (`array` or views of it) are still alive; drop them first")
            self.array = None
            self._base = None
            self._buf = None
            load_library().ft8gpu_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Ft8GpuError as e:
            import warnings
            warnings.warn(f"PinnedArray collected while views of it are alive: {self.nbytes} bytes of pinned host memory are NOT freed ({e})",
                          ResourceWarning, source=self)
        except Exception:
            pass


def decode_batch_multi_dev(decoders, iq_devs, nframes, decodes=None):
    """ft8gpu_decode_batch_multi_dev: shard g's frames are resident on decoders[g]'s GPU (iq_devs[g]: device
    pointer / tensor, nframes[g] frames); records gathered on the host in shard order"""
    total = int(sum(nframes))
    if decodes is None:
        decodes = np.zeros((total, MAX_MESSAGES), RESULT_DTYPE)
    n = np.zeros(total, np.int32)
    k = len(decoders)
    hs = (C.c_void_p * k)(*[d.h for d in decoders])
    ps = (C.c_void_p * k)(*[_ptr(p) if p is not None else None for p in iq_devs])
    ns = (C.c_int * k)(*[int(x) for x in nframes])
    _check(load_library().ft8gpu_decode_batch_multi_dev(hs, k, ps, ns, decodes.ctypes.data, n.ctypes.data))
    return decodes, n


def gather_spots(decoders, decodes_devs, n_results_devs, frames_per_dev, all_decodes_devs, all_n_results_devs):
    """ft8gpu_gather_spots: single-process RCCL all-gather of every GPU's device-resident records and counts"""
    k = len(decoders)
    arr = lambda xs: (C.c_void_p * k)(*[_ptr(x) for x in xs])
    hs = (C.c_void_p * k)(*[d.h for d in decoders])
    _check(load_library().ft8gpu_gather_spots(hs, k, arr(decodes_devs), arr(n_results_devs), int(frames_per_dev),
                                              arr(all_decodes_devs), arr(all_n_results_devs)))


def format_spots(decodes, n_results, dial_freq, year, month, mday, hour, minute):
    """printSpots() (rtlsdr_ft8d.c:643-663) as a string"""
    L = load_library()
    decodes = np.ascontiguousarray(decodes)
    assert decodes.dtype == RESULT_DTYPE
    buf = C.create_string_buffer(64 + 48 * MAX_MESSAGES)
    n = L.ft8gpu_format_spots(decodes.ctypes.data, int(n_results), int(dial_freq), year, month, mday, hour, minute, buf, len(buf))
    if n < 0:
        raise Ft8GpuError("ft8gpu_format_spots failed")
    return buf.value.decode()


def format_messages(msgs, n):
    """ft8gpu_format_messages: "SNR DT Freq ~ Message", one line per record of msgs[0..n)"""
    L = load_library()
    msgs = np.ascontiguousarray(msgs)
    assert msgs.dtype == MESSAGE_DTYPE
    n = int(min(n, msgs.size))
    need = L.ft8gpu_format_messages(msgs.ctypes.data, n, None, 0)
    if need < 0:
        raise Ft8GpuError("ft8gpu_format_messages failed")
    buf = C.create_string_buffer(need + 1)
    L.ft8gpu_format_messages(msgs.ctypes.data, n, buf, len(buf))
    return buf.value.decode()


def refined_estimate(msgs, refined):
    """ft8gpu_refined_estimate for arrays of records of one shape -> (dt_s, freq_hz, snr_db, valid), float32 / bool arrays of that
    shape; where a record is not valid the three values are NaN"""
    L = load_library()
    msgs = np.ascontiguousarray(msgs)
    refined = np.ascontiguousarray(refined)
    assert msgs.dtype == MESSAGE_DTYPE and refined.dtype == REFINED_DTYPE and msgs.shape == refined.shape
    out = np.full((3,) + msgs.shape, np.nan, np.float32)
    ok = np.zeros(msgs.shape, bool)
    m, r = msgs.reshape(-1), refined.reshape(-1)
    o = out.reshape(3, -1)
    a, b, c = C.c_float(), C.c_float(), C.c_float()
    for i in range(m.size):
        if L.ft8gpu_refined_estimate(m[i:].ctypes.data, r[i:].ctypes.data, C.byref(a), C.byref(b), C.byref(c)) == 0:
            o[:, i] = (a.value, b.value, c.value)
            ok.reshape(-1)[i] = True
    return out[0], out[1], out[2], ok


def subtract_twiddles():
    """ft8gpu_subtract_twiddles: w4[i] = (cos, -sin)(2 pi i / 4096) as float32 [4096][2]"""
    L = load_library()
    out = np.zeros((SUBTRACT_TABLE, 2), np.float32)
    L.ft8gpu_subtract_twiddles(out.ctypes.data)
    return out


def audio_taps():
    """ft8gpu_audio_taps: the Kaiser low-pass of the audio front end as float32 [160]"""
    out = np.zeros(AUDIO_TAPS, np.float32)
    load_library().ft8gpu_audio_taps(out.ctypes.data)
    return out


def audio_mixer():
    """ft8gpu_audio_mixer: wm[i] = (cos, -sin)(2 pi i / 1920) as float32 [1920][2]"""
    out = np.zeros((AUDIO_MIX, 2), np.float32)
    load_library().ft8gpu_audio_mixer(out.ctypes.data)
    return out


def wide_mixer1():
    """ft8gpu_wide_mixer1: w1[i] = (lrint(32767 cos), -lrint(32767 sin))(2 pi i / 6000) as int16 [6000][2]"""
    out = np.zeros((WIDE_MIX1, 2), np.int16)
    load_library().ft8gpu_wide_mixer1(out.ctypes.data)
    return out


def wide_mixer2():
    """ft8gpu_wide_mixer2: w2[i] = (cos, -sin)(2 pi i / 3072) as float32 [3072][2]"""
    out = np.zeros((WIDE_MIX2, 2), np.float32)
    load_library().ft8gpu_wide_mixer2(out.ctypes.data)
    return out


def wide_taps():
    """ft8gpu_wide_taps: the second stage's low-pass of the wideband RX front end as float32 [96]"""
    out = np.zeros(WIDE_TAPS, np.float32)
    load_library().ft8gpu_wide_taps(out.ctypes.data)
    return out


def _pcm_d(D):
    if 3200 * int(D) not in PCM_RATES:
        raise Ft8GpuError(f"D = {D} is not one of 15, 30, 60, 120, 240")
    return int(D)


def pcm_mixer1(D):
    """ft8gpu_pcm_mixer1: w1[i] = (cos, -sin)(2 pi i / (16 D)) as float32 [16 D][2]"""
    out = np.zeros((16 * _pcm_d(D), 2), np.float32)
    load_library().ft8gpu_pcm_mixer1(int(D), out.ctypes.data)
    return out


def pcm_mixer2():
    """ft8gpu_pcm_mixer2: w2[i] = (cos, -sin)(2 pi i / 1536) as float32 [1536][2]"""
    out = np.zeros((PCM_MIX2, 2), np.float32)
    load_library().ft8gpu_pcm_mixer2(out.ctypes.data)
    return out


def pcm_taps_a(D):
    """ft8gpu_pcm_taps_a: the first stage's low-pass at 3200 D sps as float32 [8 (D / 3) + 1]"""
    out = np.zeros(8 * (_pcm_d(D) // 3) + 1, np.float32)
    assert load_library().ft8gpu_pcm_taps_a(int(D), out.ctypes.data) == out.shape[0]
    return out


def pcm_taps_b():
    """ft8gpu_pcm_taps_b: the second stage's low-pass at 9600 sps as float32 [48], 47 taps and a zero"""
    out = np.zeros(PCM_TAPS_B, np.float32)
    load_library().ft8gpu_pcm_taps_b(out.ctypes.data)
    return out


def read_wav_pcm(path, cap_bytes=8 * PCM_MAX_SAMPLES):
    """ft8gpu_read_wav_pcm: a .wav of 16-bit PCM or 32-bit float, one channel (real) or two (I, Q), at 48 .. 768 kHz ->
    (samples, format, rate): int16 or float32 [nsamples] (two channels: [2 * nsamples], interleaved), at most 15 s.  Anything else
    raises; the library names what it found on stderr."""
    cap = max(int(cap_bytes), 0)
    out = np.zeros(cap, np.uint8)
    fmt, rate, n = C.c_int(0), C.c_int(0), C.c_int32(0)
    if load_library().ft8gpu_read_wav_pcm(os.fsencode(path), out.ctypes.data, cap, C.byref(fmt), C.byref(rate), C.byref(n)) != 0:
        raise Ft8GpuError(f"{path}: not a readable PCM .wav of the PCM front end (the reason is on stderr)")
    dtype = np.float32 if fmt.value & PCM_F32 else np.int16
    count = n.value * (2 if fmt.value & PCM_COMPLEX else 1)
    return out[:count * np.dtype(dtype).itemsize].view(dtype).copy(), fmt.value, rate.value


def read_wav(path, cap=AUDIO_NSAMPLES):
    """ft8gpu_read_wav: a 12 kHz mono 16-bit PCM .wav -> int16 [min(samples, cap)].  Anything else raises; the library names
    what it found on stderr."""
    out = np.zeros(max(int(cap), 0), np.int16)
    n = C.c_int32(0)
    if load_library().ft8gpu_read_wav(os.fsencode(path), out.ctypes.data, int(cap), C.byref(n)) != 0:
        raise Ft8GpuError(f"{path}: not a readable 12000 Hz mono 16-bit PCM .wav (the reason is on stderr)")
    return out[:n.value].copy()


def gfsk_pulse(sps):
    """ft8gpu_gfsk_pulse: Q_sps[0 .. 3 sps] as uint32, the running sum of the Gaussian frequency pulse in units of 2^-32 turn"""
    out = np.zeros(3 * int(sps) + 1, np.uint32)
    if load_library().ft8gpu_gfsk_pulse(int(sps), out.ctypes.data) != 0:
        raise Ft8GpuError(f"gfsk_pulse: sps {sps} is neither {GFSK_SPS_IQ} nor {GFSK_SPS_AUDIO}")
    return out


def gfsk_ramp(sps):
    """ft8gpu_gfsk_ramp: r[k] = 0.5 (1 - cos(pi k / nr)) as float32 [nr], nr = sps / 8"""
    out = np.zeros(max(int(sps) // 8, 1), np.float32)
    if load_library().ft8gpu_gfsk_ramp(int(sps), out.ctypes.data) != 0:
        raise Ft8GpuError(f"gfsk_ramp: sps {sps} is neither {GFSK_SPS_IQ} nor {GFSK_SPS_AUDIO}")
    return out


def gfsk_twiddles():
    """ft8gpu_gfsk_twiddles: (gc, gf), (cos, sin)(2 pi i / 4096) and (cos, sin)(2 pi i / 2^24), float32 [4096][2] each"""
    gc, gf = np.zeros((GFSK_TWIDDLES, 2), np.float32), np.zeros((GFSK_TWIDDLES, 2), np.float32)
    load_library().ft8gpu_gfsk_twiddles(gc.ctypes.data, gf.ctypes.data)
    return gc, gf


def channel_preset(name, shape=()):
    """CHANNEL_DTYPE records of one of the presets "quiet", "moderate", "disturbed", "flutter" (FT8GPU_CHANNEL_*), or "none" """
    out = np.zeros(shape, CHANNEL_DTYPE)
    if name != "none":
        out["spread_hz"], out["delay_ms"], out["path2_gain"], out["mode"] = CHANNEL_PRESETS[name]
    return out


def channel_taps(seed, clip, signal, path, spread_hz):
    """ft8gpu_channel_taps: (gstep, theta), uint32 [16] each, of one (signal, path) of global clip `clip` """
    gstep, theta = np.zeros(CHANNEL_TAPS, np.uint32), np.zeros(CHANNEL_TAPS, np.uint32)
    if load_library().ft8gpu_channel_taps(int(seed), int(clip), int(signal), int(path), float(spread_hz), gstep.ctypes.data, theta.ctypes.data) != 0:
        raise Ft8GpuError(f"channel_taps: spread_hz {spread_hz} outside [0, 20] or path {path} outside (0, 1)")
    return gstep, theta


def channel_clip(mode, signals, channels, nsamples=AUDIO_NSAMPLES, seed=0, clip=0):
    """ft8gpu_channel_clip: the fading rule on the host for one clip, before noise and normalisation: signals [nsig] of
    SIGNAL_DTYPE, channels [nsig] of CHANNEL_DTYPE or None -> float32 [2][48000] (GFSK_IQ) or [nsamples] (GFSK_AUDIO)"""
    signals = np.ascontiguousarray(signals).reshape(-1)
    assert signals.dtype == SIGNAL_DTYPE
    cp = None
    if channels is not None:
        channels = np.ascontiguousarray(channels).reshape(-1)
        assert channels.dtype == CHANNEL_DTYPE and channels.size == signals.size
        cp = channels.ctypes.data
    out = np.zeros((2, NSAMPLES) if mode == GFSK_IQ else max(int(nsamples), 1), np.float32)
    if load_library().ft8gpu_channel_clip(int(mode), signals.ctypes.data, cp, signals.size, int(nsamples), int(seed), int(clip), out.ctypes.data) != 0:
        raise Ft8GpuError("channel_clip: an argument the synthesiser's entries refuse")
    return out


def write_wav(path, pcm):
    """ft8gpu_write_wav: int16 samples -> a 12 kHz mono 16-bit PCM .wav that read_wav reads back"""
    pcm = np.ascontiguousarray(pcm, np.int16).reshape(-1)
    if load_library().ft8gpu_write_wav(os.fsencode(path), pcm.ctypes.data, pcm.size) != 0:
        raise Ft8GpuError(f"{path}: could not be written (the reason is on stderr)")


def format_messages_refined(msgs, refined, n):
    """ft8gpu_format_messages_refined: "SNR DT Freq ~ Message" with DT to two decimals and Freq to one"""
    L = load_library()
    msgs = np.ascontiguousarray(msgs)
    refined = np.ascontiguousarray(refined)
    assert msgs.dtype == MESSAGE_DTYPE and refined.dtype == REFINED_DTYPE
    n = int(min(n, msgs.size, refined.size))
    need = L.ft8gpu_format_messages_refined(msgs.ctypes.data, refined.ctypes.data, n, None, 0)
    if need < 0:
        raise Ft8GpuError("ft8gpu_format_messages_refined failed")
    buf = C.create_string_buffer(need + 1)
    L.ft8gpu_format_messages_refined(msgs.ctypes.data, refined.ctypes.data, n, buf, len(buf))
    return buf.value.decode()


def ft8_subsystem(i_samples, q_samples, decodes=None):
    """The reference's own entry point (rtlsdr_ft8d.h:164) through the drop-in symbol."""
    L = load_library()
    i_samples = np.ascontiguousarray(i_samples, np.float32)
    q_samples = np.ascontiguousarray(q_samples, np.float32)
    if decodes is None:
        decodes = np.zeros(MAX_MESSAGES, RESULT_DTYPE)
    n = C.c_int32(0)
    L.ft8_subsystem(i_samples.ctypes.data, q_samples.ctypes.data, NSAMPLES, decodes.ctypes.data, C.byref(n))
    return decodes, n.value
