/*
 * ft8gpu.h -- C ABI of libft8gpu.so: the FT8 decode hot path of Guenael/rtlsdr-ft8d on one
 * AMD MI355X (gfx950), as hand-written HIP kernels behind the reference's own function boundary.
 *
 * Everything here is plain C: pointers, sizes, POD structs.  No HIP, torch or C++ types.
 * Every entry point names the reference interface it replaces (file:line into the reference).
 *
 * Frame conventions (identical to the reference, rtlsdr_ft8d.h:34-56, rtlsdr_ft8d.c:274-278):
 *   one frame = 15 s at 3200 sps = 48000 complex samples, planar float32: I[48000] then Q[48000].
 *   A batch is `nframes` such frames back to back: iq[nframes][2][48000].
 *   waterfall = uint8 mag[92][2][2][256] (block, time_sub, freq_sub, bin) = 94208 bytes per frame.
 *
 * Environment: FT8GPU_DEVICE=<n> is the GPU used by the drop-in ft8_subsystem (default 0; the reference's function has no
 * device argument).  Nothing else is read from the environment: every test hook is a per-context flag
 * (ft8gpu_set_debug_flags), so that behaviour never depends on the process environment.
 */
#ifndef FT8GPU_H
#define FT8GPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden; only the C ABI below is exported */
#pragma GCC visibility push(default)

/* ---- constants: rtlsdr_ft8d.h:34-56 ------------------------------------------------------- */
#define FT8GPU_NSAMPLES        48000   /* SIGNAL_LENGHT * SIGNAL_SAMPLE_RATE */
#define FT8GPU_K_MIN_SCORE     10      /* K_MIN_SCORE      rtlsdr_ft8d.h:43 */
#define FT8GPU_K_MAX_CANDIDATES 120    /* K_MAX_CANDIDATES rtlsdr_ft8d.h:44 */
#define FT8GPU_K_LDPC_ITERS    20      /* K_LDPC_ITERS     rtlsdr_ft8d.h:45 */
#define FT8GPU_K_MAX_MESSAGES  50      /* K_MAX_MESSAGES   rtlsdr_ft8d.h:46 */
#define FT8GPU_NUM_BIN         256     /* NUM_BIN          rtlsdr_ft8d.h:51 */
#define FT8GPU_NFFT            1024    /* NFFT             rtlsdr_ft8d.h:54 */
#define FT8GPU_NUM_BLOCKS      92      /* NUM_BLOCKS       rtlsdr_ft8d.h:55 */
#define FT8GPU_MAG_ARRAY       94208   /* MAG_ARRAY        rtlsdr_ft8d.h:56 */
#define FT8GPU_NN              79      /* FT8_NN (ft8_lib constants.h; used rtlsdr_ft8d.c:933,:947) */
#define FT8GPU_ABS_MAX_CANDIDATES 1024 /* upper bound accepted for ft8gpu_params.max_candidates */

/* ---- ABI structs --------------------------------------------------------------------------- */

/* struct decoder_results, rtlsdr_ft8d.h:136-141 (offsets 0/13/20/24, size 28).  The name is kept
 * so that rtlsdr_ft8d.c compiles against this header unchanged. */
#ifndef FT8GPU_NO_DECODER_RESULTS
struct decoder_results {
    char    call[13];
    char    loc[7];
    int32_t freq;
    int32_t snr;
};
#endif

/* candidate_t of ft8_lib decode.h, as used at rtlsdr_ft8d.c:1439, :1466-1470 (8 bytes) */
typedef struct {
    int16_t score;
    int16_t time_offset;
    int16_t freq_offset;
    uint8_t time_sub;
    uint8_t freq_sub;
} ft8gpu_candidate;

/* Per-candidate outcome of ft8_decode(): message_t + decode_status_t of ft8_lib decode.h
 * (rtlsdr_ft8d.c:1474-1487, :1494) folded into one 48-byte record, plus the packed 91 bits. */
typedef struct {
    int16_t  ldpc_errors;     /* decode_status_t.ldpc_errors (min parity errors seen, 0 = codeword) */
    int16_t  iters;           /* BP iterations entered before exit (diagnostic) */
    uint16_t crc_extracted;   /* valid when ldpc_errors == 0 */
    uint16_t crc_calculated;  /* valid when ldpc_errors == 0 */
    int8_t   unpack_status;   /* valid when CRCs match; < 0 = unpack77 failed */
    uint8_t  ok;              /* 1 iff ft8_decode() would have returned true */
    uint8_t  a91[12];         /* packed payload+CRC bits of the last hard decision */
    char     text[25];        /* message_t.text (valid when ok) */
    uint8_t  pad;
} ft8gpu_decode_status;

/* run-time forms of K_MIN_SCORE / K_MAX_CANDIDATES / K_LDPC_ITERS (rtlsdr_ft8d.h:43-45) */
typedef struct {
    int32_t min_score;
    int32_t max_candidates;
    int32_t ldpc_iters;
} ft8gpu_params;

typedef struct ft8gpu_ctx ft8gpu_ctx;

/* flags for the batch entry points */
#define FT8GPU_HOST_PTRS    0   /* all array arguments are host memory; copies are staged by the library */
#define FT8GPU_DEVICE_PTRS  1   /* all array arguments are device (HBM) pointers on the context's GPU */

/* per-stage kernel timings of ft8gpu_decode_batch(), hipEvent-measured on the context stream and
 * averaged over the pipeline runs recorded since ft8gpu_enable_timing(ctx, 1) (ring of 32 runs;
 * recording does not synchronise the host) */
typedef struct {
    float waterfall_ms;
    float sync_ms;        /* score + compaction */
    float heap_ms;        /* top-N selection (exact heap replay) */
    float decode_ms;      /* LLR + LDPC BP + CRC + unpack */
    float spots_ms;       /* dedup + CQ spot fill */
    float total_ms;       /* first kernel start to last kernel end */
    int32_t launches_per_stage; /* 1, or 2 when a large batch is processed as two overlapped parts (the first quarter and the
                                   rest): the heap replay of one part then runs on a side stream under the other part's
                                   kernels, and the per-stage figures are sums over both launches of a stage (the spot
                                   collection is one launch for both parts) */
} ft8gpu_timings;

/* ---- lifecycle: replaces initFFTW()/freeFFTW(), rtlsdr_ft8d.c:314-347 ----------------------- */

/* Creates a decoder context on GPU `device` with persistent buffers for up to `max_frames` frames
 * (larger batches are processed in chunks of max_frames).  `params` may be NULL (reference defaults
 * 10 / 120 / 20).  Returns 0 on success.  A context owns its intermediate buffers; every entry point
 * holds the context's mutex, so two host threads calling into ONE context serialise (use one context
 * per thread / per GPU for concurrency: contexts are independent, unlike the reference's process-global
 * FFTW state, rtlsdr_ft8d.c:57-60).  Entry points make the context's GPU current for their duration and
 * restore the caller's current device before returning.
 * ft8gpu_destroy waits for the context's streams and frees everything the context allocated.  It takes no lock: destroying a
 * context while any entry on it is still running (on another thread, or inside a multi-context call) is a caller error. */
int  ft8gpu_create(ft8gpu_ctx **out, int device, int max_frames, const ft8gpu_params *params);
void ft8gpu_destroy(ft8gpu_ctx *ctx);
/* Use an existing hipStream_t (passed as void*) for all work of this context.  NULL = the context
 * creates its own non-blocking stream; FT8GPU_STREAM_LEGACY (= hipStreamLegacy) selects the legacy
 * null stream explicitly.  The call synchronises the old and the new stream and runs the co-execution probe of
 * ft8gpu_overlap_active on the new one (a few one-thread kernels and host synchronisations, well under a millisecond
 * when the streams co-run): do not call it on a stream that is being captured into a graph. */
int  ft8gpu_set_stream(ft8gpu_ctx *ctx, void *hip_stream);
#define FT8GPU_STREAM_LEGACY ((void *)1)
/* The hipStream_t (as void*) the context enqueues on, so that a caller can order its own work behind the decoder's
 * (hipStreamWaitEvent / an RCCL collective) without moving the decoder onto a foreign stream: the context's streams
 * are created together and map to distinct hardware queues, which the overlap of the heap / spots kernels with the
 * throughput kernels relies on (measured: the same pipeline takes 1.48 ms on a borrowed framework stream against 1.28 ms
 * on the context's own at 1024 frames, cap 480). */
void *ft8gpu_get_stream(ft8gpu_ctx *ctx);
/* 1: batches of >= 512 frames run the two-part pipeline with the serial kernels (heap replay, spot collection) on side
 * streams under the throughput kernels of the other part; 0: plain pipeline, one launch per stage.  Whether streams run
 * side by side depends on which hardware queues HIP hands out, so the context measures it at ft8gpu_create and again at
 * ft8gpu_set_stream (a 2 ms co-execution probe per pair of streams), replaces side streams that share a queue with another
 * one, and only falls back when that does not help.  Records are identical either way.  A pure query: it does not touch
 * ft8gpu_last_error().  The probe is a timing measurement: on a GPU shared with other work, or under a profiler that
 * serialises kernels, it can come out 0 -- ft8gpu_overlap_reason says why. */
int  ft8gpu_overlap_active(ft8gpu_ctx *ctx);
/* why the plain pipeline runs ("" while the overlapped one is active), copied into buf (NUL-terminated, truncated to cap) */
int  ft8gpu_overlap_reason(ft8gpu_ctx *ctx, char *buf, size_t cap);
/* test hooks, per context (any combination; 0 = product behaviour) */
#define FT8GPU_DBG_FORCE_IEEE_DIV 1u  /* LDPC kernel: the compiler's IEEE division everywhere (the guard's fallback path) */
#define FT8GPU_DBG_PIPELINE_FORM  2u  /* ft8gpu_decode_candidates runs the form of the LDPC kernel ft8gpu_decode_batch
                                         uses (no exact error count: ldpc_errors is 0 or 83) */
#define FT8GPU_DBG_NO_OVERLAP     4u  /* one launch per stage for the whole batch: no two-half overlap, no chunked upload */
#define FT8GPU_DBG_ALL            7u
/* (Alternative, bit-identical forms of the waterfall and heap kernels are not in this library: they are compiled into the
 * A/B build only -- `make -C rtlsdr_ft8d_amd/csrc ab` -> libft8gpu_ab.so, whose ft8gpu_set_debug_flags accepts the extra
 * selector bits of csrc/ft8gpu_internal.h.) */
int  ft8gpu_set_debug_flags(ft8gpu_ctx *ctx, unsigned flags);   /* unknown bits are refused */
/* Identity of the build: "<dev>.<all>[+ab]" -- 16 hex digits of SHA-256 over the device sources (csrc/ *.hip, *.h) and 16 over
 * every source of the library (those + csrc/ *.c, Makefile, include/), computed by the Makefile when the library is
 * linked.  rtlsdr_ft8d_amd.source_build_id() recomputes it from the tree: smoke(), the GPU tests and bench.py refuse a
 * library whose id differs from the sources beside it (a stale or foreign .so fails instead of producing numbers). */
const char *ft8gpu_build_id(void);
/* Proof by exhaustion behind the LDPC kernel's short division chains (csrc/bp_math.h): fast_tanh / fast_atanh of
 * ft8_lib ldpc.c (reached through ft8_decode, rtlsdr_ft8d.c:1476) are functions of one float, so all 2^32 inputs are
 * evaluated on the GPU, fast form against the compiler's IEEE-754 division, on the domain the kernel's guard
 * establishes.  out[0..6] = tanh inputs, tanh mismatches, atanh inputs, atanh mismatches, packed-form mismatches,
 * float bits of max |fast_tanh|, one offending input pattern (0 = none).  About 40 ms. */
int  ft8gpu_selftest_bp_math(ft8gpu_ctx *ctx, uint64_t out[7]);
/* The same kind of proof for the scale factor of the soft bits, sqrtf(24.0f / variance) (ftx_normalize_logl of ft8_lib decode.c,
 * reached through ft8_decode, rtlsdr_ft8d.c:1476): for every float v in [2^-60, 2^60] the quotient and the root the LDPC kernel
 * computes are checked against exact arithmetic (products and squares that are exact in double), not against another
 * division or root.  The same exact test is applied to the divisions of fast_tanh / fast_atanh themselves on their whole
 * domains -- the "IEEE quotient" ft8gpu_selftest_bp_math compares the short chains with.  out[0..6] = inputs, quotients 24/v not
 * correctly rounded, roots not correctly rounded, kernel function != sqrtf(24.0f / v), one offending input pattern (0 = none),
 * rational-function divisions tested, of those not correctly rounded.  (Round 5: HIP's __fsqrt_rn turned out to be the 1-ulp
 * native root.) */
int  ft8gpu_selftest_norm_math(ft8gpu_ctx *ctx, uint64_t out[7]);
/* The same kind of proof for the dB quantiser of the waterfall kernel (rtlsdr_ft8d.c:1415-1427; csrc/quant_math.h), which does not
 * evaluate the reference's log10f expression but a v_log_f32 guess and one compare against a threshold table built at
 * ft8gpu_create.  One kernel walks every |X|^2 bit pattern the waterfall kernel can produce -- 0x00000000 .. 0x7F800000 (0 .. +inf)
 * and every NaN of both signs; a sum of two squares is never negative -- through the kernel's own functions and this context's
 * uploaded table, in both slots of the packed pair and beside partners from elsewhere in the domain, and returns the step function:
 * step_bits[k] = the k-th pattern b (ascending) with q(b) != q(b - 1), step_val[k] = q(b); at most min(cap, 4096) entries are
 * written.  out[0..6] = number of steps (the true count, also when it exceeds what was written), q(0), NaN patterns not quantised
 * to 0, evaluations of one pattern that disagree, results that were the guess, results that were the guess + 1, one offending
 * pattern (0 = none).  qthr[0..255] = the threshold table as it lies on the device.  Equal step lists and equal q(0) on the
 * device and in the reference expression mean equal bytes for every float; the tests hold them against the CPU oracle.  About
 * 6 ms. */
int  ft8gpu_selftest_quantiser(ft8gpu_ctx *ctx, uint64_t out[7], uint32_t *step_bits, uint8_t *step_val, int32_t cap, float qthr[256]);
int  ft8gpu_set_params(ft8gpu_ctx *ctx, const ft8gpu_params *params);
int  ft8gpu_enable_timing(ft8gpu_ctx *ctx, int on);
int  ft8gpu_get_timings(ft8gpu_ctx *ctx, ft8gpu_timings *out, int32_t *nruns);
int  ft8gpu_synchronize(ft8gpu_ctx *ctx);
/* The reference path has no error channel (void ft8_subsystem, rtlsdr_ft8d.h:164); failures are
 * reported here and by the int return codes of the batch API (0 = ok, <0 = error). */
const char *ft8gpu_last_error(void);
int  ft8gpu_device_count(void);

/* ---- the whole path: ft8_subsystem(), rtlsdr_ft8d.c:1387-1524, for `nframes` frames ----------
 * decodes:   [nframes][50] struct decoder_results.  Exactly as the reference (:1509-1520), slot k
 *            of a frame is written only if the k-th unique message of that frame starts with "CQ";
 *            other slots are left untouched.  n_results[f] = number of unique messages (:1523).
 * Fences (documented deviations where the reference is undefined): more than 50 unique messages
 * in a frame -> the surplus is dropped (reference: infinite loop); missing tokens -> "(null)". */
int ft8gpu_decode_batch(ft8gpu_ctx *ctx, const float *iq, int nframes,
                        struct decoder_results *decodes, int32_t *n_results, int flags);

/* ---- the same across several GPUs of one node, for a plain C caller ------
 * ctxs[0..ndev): one context per GPU (normally ft8gpu_create(&ctxs[g], g, ...); several contexts on one
 * GPU are legal).  Frames are independent, so the batch is cut into ndev contiguous shards (shard g =
 * frames [g*n/ndev, (g+1)*n/ndev)), each decoded by its own host thread on its own context, and every
 * shard's records land directly at their frame offsets in the caller's HOST arrays -- the gather of the
 * 1 404 B/frame spot records is that placement; no collective is needed when the list is consumed on
 * the host, as the daemon does.  iq / decodes / n_results are host memory (FT8GPU_HOST_PTRS layout of
 * ft8gpu_decode_batch; take them from ft8gpu_host_alloc when throughput matters: uploads from pageable memory are
 * staged and do not overlap the kernels).  Returns 0, or -1 with ft8gpu_last_error() naming the failing shard. */
int ft8gpu_decode_batch_multi(ft8gpu_ctx *const *ctxs, int ndev, const float *iq, int nframes,
                              struct decoder_results *decodes, int32_t *n_results);
/* Device-resident form: shard g's frames already sit in HBM of ctxs[g]'s GPU (iq_dev[g]: [nframes_dev[g]][2][48000],
 * e.g. synthesised or decimated there); records are gathered into the host arrays in shard order. */
int ft8gpu_decode_batch_multi_dev(ft8gpu_ctx *const *ctxs, int ndev, const float *const *iq_dev,
                                  const int *nframes_dev, struct decoder_results *decodes, int32_t *n_results);

/* Device-resident gather of the spot list over RCCL / xGMI: after every GPU g has decoded its shard
 * into its own HBM (ft8gpu_decode_batch with FT8GPU_DEVICE_PTRS: decodes_dev[g] = [frames_per_dev][50] records,
 * n_results_dev[g] = [frames_per_dev] counts), ONE grouped all-gather per buffer leaves the whole job's list, in shard
 * order, on EVERY GPU: all_decodes_dev[g] = [ndev * frames_per_dev][50], all_n_results_dev[g] = [ndev * frames_per_dev].
 * The collectives are enqueued on each context's own stream (ordered behind the kernels that produced the records; the
 * host is not synchronised: ft8gpu_synchronize(ctxs[g]) waits).  Single-process RCCL (ncclCommInitAll over the contexts'
 * devices, created on first use, one rank per GPU -- two contexts on one GPU are refused); librccl is bound at run time,
 * so -1 with "RCCL unavailable" on a box without it.  Equal shard sizes only (pad the last shard).  Replaces nothing in
 * the reference (single decoder thread, rtlsdr_ft8d.c:221-285); the host-side gather of ft8gpu_decode_batch_multi is what
 * a daemon consumes.  ft8gpu_gather_shutdown() destroys the communicators. */
int  ft8gpu_gather_spots(ft8gpu_ctx *const *ctxs, int ndev, const struct decoder_results *const *decodes_dev,
                         const int32_t *const *n_results_dev, int frames_per_dev,
                         struct decoder_results *const *all_decodes_dev, int32_t *const *all_n_results_dev);
void ft8gpu_gather_shutdown(void);
/* host worker threads the multi-GPU entries keep alive between calls (created on first use; diagnostic) */
int  ft8gpu_shard_workers(void);

/* ---- stage entries (same data, stage by stage; used by the parity tests) --------------------- */
/* rtlsdr_ft8d.c:1395-1435: window, 184 FFTs, log-magnitude, quantise.  mag: [nframes][94208] */
int ft8gpu_waterfall(ft8gpu_ctx *ctx, const float *iq, int nframes, uint8_t *mag, int flags);
/* ft8_find_sync(&power, K_MAX_CANDIDATES, candidate_list, K_MIN_SCORE), rtlsdr_ft8d.c:1450.
 * cands: [nframes][max_candidates], counts: [nframes] */
int ft8gpu_find_sync(ft8gpu_ctx *ctx, const uint8_t *mag, int nframes,
                     ft8gpu_candidate *cands, int32_t *counts, int flags);
/* every sync score of the scan, int16 [nframes][2][2][36][249] (diagnostic / parity) */
int ft8gpu_score_map(ft8gpu_ctx *ctx, const uint8_t *mag, int nframes, int16_t *scores, int flags);
/* ft8_decode(&power, cand, &message, K_LDPC_ITERS, &status) for every candidate, :1476.
 * status: [nframes][max_candidates] */
int ft8gpu_decode_candidates(ft8gpu_ctx *ctx, const uint8_t *mag, const ft8gpu_candidate *cands,
                             const int32_t *counts, int nframes, ft8gpu_decode_status *status, int flags);
/* dedup hash table + CQ filter + spot fill, rtlsdr_ft8d.c:1452-1460, :1487-1523 */
int ft8gpu_collect_spots(ft8gpu_ctx *ctx, const ft8gpu_candidate *cands, const int32_t *counts,
                         const ft8gpu_decode_status *status, int nframes,
                         struct decoder_results *decodes, int32_t *n_results, int flags);

/* ---- every decoded message with SNR, time offset and frequency (a second output path beside the reference's) ----------
 * ft8gpu_decode_batch keeps the reference's contract: only CQ messages reach a record, and decoder_results.snr is the sync
 * score (rtlsdr_ft8d.c:1509-1520; the reference itself notes "score != snr", :1517).  The entries below number the unique
 * messages of a frame exactly as that path does (:1487-1520, the same dedup, order and cap of 50, so n_msgs[f] ==
 * n_results[f] for the same input and parameters) and write one record for EVERY one of them, CQ or not.
 * How the stage entries below (and ft8gpu_collect_spots) read a caller-made list: candidate idx of frame f is looked at when
 * idx < max_candidates && idx < counts[f], so a count below 0 reads as 0 and one above max_candidates as max_candidates; a
 * candidate counts when its score >= min_score and its status record's ok is NON-ZERO (any of 1..255); two candidates carry
 * the same message when crc_extracted (all 16 bits) and the text up to its first NUL (all 25 bytes if there is none) agree.
 * The tones under which the signal is measured (and which the mask and the refinement rebuild) are "re-encoded from a91":
 * ALL 91 BITS AS STORED -- the 77 payload bits and the 14 bits of the CRC field the record carries, not a CRC recomputed
 * from the payload -- through the generator, the Gray map and the Costas arrays; the low five bits of a91[11] play no
 * part and are copied into the record as they are.  For a record the LDPC kernel wrote the two readings are the same. */
typedef struct {
    char     text[25];       /*  0  message_t.text, as the LDPC kernel unpacked it (== ft8gpu_decode_status.text) */
    int8_t   snr_db;         /* 25  estimated SNR in 2500 Hz, integer dB, [-30, 49] (DESIGN.md "Every decoded message");
                              *     49 when no symbol of the signal lies inside the waterfall (time_offset <= -79 or >= 92:
                              *     the empty sum meets every threshold, 0 >= 0) */
    int16_t  score;          /* 26  sync score: what decoder_results.snr carries */
    float    freq_hz;        /* 28  (freq_offset + (float)freq_sub / 2) * 6.25f, rtlsdr_ft8d.c:1470, before the int cast */
    float    dt_s;           /* 32  (time_offset + (float)time_sub / 2) / 6.25f, the formula of rtlsdr_ft8d.c:1471, in float */
    uint16_t hash;           /* 36  message.hash (crc_extracted) */
    uint16_t cand_index;     /* 38  index in the frame's candidate list of the first candidate that carried the message */
    ft8gpu_candidate cand;   /* 40  that candidate */
    uint8_t  a91[12];        /* 48  its packed payload + CRC */
    uint8_t  pad[4];         /* 60  zero */
} ft8gpu_message;
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_message) == 64, "ft8gpu_message is 64 bytes");
_Static_assert(offsetof(ft8gpu_message, snr_db) == 25 && offsetof(ft8gpu_message, score) == 26 &&
               offsetof(ft8gpu_message, freq_hz) == 28 && offsetof(ft8gpu_message, dt_s) == 32 &&
               offsetof(ft8gpu_message, hash) == 36 && offsetof(ft8gpu_message, cand_index) == 38 &&
               offsetof(ft8gpu_message, cand) == 40 && offsetof(ft8gpu_message, a91) == 48 &&
               offsetof(ft8gpu_message, pad) == 60, "ft8gpu_message field offsets");
#else
static_assert(sizeof(ft8gpu_message) == 64, "ft8gpu_message is 64 bytes");
static_assert(offsetof(ft8gpu_message, snr_db) == 25 && offsetof(ft8gpu_message, score) == 26 &&
              offsetof(ft8gpu_message, freq_hz) == 28 && offsetof(ft8gpu_message, dt_s) == 32 &&
              offsetof(ft8gpu_message, hash) == 36 && offsetof(ft8gpu_message, cand_index) == 38 &&
              offsetof(ft8gpu_message, cand) == 40 && offsetof(ft8gpu_message, a91) == 48 &&
              offsetof(ft8gpu_message, pad) == 60, "ft8gpu_message field offsets");
#endif
/* The whole path for a batch, host or device pointers, chunked by max_frames like ft8gpu_decode_batch.
 * msgs: [nframes][50], n_msgs: [nframes].  Frame f gets its unique messages in the reference's order in slots
 * 0..n_msgs[f]-1; slots n_msgs[f]..49 are left untouched.  ft8gpu_enable_timing: spots_ms then holds the noise
 * baseline and message kernels. */
int ft8gpu_decode_messages(ft8gpu_ctx *ctx, const float *iq, int nframes, ft8gpu_message *msgs, int32_t *n_msgs, int flags);
/* stage entry, the counterpart of ft8gpu_collect_spots: mag [nframes][94208], cands / status [nframes][max_candidates],
 * counts [nframes] -> msgs [nframes][50], n_msgs [nframes] */
int ft8gpu_collect_messages(ft8gpu_ctx *ctx, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                            const ft8gpu_decode_status *status, int nframes, ft8gpu_message *msgs, int32_t *n_msgs, int flags);
/* per-frame noise floor of the SNR estimate: base[f][fs][j] = the 47th smallest (index 46) of the 184 bytes
 * mag[f][b][ts][fs][j] over b < 92, ts < 2 (the 25th percentile over time).  base: [nframes][2][256] */
int ft8gpu_noise_baseline(ft8gpu_ctx *ctx, const uint8_t *mag, int nframes, uint8_t *base, int flags);
/* ---- multi-pass decoding: decode again after the decoded signals are masked out of the waterfall ----------------------
 * (DESIGN.md "Multi-pass decoding").  Pass 1 is ft8gpu_decode_messages, unchanged: waterfall W1, its noise baseline B
 * (ft8gpu_noise_baseline), records [0, n1).  Pass p+1 masks W(p): for every symbol k of every record first written in
 * pass p, the cell mag[(to+k)*1024 + ts*512 + fs*256 + fo + tone_k] with 0 <= to+k < 92 takes the baseline B[fs][fo + tone_k]
 * ((to, ts, fo, fs) = the record's cand with ts, fs taken mod 2 and fo clamped to [0, 248]; tone_k re-encoded from a91).
 * It then runs find_sync, the candidate heap and the LDPC decode on the masked waterfall with the context's params, and
 * appends, in candidate order, every unique message (hash, text) that is not yet among the frame's records, up to 50 in
 * all.  An appended record is built as ft8gpu_decode_messages builds one (cand_index indexes this pass's candidate list);
 * its snr_db is measured on the masked waterfall against the pass-1 baseline.  A frame that gained nothing in pass p, or
 * holds 50 records, is not decoded again.  Slots [0, n1) are those of ft8gpu_decode_messages; counts never shrink. */
#define FT8GPU_MAX_PASSES 4
/* passes in [1, FT8GPU_MAX_PASSES]; msgs [nframes][50], n_msgs [nframes] as ft8gpu_decode_messages (slots >= n_msgs[f]
 * untouched); n_by_pass [nframes][passes]: the count after each pass (NULL: not written).  Host or device pointers,
 * chunked by max_frames.  The host reads one int per later pass (the number of frames still decoding) and stops early at 0.
 * ft8gpu_enable_timing records the first pass. */
int ft8gpu_decode_messages_passes(ft8gpu_ctx *ctx, const float *iq, int nframes, int passes, ft8gpu_message *msgs,
                                  int32_t *n_msgs, int32_t *n_by_pass, int flags);
/* stage entry of the mask: mag_out[f] = mag[f] with the cells of records [first[f], n_msgs[f]) (clamped to [0, 50]) set to
 * the baseline.  mag / mag_out [nframes][94208] (mag_out may be mag), base [nframes][2][256], msgs [nframes][50],
 * first / n_msgs [nframes] */
int ft8gpu_mask_messages(ft8gpu_ctx *ctx, const uint8_t *mag, const uint8_t *base, const ft8gpu_message *msgs,
                         const int32_t *first, const int32_t *n_msgs, int nframes, uint8_t *mag_out, int flags);
/* stage entry of the append: mag = the pass's waterfall, base = the pass-1 baseline, cands / counts / status = the pass's
 * stage outputs ([nframes][max_candidates]); msgs / n_msgs are in-out: the frame's records so far (n_msgs[f] clamped to
 * [0, 50]), and the new ones appended behind them */
int ft8gpu_append_messages(ft8gpu_ctx *ctx, const uint8_t *mag, const uint8_t *base, const ft8gpu_candidate *cands,
                           const int32_t *counts, const ft8gpu_decode_status *status, int nframes, ft8gpu_message *msgs,
                           int32_t *n_msgs, int flags);
/* ---- ordered-statistics decoding (OSD) of the candidates belief propagation gives up on --------------------------------
 * (DESIGN.md "Ordered-statistics decoding"; not in the reference, whose ft8_decode, rtlsdr_ft8d.c:1476, stops at BP.)
 * A candidate whose status record has ok == 0 and ldpc_errors != 0 is decoded again from llr[0..173], the normalised soft
 * bits BP starts from; a non-finite value means no attempt (result 6).  The rule is exact:
 *   h[i] = llr[i] > 0;  w[i] = 255 if |llr[i]| >= 32.0f, else (int)(|llr[i]| * 8.0f)
 *   positions sorted by the bit pattern of |llr[i]| as uint32, descending, ties by ascending i
 *   G = the 91 x 174 generator (row k = the codeword of the message whose only set bit is k).  Walking its columns in the
 *   sorted order, a column independent of the pivots so far becomes a pivot, up to 91; full reduction; R_k = the reduced
 *   row with a 1 in the k-th pivot column (k = 0 the most reliable)
 *   pattern 0 = c0 = XOR of the R_k whose pivot position has h = 1; order >= 1 adds 1 + k = c0 ^ R_k (k = 0..90); order 2
 *   adds 92 + rank(i, j) = c0 ^ R_i ^ R_j, i < j in lexicographic order (4187 patterns in all)
 *   metric = sum of w over the positions where a pattern differs from h, nhard = their number; the best pattern has the
 *   smallest metric, ties go to the smallest index
 * Only the best pattern is judged; the first failing check names the result: 5 all-zero, 2 nhard > max_hard_errors,
 * 3 CRC-14 mismatch, 4 unpack77 < 0, else 1 = accepted.  On acceptance the status record becomes that of a BP success
 * (ok = 1, ldpc_errors = 0, CRC fields, unpack_status, a91, text; iters as it was); otherwise it is unchanged. */
typedef struct {
    uint8_t  result;         /* 0 not attempted, 1 accepted, 2..5 the failing check, 6 non-finite soft bits (nothing searched) */
    uint8_t  nhard;          /* the best pattern's values, accepted or not */
    uint16_t pattern;
    int32_t  metric;
} ft8gpu_osd_info;
/* Recommended max_hard_errors, from profiles/osd_gain.json (96 frames of 20 signals at -22..0 dB): at 27, order 1 keeps 17
 * of the 32 messages OSD gains without a gate and order 2 keeps 30 of 45, and 232 / 955 of about 7100 failing candidates have
 * a wrong best pattern within the gate -- each passes the CRC with probability 2^-14: 1.5e-4 / 6.1e-4 expected false
 * decodes per frame.  At 31 those are 1.1e-3 / 2.4e-3 (DESIGN.md has the sweep). */
#define FT8GPU_OSD_MAX_HARD_ERRORS 27
/* stage entry: mag [nframes][94208], cands / status_in / status_out / info [nframes][max_candidates], counts [nframes].
 * order in [0, 2], max_hard_errors in [0, 83].  Records below counts[f] are written (a candidate that does not qualify:
 * status_out = status_in, info all zero), records at and behind it are not touched.  status_out may be status_in. */
int ft8gpu_osd_candidates(ft8gpu_ctx *ctx, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                          const ft8gpu_decode_status *status_in, int nframes, int order, int max_hard_errors,
                          ft8gpu_decode_status *status_out, ft8gpu_osd_info *info, int flags);
/* The whole path with OSD behind every pass.  Each pass runs as in ft8gpu_decode_messages_passes (sync, heap, LDPC, collect
 * or append); then OSD runs on that pass's failures and the append step adds, in candidate order, the unique messages it
 * gained (pad[0] of such a record = the pattern's nhard, >= 1; BP records keep 0).  The mask of the next pass uses all
 * records so far.  n_by_stage [nframes][passes][2] (NULL: not written): the count after BP and after OSD of each pass.
 * osd_order -1: no OSD, the records are those of ft8gpu_decode_messages_passes.  With passes = 1 the slots below the BP
 * count are those of ft8gpu_decode_messages. */
typedef struct {
    int32_t passes;                 /* 1 .. FT8GPU_MAX_PASSES */
    int32_t osd_order;              /* -1 (no OSD), 0, 1, 2 */
    int32_t osd_max_hard_errors;    /* 0 .. 83; FT8GPU_OSD_MAX_HARD_ERRORS is the recommended value */
} ft8gpu_deep_params;
int ft8gpu_decode_messages_deep(ft8gpu_ctx *ctx, const float *iq, int nframes, const ft8gpu_deep_params *params,
                                ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags);
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_osd_info) == 8 && offsetof(ft8gpu_osd_info, nhard) == 1 && offsetof(ft8gpu_osd_info, pattern) == 2 &&
               offsetof(ft8gpu_osd_info, metric) == 4, "ft8gpu_osd_info layout");
_Static_assert(sizeof(ft8gpu_deep_params) == 12 && offsetof(ft8gpu_deep_params, osd_order) == 4 &&
               offsetof(ft8gpu_deep_params, osd_max_hard_errors) == 8, "ft8gpu_deep_params layout");
#else
static_assert(sizeof(ft8gpu_osd_info) == 8 && offsetof(ft8gpu_osd_info, nhard) == 1 && offsetof(ft8gpu_osd_info, pattern) == 2 &&
              offsetof(ft8gpu_osd_info, metric) == 4, "ft8gpu_osd_info layout");
static_assert(sizeof(ft8gpu_deep_params) == 12 && offsetof(ft8gpu_deep_params, osd_order) == 4 &&
              offsetof(ft8gpu_deep_params, osd_max_hard_errors) == 8, "ft8gpu_deep_params layout");
#endif
/* ---- a-priori (AP) decoding: BP once more with known message bits fixed ---------------------------------------------------
 * (DESIGN.md "A-priori decoding"; not in the reference, whose ft8_decode, rtlsdr_ft8d.c:1476, runs BP once.  The reference
 * reports CQ calls only, rtlsdr_ft8d.c:1509-1520, and 32 of the 77 payload bits of "CQ CALL GRID" are the same every time.)
 * A hypothesis is 77 payload bits with a mask, both numbered as in a91, MSB first.  Bits 77..79 of both arrays are zero,
 * bits & ~mask == 0, and between 1 and 77 bits are masked; anything else is refused with an error message.  Codeword
 * positions 0..76 are the payload bits (the code is systematic).
 * A candidate qualifies as for OSD: its status record has ok == 0 and ldpc_errors != 0 (either form of the LDPC kernel).
 * llr[0..173] = the normalised soft bits BP starts from, in the LDPC kernel's arithmetic; h[i] = llr[i] > 0;
 * apmag = max |llr[i]|.  A non-finite llr[i], or apmag == 0: nothing is tried, result 6.
 * Hypotheses are tried in table order k = 0 .. nhyp - 1:
 *   llr_k[i] = bits_k[i] ? +apmag : -apmag on the masked positions, llr[i] elsewhere
 *   ft8_lib's bp_decode(llr_k, ldpc_iters) runs as in the LDPC kernel; nhard = the number of unmasked positions at which
 *   the word it leaves differs from h; iters = its iteration count (255 for more)
 *   the first failing check names the hypothesis's result: 7 no codeword within ldpc_iters, 8 the codeword differs from the
 *   hypothesis on a masked position, 5 all-zero, 2 nhard > max_hard_errors, 3 CRC-14 mismatch, 4 unpack77 < 0, else
 *   1 = accepted.  (bp_decode leaves at an all-zero word before checking it, so such a word is "no codeword", 7; 5 keeps
 *   its place for a decoder that would hand one over.)
 * The first accepted hypothesis wins; later ones are not tried and their results[] stay 0.  On acceptance the status record
 * becomes that of a BP success, as OSD writes it (ok = 1, ldpc_errors = 0, CRC fields, unpack_status, a91, text; iters as it
 * was); otherwise it is unchanged.  The rule is defined per (candidate, hypothesis): a wave per pair plus a resolve step would
 * give the same bytes as the loop inside a wave. */
#define FT8GPU_AP_MAX_HYPOTHESES 4
typedef struct { uint8_t mask[10]; uint8_t bits[10]; } ft8gpu_ap_hypothesis;
typedef struct {
    uint8_t result;          /* 0 not attempted, 1 accepted, 2..5, 7, 8 the failing check, 6 unusable soft bits (nothing tried) */
    uint8_t nhard;           /* result, nhard, iters: of hypothesis `hyp` */
    uint8_t hyp;             /* the accepted hypothesis, or the last one tried */
    uint8_t iters;
    uint8_t results[FT8GPU_AP_MAX_HYPOTHESES];    /* the code of every hypothesis tried, 0 for the others */
} ft8gpu_ap_info;
/* Recommended max_hard_errors, from profiles/ap_gain.json (tools/ap_gain.py: six workloads of 96 frames, 33 127 failing
 * candidates).  Under "CQ ? ?" BP converges on 469 words that agree with the hypothesis: 463 planted codewords with 6 .. 35
 * hard errors (one of 45 that gains nothing), and 6 wrong words with 20, 25, 25, 26, 26, 26 -- inside the range of the right
 * ones, so the gate separates nothing: on 96 frames of 20 CQ signals it costs 13 of the 42 gained messages at 20 and 2 at 25
 * while it still admits the wrong words.  40 is the smallest gate of the sweep that loses no message in any row, and it only
 * cuts the tail.  What keeps false decodes out is that a wrong word must satisfy 83 parity checks, agree with the forced
 * bits, and then pass the 14-bit CRC: 6 / 2^14 = 4e-4 expected false decodes in those 576 frames. */
#define FT8GPU_AP_MAX_HARD_ERRORS 40
/* stage entry: mag [nframes][94208], cands / status_in / status_out / info [nframes][max_candidates], counts [nframes];
 * host or device pointers by `flags`, hyps [nhyp] always in host memory.  nhyp in [1, 4], max_hard_errors in [0, 174];
 * ldpc_iters is the context's.  Records below counts[f] are written (a candidate that does not qualify: status_out =
 * status_in, info all zero), records at and behind it are not touched.  status_out may be status_in.
 * The reference's CQ spot list with AP: ft8gpu_decode_candidates -> ft8gpu_ap_candidates -> ft8gpu_collect_spots. */
int ft8gpu_ap_candidates(ft8gpu_ctx *ctx, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                         const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_ap_hypothesis *hyps, int nhyp,
                         int max_hard_errors, ft8gpu_decode_status *status_out, ft8gpu_ap_info *info, int flags);
/* A hypothesis from a standard type 1 message with `?` for the unknown tokens: "CQ ? ?", "CQ DX ? ?", "CQ POTA ? ?",
 * "K1ABC ? ?", "K1ABC W9XYZ ?", "? W9XYZ FN42", ...  FIELD1 CALL2 THIRD as ft8gpu_pack77 takes them for i3 = 1 ("CQ nnn" /
 * "CQ aaaa" count as FIELD1; THIRD is one token).  A known FIELD1 masks bits 0..28, a known CALL2 bits 29..57, a known THIRD
 * bits 58..73; bits 74..76 (i3 = 1) are always masked.  "CQ ? ?" gives exactly the 32 bits 0..28 and 74..76.
 * A pattern without `?` masks all 77 bits.  0 = ok, -1 = not such a pattern (a token the packer refuses, a /P call, more
 * or fewer than three fields).  Host C. */
int ft8gpu_ap_from_text(const char *pattern, ft8gpu_ap_hypothesis *out);
/* The whole path with AP and OSD behind every pass: each pass runs as in ft8gpu_decode_messages_deep; then AP runs in place
 * on the pass's status records and the append step adds the unique messages it gained, in candidate order (pad[1] of such a
 * record = 1 + the accepted hypothesis); then OSD runs in place on what AP left undecoded (pad[0] as in the deep entry).
 * n_by_stage [nframes][passes][3] (NULL: not written): the count after BP, after AP and after OSD of each pass.
 * nhyp = 0: no AP -- the launches and the message bytes of ft8gpu_decode_messages_deep.  osd_order -1: no OSD. */
typedef struct {
    int32_t passes;                 /* 1 .. FT8GPU_MAX_PASSES */
    int32_t nhyp;                   /* 0 (no AP) .. FT8GPU_AP_MAX_HYPOTHESES */
    int32_t ap_max_hard_errors;     /* 0 .. 174; FT8GPU_AP_MAX_HARD_ERRORS is the recommended value */
    int32_t osd_order;              /* -1 (no OSD), 0, 1, 2 */
    int32_t osd_max_hard_errors;    /* 0 .. 83 */
    ft8gpu_ap_hypothesis hyps[FT8GPU_AP_MAX_HYPOTHESES];
} ft8gpu_ap_params;
int ft8gpu_decode_messages_ap(ft8gpu_ctx *ctx, const float *iq, int nframes, const ft8gpu_ap_params *params,
                              ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags);
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_ap_hypothesis) == 20 && offsetof(ft8gpu_ap_hypothesis, bits) == 10, "ft8gpu_ap_hypothesis layout");
_Static_assert(sizeof(ft8gpu_ap_info) == 8 && offsetof(ft8gpu_ap_info, nhard) == 1 && offsetof(ft8gpu_ap_info, hyp) == 2 &&
               offsetof(ft8gpu_ap_info, iters) == 3 && offsetof(ft8gpu_ap_info, results) == 4, "ft8gpu_ap_info layout");
_Static_assert(sizeof(ft8gpu_ap_params) == 100 && offsetof(ft8gpu_ap_params, osd_order) == 12 && offsetof(ft8gpu_ap_params, hyps) == 20,
               "ft8gpu_ap_params layout");
#else
static_assert(sizeof(ft8gpu_ap_hypothesis) == 20 && offsetof(ft8gpu_ap_hypothesis, bits) == 10, "ft8gpu_ap_hypothesis layout");
static_assert(sizeof(ft8gpu_ap_info) == 8 && offsetof(ft8gpu_ap_info, nhard) == 1 && offsetof(ft8gpu_ap_info, hyp) == 2 &&
              offsetof(ft8gpu_ap_info, iters) == 3 && offsetof(ft8gpu_ap_info, results) == 4, "ft8gpu_ap_info layout");
static_assert(sizeof(ft8gpu_ap_params) == 100 && offsetof(ft8gpu_ap_params, osd_order) == 12 && offsetof(ft8gpu_ap_params, hyps) == 20,
              "ft8gpu_ap_params layout");
#endif
/* one line per message, "%3d %4.1f %4d ~  %s\n" of snr_db, dt_s, (int)freq_hz, text (NUL-terminated, truncated to cap);
 * returns the untruncated length.  Host-side text formatting, no GPU involved. */
int ft8gpu_format_messages(const ft8gpu_message *msgs, int32_t n, char *out, size_t cap);

/* ---- hashed call signs: a call hash table per receiver, carried from one 15 s slot into the next ---------------------------
 * (DESIGN.md "Call hash table"; not in the reference, whose ft8_lib era prints "<...>" for every hashed call.)  A type 1 / 2
 * message may carry a call as a 22-bit hash, and a type 4 message carries one of its two calls as a 12-bit hash; a receiver
 * names the sender from the calls it has heard in clear.  ft8gpu_message.text keeps "<...>"; the resolved text is a second
 * record array beside the messages.  The rule is exact, integers and bytes only:
 *
 * Hash.  The call, left-justified in 11 characters and padded with blanks, read as a base-38 number over " 0-9A-Z/" (blank
 * = 0 .. '/' = 37), times 47055833459 modulo 2^64; the m-bit hash is the top m bits.  h22 is the 22-bit hash, and the 12-bit
 * hash is h22 >> 10.
 *
 * State.  One ft8gpu_callhash_state per receiver, caller-owned, read at entry and written at exit, in host or device memory
 * like the arrays of the call.  entry[i] holds the last call written with h22 >> 10 == i: `call` left-justified with blanks
 * at `len` and behind it, len = 0 for an empty entry (a len above 11 reads as 11), h22 its 22-bit hash.  stamp[i] is the value
 * of `slot` when entry[i] was written, slot the number of slots consumed so far, pad is zero.  ft8gpu_callhash_reset zeroes
 * all of it.
 *
 * Per slot (one frame of the receiver), with the frame's records [0, n), n = n_msgs[f] clamped to [0, 50], and the fields
 * taken from a91 as unpack77 takes them (i3 = bits 74..76; type 1 / 2: n28a = bits 0..27, n28b = bits 29..56; type 4:
 * n12 = bits 0..11, n58 = bits 12..69, iflip = bit 70, icq = bit 73).  NTOKENS = 2063592, MAX22 = 4194304.
 *   Insert phase.  The records in order, within a record the first call field before the second; every call that travels in
 *   clear is written to entry[h22 >> 10] with stamp = slot, over whatever is there: the last writer in (record, field) order
 *   wins.  A call in clear is
 *     - i3 = 1 or 2, a field with n28 >= NTOKENS + MAX22: the standard call as unpack77 prints it, without /R or /P (and
 *       without the 3DA0 / 3X rewriting of later ft8_lib versions, which this unpacker does not do);
 *     - i3 = 4: the 11 characters of n58 without leading and trailing blanks, also when icq is set; nothing if none is left.
 *   Special tokens, hashed fields (resolved or not), free text, telemetry and every other i3 insert nothing.
 *   Resolve phase, against the table as it stands after the slot's own inserts (a message resolves against a call heard in
 *   the same slot, whichever record came first).
 *     - i3 = 1 or 2, a field with NTOKENS <= n28 < NTOKENS + MAX22: h = n28 - NTOKENS is looked up at entry[h >> 10]; it
 *       resolves iff len != 0, the entry is not expired, and the stored h22 == h;
 *     - i3 = 4 with icq = 0: entry[n12]; it resolves iff len != 0 and the entry is not expired.
 *     An entry is expired when max_age != 0 and (uint32_t)(slot - stamp) > max_age (unsigned: the counter may wrap);
 *     max_age = 0 never expires.
 *   Then slot increments, also for a slot without records.
 *
 * Output.  One ft8gpu_resolved per record, parallel to msgs [nframes][50]; records at index n and above are not touched.
 *   n_hashed       hashed fields of the record by a91 (0 .. 2);  n_inserted  calls it inserted (0 .. 2, the overwritten too)
 *   resolved_mask  bit k set iff the k-th hashed field resolved, k counted in text order: for i3 = 1 / 2 the first field
 *                  before the second, for i3 = 4 the only one;  n_resolved = the number of set bits
 *   text           msgs.text (its first 25 bytes up to a NUL) with the k-th "<...>" replaced by '<' call[0 .. len) '>' where
 *                  bit k is set, cut at 39 characters and zero-filled behind the string.  '<' is not in the free-text
 *                  alphabet and no other field prints one, so "<...>" in a message text comes only from a hashed field, and
 *                  the k-th one is the k-th hashed field.  The longest text is two 11-character calls and "R FN20": 34. */
typedef struct {
    char     call[11];       /*  0  left-justified, blanks at len and behind it */
    uint8_t  len;            /* 11  0 = empty */
    uint32_t h22;            /* 12  the 22-bit hash of call */
} ft8gpu_callhash_entry;
#define FT8GPU_CALLHASH_ENTRIES 4096
typedef struct {
    ft8gpu_callhash_entry entry[FT8GPU_CALLHASH_ENTRIES];   /*     0  direct-mapped by the 12-bit hash = h22 >> 10 */
    uint32_t stamp[FT8GPU_CALLHASH_ENTRIES];                 /* 65536  the value of `slot` when the entry was written */
    uint32_t slot;                                           /* 81920  slots consumed so far */
    uint32_t pad[3];                                         /* 81924  zero */
} ft8gpu_callhash_state;
typedef struct {
    char    text[40];        /*  0 */
    uint8_t n_hashed;        /* 40 */
    uint8_t n_resolved;      /* 41 */
    uint8_t n_inserted;      /* 42 */
    uint8_t resolved_mask;   /* 43 */
    uint8_t pad[4];          /* 44  zero */
} ft8gpu_resolved;
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_callhash_entry) == 16 && offsetof(ft8gpu_callhash_entry, len) == 11 &&
               offsetof(ft8gpu_callhash_entry, h22) == 12, "ft8gpu_callhash_entry layout");
_Static_assert(sizeof(ft8gpu_callhash_state) == 81936 && offsetof(ft8gpu_callhash_state, stamp) == 65536 &&
               offsetof(ft8gpu_callhash_state, slot) == 81920 && offsetof(ft8gpu_callhash_state, pad) == 81924,
               "ft8gpu_callhash_state layout");
_Static_assert(sizeof(ft8gpu_resolved) == 48 && offsetof(ft8gpu_resolved, n_hashed) == 40 && offsetof(ft8gpu_resolved, n_resolved) == 41 &&
               offsetof(ft8gpu_resolved, n_inserted) == 42 && offsetof(ft8gpu_resolved, resolved_mask) == 43 &&
               offsetof(ft8gpu_resolved, pad) == 44, "ft8gpu_resolved layout");
#else
static_assert(sizeof(ft8gpu_callhash_entry) == 16 && offsetof(ft8gpu_callhash_entry, len) == 11 &&
              offsetof(ft8gpu_callhash_entry, h22) == 12, "ft8gpu_callhash_entry layout");
static_assert(sizeof(ft8gpu_callhash_state) == 81936 && offsetof(ft8gpu_callhash_state, stamp) == 65536 &&
              offsetof(ft8gpu_callhash_state, slot) == 81920 && offsetof(ft8gpu_callhash_state, pad) == 81924,
              "ft8gpu_callhash_state layout");
static_assert(sizeof(ft8gpu_resolved) == 48 && offsetof(ft8gpu_resolved, n_hashed) == 40 && offsetof(ft8gpu_resolved, n_resolved) == 41 &&
              offsetof(ft8gpu_resolved, n_inserted) == 42 && offsetof(ft8gpu_resolved, resolved_mask) == 43 &&
              offsetof(ft8gpu_resolved, pad) == 44, "ft8gpu_resolved layout");
#endif
/* stage entry: msgs [nstreams][nslots][50], n_msgs [nstreams][nslots], resolved [nstreams][nslots][50]: nstreams independent
 * receivers, each with nslots consecutive slots; state [nstreams], one object per receiver (the states of a call must be
 * distinct objects: receivers run side by side), 16-byte aligned in the device form.  FT8GPU_HOST_PTRS / FT8GPU_DEVICE_PTRS
 * for every array, state included.  Any nstreams * nslots: the host form stages whole receivers, or runs of slots of one
 * receiver, at most max_frames frames at a time, and the result does not depend on the cut -- as nslots slots in one call
 * leave the bytes that nslots calls of one slot leave.  nslots <= 2^24. */
int ft8gpu_resolve_calls(ft8gpu_ctx *ctx, const ft8gpu_message *msgs, const int32_t *n_msgs, int nstreams, int nslots,
                         ft8gpu_callhash_state *state, uint32_t max_age, ft8gpu_resolved *resolved, int flags);
/* The whole path: ft8gpu_decode_messages (ap_params == NULL) or ft8gpu_decode_messages_ap (n_by_stage NULL) over the
 * nstreams * nslots frames iq [nstreams][nslots][2][48000], then ft8gpu_resolve_calls on its records.  msgs and n_msgs are
 * byte for byte what that entry writes.  With ft8gpu_rx_stream in front, a daemon carries two states per receiver from slot
 * to slot: the filter state and this one. */
int ft8gpu_decode_messages_resolved(ft8gpu_ctx *ctx, const float *iq, int nstreams, int nslots, const ft8gpu_ap_params *ap_params,
                                    ft8gpu_callhash_state *state, uint32_t max_age, ft8gpu_message *msgs, int32_t *n_msgs,
                                    ft8gpu_resolved *resolved, int flags);
/* Host helpers of the table (plain C, no GPU).  A call is 1 .. 11 characters of " 0-9A-Z/" without a leading or trailing
 * blank, NUL-terminated; anything else is refused with -1. */
void ft8gpu_callhash_reset(ft8gpu_callhash_state *state);
/* the bits-bit hash (1 .. 32) of call */
int  ft8gpu_call_hash(const char *call, int bits, uint32_t *out);
/* writes call into state as the insert phase does, with stamp = state->slot: e.g. the operator's own call before the first slot */
int  ft8gpu_callhash_insert(ft8gpu_callhash_state *state, const char *call);
/* the resolve phase's lookup of a hash of 12 or 22 bits at state->slot: 1 and the call in out (NUL-terminated), else 0 and
 * out[0] = 0; -1 for other bits or a hash that does not fit them */
int  ft8gpu_callhash_lookup(const ft8gpu_callhash_state *state, int bits, uint32_t hash, uint32_t max_age, char out[12]);
/* ft8gpu_format_messages with the resolved text: "%3d %4.1f %4d ~  %s\n" of msgs[i].snr_db, dt_s, (int)freq_hz and
 * resolved[i].text, for i < n (at most 50) */
int  ft8gpu_format_resolved(const ft8gpu_message *msgs, const ft8gpu_resolved *resolved, int32_t n, char *out, size_t cap);

/* ---- expected messages: undecoded candidates against what a receiver heard in earlier slots ------------------------------
 * (DESIGN.md "Expected messages"; not in the reference, which treats every 15 s slot as if nothing had been heard before it.)
 * FT8 traffic repeats: the same CQ two slots later, the RRR / RR73 / 73 that closes a QSO.  A receiver keeps a table of
 * expected payloads, and every candidate BP fails on is compared with the codewords of the table: a full 77-bit hypothesis
 * where AP uses a partial one.  The rule is exact, integers and float comparisons only.
 *
 * State.  One ft8gpu_expect_state per receiver, caller-owned, in host or device memory like the arrays of the call.
 * entry[i]: payload = 77 bits, MSB first, as ft8gpu_pack77 writes them (bits 77..79 are ignored wherever a payload is read
 * and zero wherever one is written); used != 0 = the entry is live; kind 0 = heard, 1 = derived; stamp = the value of `slot`
 * at the last write or refresh.  cursor (read modulo 512) is where the next new entry goes, slot the number of slots
 * consumed so far, pad is zero.  An entry is expired when max_age != 0 and (uint32_t)(slot - stamp) > max_age (unsigned:
 * the counter may wrap); max_age = 0 never expires.  Expiry is judged only when candidates are matched: an expired entry
 * stays in the table and can be refreshed.
 *
 * Matching (ft8gpu_match_candidates; the states are read only).
 *   A candidate qualifies as for OSD: its status record has ok == 0 and ldpc_errors != 0; one that does not gets
 *   status_out = status_in and an all-zero info record.
 *   llr[0..173], h[i] = llr[i] > 0 and w[i] = 255 if |llr[i]| >= 32 else (int)(|llr[i]| * 8) are exactly OSD's.  A non-finite
 *   llr[i]: result 6, nothing is compared.
 *   The live entries of the frame's state are those with used != 0 that are not expired at state.slot.  None: result 0, the
 *   info record is all zero and the status is copied.
 *   c_j = the codeword of live entry j's payload: the 77 bits, their CRC-14 as ft8_lib's encoder computes it, the 83 generator
 *   parities.  nhard_j = the number of positions where c_j differs from h, metric_j = the sum of w over those positions.
 *   The best entry has the smallest metric, ties go to the smallest table index; info.index is that index, info.nhard and
 *   info.metric its values, accepted or not.
 *   Only the best entry is judged; the first failing check names the result: 5 all-zero payload, 2 nhard > max_hard_errors,
 *   4 unpack77 < 0, else 1 = accepted.  (3 and 7 do not occur here; the numbering stays that of OSD and AP.)
 *   On acceptance the status record becomes that of a BP success, as OSD writes it (ok = 1, ldpc_errors = 0, both CRC fields
 *   the codeword's CRC, unpack_status, a91, text; iters as it was); otherwise it is unchanged.
 *
 * Update (ft8gpu_expect_update).  Each receiver takes its slots in order, within a slot the records [0, n) in order,
 * n = n_msgs[f] clamped to [0, 50].  The record's payload P (the first 77 bits of a91) goes through insert(P, 0).  With
 * derive != 0, a record of type 1 (i3 = bits 74..76 = 1) whose two call fields are standard calls in clear (n28 >= NTOKENS +
 * MAX22, the constants of the call hash rule) then inserts three derived payloads with kind 1: the two 29-bit call fields
 * swapped (bits 0..28 and 29..57 change places, each call keeps its /R or /P flag), ir (bit 58) = 0, i3 = 1, and igrid4
 * (bits 59..73) = 32402, 32403, 32404 in that order: RRR, RR73, 73.  CQ and the other special tokens, hashed fields, i3 = 2
 * and every other message type derive nothing.
 *   insert(P, kind): if an entry with used != 0 and the same 77 bits exists, expired or not (the smallest index if a
 *   caller-built state holds several), its stamp = slot and its kind &= kind -- a message once heard stays kind 0.  Otherwise
 *   entry[cursor % 512] = { P, used = 1, kind, stamp = slot } and cursor = cursor % 512 + 1.
 * After the slot's records slot increments, also for a slot without records. */
#define FT8GPU_EXPECT_ENTRIES 512
typedef struct {
    uint8_t  payload[10];    /*  0 */
    uint8_t  used;           /* 10 */
    uint8_t  kind;           /* 11 */
    uint32_t stamp;          /* 12 */
} ft8gpu_expect_entry;
typedef struct {
    ft8gpu_expect_entry entry[FT8GPU_EXPECT_ENTRIES];   /*    0 */
    uint32_t cursor;                                    /* 8192 */
    uint32_t slot;                                      /* 8196 */
    uint32_t pad[2];                                    /* 8200  zero */
} ft8gpu_expect_state;
typedef struct {
    uint8_t  result;         /* 0 not attempted or no live entry, 1 accepted, 2, 4, 5 the failing check, 6 non-finite soft bits */
    uint8_t  nhard;          /* the best entry's values, accepted or not */
    uint16_t index;
    int32_t  metric;
} ft8gpu_match_info;
typedef struct {
    int32_t  max_hard_errors;    /* 0 .. 174; FT8GPU_MATCH_MAX_HARD_ERRORS is the recommended value */
    uint32_t max_age;            /* slots; 0 = entries never expire */
    int32_t  derive;             /* != 0: the update rule derives RRR / RR73 / 73 */
} ft8gpu_expect_params;
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_expect_entry) == 16 && offsetof(ft8gpu_expect_entry, used) == 10 && offsetof(ft8gpu_expect_entry, kind) == 11 &&
               offsetof(ft8gpu_expect_entry, stamp) == 12, "ft8gpu_expect_entry layout");
_Static_assert(sizeof(ft8gpu_expect_state) == 8208 && offsetof(ft8gpu_expect_state, cursor) == 8192 &&
               offsetof(ft8gpu_expect_state, slot) == 8196 && offsetof(ft8gpu_expect_state, pad) == 8200, "ft8gpu_expect_state layout");
_Static_assert(sizeof(ft8gpu_match_info) == 8 && offsetof(ft8gpu_match_info, nhard) == 1 && offsetof(ft8gpu_match_info, index) == 2 &&
               offsetof(ft8gpu_match_info, metric) == 4, "ft8gpu_match_info layout");
_Static_assert(sizeof(ft8gpu_expect_params) == 12 && offsetof(ft8gpu_expect_params, max_age) == 4 &&
               offsetof(ft8gpu_expect_params, derive) == 8, "ft8gpu_expect_params layout");
#else
static_assert(sizeof(ft8gpu_expect_entry) == 16 && offsetof(ft8gpu_expect_entry, used) == 10 && offsetof(ft8gpu_expect_entry, kind) == 11 &&
              offsetof(ft8gpu_expect_entry, stamp) == 12, "ft8gpu_expect_entry layout");
static_assert(sizeof(ft8gpu_expect_state) == 8208 && offsetof(ft8gpu_expect_state, cursor) == 8192 &&
              offsetof(ft8gpu_expect_state, slot) == 8196 && offsetof(ft8gpu_expect_state, pad) == 8200, "ft8gpu_expect_state layout");
static_assert(sizeof(ft8gpu_match_info) == 8 && offsetof(ft8gpu_match_info, nhard) == 1 && offsetof(ft8gpu_match_info, index) == 2 &&
              offsetof(ft8gpu_match_info, metric) == 4, "ft8gpu_match_info layout");
static_assert(sizeof(ft8gpu_expect_params) == 12 && offsetof(ft8gpu_expect_params, max_age) == 4 &&
              offsetof(ft8gpu_expect_params, derive) == 8, "ft8gpu_expect_params layout");
#endif
/* Recommended max_hard_errors, from profiles/match_gain.json (tools/match_gain.py, a sweep over 30 .. 60): the largest gate
 * that accepts nothing wrong on the 96 CQ frames of 20 and of 30 signals at -22 .. 0 dB (7119 / 8078 failing candidates, the
 * planted messages and 236 unrelated CQ messages in the table) and on 96 noise frames (942 candidates, 256 unrelated CQ
 * messages).  The wrong best entries begin at 50 hard errors on both CQ rows and at 54 on noise; at 49 matching gains 334 /
 * 494 planted messages over BP's 1046 / 1295 (+32 % / +38 %; AP gains 42 and OSD order 2 gains 30 on the first row).  Nothing
 * but the gate keeps a wrong entry out: every table entry is a codeword with a good CRC.  The hazard is a message on the air
 * whose near relative is in the table while it is not itself: on 48 two-call frames whose table holds RRR / RR73 / 73 / -10
 * of every planted pair but never the message, 7 of 3867 candidates accept a sibling at 49 (0.15 per frame; 1 at 45, 13 at
 * 50).  A caller that lists closings without hearing them (derive, or its own list) and cannot afford those uses 40: no
 * sibling is accepted up to 42, and the gain on the first row is still 236. */
#define FT8GPU_MATCH_MAX_HARD_ERRORS 49
/* stage entry: mag [nframes][94208], cands / status_in / status_out / info [nframes][max_candidates], counts [nframes],
 * states [nframes] (the state of the receiver each frame belongs to; 16-byte aligned in the device form); host or device
 * pointers by `flags`.  max_hard_errors in [0, 174].  Records below counts[f] are written, records at and behind it are
 * not touched.  status_out may be status_in. */
int ft8gpu_match_candidates(ft8gpu_ctx *ctx, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                            const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_expect_state *states,
                            uint32_t max_age, int max_hard_errors, ft8gpu_decode_status *status_out, ft8gpu_match_info *info,
                            int flags);
/* stage entry of the update rule: msgs [nstreams][nslots][50], n_msgs [nstreams][nslots], state [nstreams], one object per
 * receiver, read at entry and written at exit; host or device pointers by `flags` (device form: msgs and state 16-byte
 * aligned).  The host form stages whole receivers, or runs of slots of one receiver, at most max_frames frames at a time;
 * the result does not depend on the cut. */
int ft8gpu_expect_update(ft8gpu_ctx *ctx, const ft8gpu_message *msgs, const int32_t *n_msgs, int nstreams, int nslots,
                         ft8gpu_expect_state *state, int derive, int flags);
/* The whole path over iq [nstreams][nslots][2][48000], for the frame of receiver r at slot t:
 *   1. the records [0, n1) are byte for byte those of ft8gpu_decode_messages;
 *   2. ft8gpu_match_candidates runs in place on that frame's BP status records, against the receiver's state as the slots
 *      0 .. t - 1 left it;
 *   3. the append step of the multi-pass path (ft8gpu_append_messages' rule) adds, in candidate order, every unique gained
 *      message not yet among the frame's records, up to 50 in all; pad[2] of such a record is 1;
 *   4. the update rule runs over the frame's final records.
 * n_by_stage [nstreams][nslots][2] (NULL: not written): the count after BP and after matching.  nslots slots in one call
 * leave the bytes that nslots calls of one slot leave, in msgs, n_msgs and the state.  Not composed with AP, OSD or
 * multi-pass. */
int ft8gpu_decode_messages_expected(ft8gpu_ctx *ctx, const float *iq, int nstreams, int nslots, ft8gpu_expect_state *state,
                                    const ft8gpu_expect_params *params, ft8gpu_message *msgs, int32_t *n_msgs,
                                    int32_t *n_by_stage, int flags);
/* Host helpers of the table (plain C, no GPU): a caller builds any list for the stage entry with them, e.g. the replies it
 * expects to its own call. */
void ft8gpu_expect_reset(ft8gpu_expect_state *state);
/* insert(payload, kind) of the update rule at state->slot; kind 0 or 1, else -1 */
int  ft8gpu_expect_insert(ft8gpu_expect_state *state, const uint8_t payload[10], int kind);
/* the same with the payload ft8gpu_pack77 gives for text, as kind 0; -1 if the packer refuses the text */
int  ft8gpu_expect_insert_text(ft8gpu_expect_state *state, const char *text);

/* ---- call hints: a-priori decoding from the calls a receiver heard in earlier slots ----------------------------------------
 * (DESIGN.md "Call hints"; not in the reference.)  Between AP's fixed guesses for the whole batch and a whole expected message
 * lies most QSO traffic: a station heard in slot t sends again in t + 2 with the same call in the second field and new content,
 * and its partner answers in t + 1 with both calls swapped and a third field nobody can predict.  A receiver keeps a table of
 * call fields, and a candidate BP fails on is decoded again by the per-hypothesis rule of ft8gpu_ap_candidates under the
 * few table entries its hard decisions agree with best.  The rule is exact; the preselection is integers only.
 *
 * State.  One ft8gpu_hint_state per receiver, caller-owned, in host or device memory like the arrays of the call (16-byte
 * aligned in the device form).  entry[i]: a = field 1, payload bits 0..28 as a number, MSB first (n28 << 1 | flag), read
 * & 0x1FFFFFFF; b = field 2, payload bits 29..57, likewise; stamp = the value of `slot` at the last write or refresh;
 * kind 1 = "A ? ?", 2 = "? B ?", 3 = "A B ?"; phase (read & 1) = the slot parity at which the message is expected.  cursor
 * (read modulo 512) is where the next new entry goes, slot the number of slots consumed so far, pad is zero.
 * An entry is live when used != 0, kind is 1, 2 or 3, it is not expired -- max_age != 0 and (uint32_t)(slot - stamp) >
 * max_age (unsigned: the counter may wrap) -- and, with use_phase != 0, ((slot ^ phase) & 1) == 0.  Expiry and phase are
 * judged only when candidates are tried: an expired entry stays in the table and can be refreshed.
 * The hypothesis of an entry (ft8gpu_hint_hypothesis): bits 74..76 are always masked, value 001 (i3 = 1); kind & 1 masks bits
 * 0..28 with a, kind & 2 masks bits 29..57 with b.  nmask is 32 or 61.
 *
 * Trying candidates (ft8gpu_hint_candidates; the states are read only).
 *   A candidate qualifies as for AP: its status record has ok == 0 and ldpc_errors != 0; one that does not gets status_out =
 *   status_in and an all-zero info record.  llr, h and apmag are AP's; a non-finite llr[i] or apmag == 0: result 6, nothing
 *   is tried.
 *   Preselection.  For each live entry j, nbad_j = the number of masked positions where h differs from the hypothesis.  The
 *   entry passes when nbad_j * 64 <= max_bad_per_64 * nmask_j.  Passing entries are ordered by nbad_j / nmask_j, compared by
 *   cross-multiplication (key = nbad_j * 61 for nmask 32, nbad_j * 32 for nmask 61); ties go to the larger nmask, then to the
 *   smaller index.  No passing entry: result 0, the info record is all zero and the status is copied.
 *   The first `tries` passing entries are tried in that order, each by exactly the per-hypothesis rule of
 *   ft8gpu_ap_candidates (the codes 7, 8, 5, 2, 3, 4, 1; the hard errors counted on the unmasked positions; the record
 *   written on acceptance; 5 cannot occur: bit 76 of every hypothesis is 1, so a word that agrees with it is not all-zero, and
 *   bp_decode leaves at an all-zero word as "no codeword", 7).  The first accepted entry wins.  For any candidate, the stage's status bytes equal those of
 *   ft8gpu_ap_candidates called with these hypotheses in this order.
 *
 * Update (ft8gpu_hint_update).  Each receiver takes its slots in order, within a slot the records [0, n) in order, n =
 * n_msgs[f] clamped to [0, 50].  Only records of type 1 (bits 74..76 = 1) count.  A field is a clear call when its n28 >=
 * NTOKENS + MAX22 (the constants of the call hash rule): CQ and the other tokens, and hashed calls, are not.  With F1 = bits
 * 0..28, F2 = bits 29..57 and p = slot & 1, in this order:
 *   F2 clear:          insert(2, 0, F2, p)        the sender sends again
 *   F2 clear:          insert(1, F2, 0, p ^ 1)    somebody calls the sender
 *   F1 and F2 clear:   insert(3, F1, F2, p)       same direction, next step
 *   F1 and F2 clear:   insert(3, F2, F1, p ^ 1)   the reply
 *   insert(kind, a, b, phase): if an entry with used != 0 and the same (kind, a & 0x1FFFFFFF, b & 0x1FFFFFFF, phase & 1)
 *   exists, expired or not (the smallest index if a caller-built state holds several), its stamp = slot.  Otherwise
 *   entry[cursor % 512] = { a, b, stamp = slot, kind, used = 1, phase, pad = 0 } and cursor = cursor % 512 + 1.
 * After the slot's records slot increments (unsigned, it wraps), also for a slot without records. */
#define FT8GPU_HINT_ENTRIES 512
typedef struct {
    uint32_t a;              /*  0 */
    uint32_t b;              /*  4 */
    uint32_t stamp;          /*  8 */
    uint8_t  kind;           /* 12 */
    uint8_t  used;           /* 13 */
    uint8_t  phase;          /* 14 */
    uint8_t  pad;            /* 15 */
} ft8gpu_hint_entry;
typedef struct {
    ft8gpu_hint_entry entry[FT8GPU_HINT_ENTRIES];       /*    0 */
    uint32_t cursor;                                    /* 8192 */
    uint32_t slot;                                      /* 8196 */
    uint32_t pad[2];                                    /* 8200  zero */
} ft8gpu_hint_state;
typedef struct {
    uint8_t  result;         /* 0 not attempted or no passing entry, 1 accepted, 2..5, 7, 8 the failing check, 6 unusable soft bits */
    uint8_t  nhard;          /* result, nhard, iters: of the last entry tried */
    uint8_t  ntried;         /* the number of entries tried, 0 .. tries */
    uint8_t  iters;
    uint8_t  results[FT8GPU_AP_MAX_HYPOTHESES];     /* the code of every entry tried, 0 for the others */
    uint16_t index[FT8GPU_AP_MAX_HYPOTHESES];       /* the table indices tried, in order; 0 beyond ntried */
} ft8gpu_hint_info;
/* Recommended preselection gate, tries and max_hard_errors, from profiles/hint_gain.json (tools/hint_gain.py on one MI355X: a
 * sweep over gates 8 .. 24, tries 1 / 2 / 4 and hard-error gates 30 / 40 / 50 / 174 on 96 receivers x 4 slots of QSOs that
 * advance one step per slot at 20 and at 30 signals per frame, -24 .. 0 dB, the tables filled by the update rule alone and
 * pre-filled with 236 entries from unrelated calls, and on 384 noise frames against full tables of unrelated entries).  No
 * parameter set of the sweep accepts a message that was not sent, on any row, so the values are those of the largest gain:
 * +246 / +367 planted messages over BP's 3848 / 4754 (+6.4 % / +7.7 %; 239 / 354 with the unrelated entries), where "CQ ? ?"
 * a-priori decoding gains 13 / 26 and matching with derive 117 / 161 (and accepts 34 / 49 siblings of what was sent).  They
 * cost 2.8 .. 3.9 BP runs per failing candidate; gate 16 with 2 tries keeps 85 % of the gain (208 / 313) for 0.54 .. 0.83.
 * 24 is the sweep's upper edge: a wider gate has not been measured.  What "nothing wrong" bounds: at 24 / 4 the noise row ran
 * 15 584 BP tries on 3977 failing candidates and the QSO rows about 90 000 without a wrong acceptance, so the rate is below
 * about 3e-5 per try (95 %), not zero.  A hard-error gate below 40 loses messages, above it
 * gains none. */
#define FT8GPU_HINT_MAX_BAD_PER_64 24
#define FT8GPU_HINT_TRIES 4
#define FT8GPU_HINT_MAX_HARD_ERRORS 40
typedef struct {
    int32_t  tries;              /* 1 .. FT8GPU_AP_MAX_HYPOTHESES */
    int32_t  max_bad_per_64;     /* 0 .. 64: the preselection gate */
    int32_t  max_hard_errors;    /* 0 .. 174 */
    uint32_t max_age;            /* slots; 0 = entries never expire */
    int32_t  use_phase;          /* != 0: only entries of the slot's parity are live */
} ft8gpu_hint_params;
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_hint_entry) == 16 && offsetof(ft8gpu_hint_entry, b) == 4 && offsetof(ft8gpu_hint_entry, stamp) == 8 &&
               offsetof(ft8gpu_hint_entry, kind) == 12 && offsetof(ft8gpu_hint_entry, used) == 13 &&
               offsetof(ft8gpu_hint_entry, phase) == 14, "ft8gpu_hint_entry layout");
_Static_assert(sizeof(ft8gpu_hint_state) == 8208 && offsetof(ft8gpu_hint_state, cursor) == 8192 &&
               offsetof(ft8gpu_hint_state, slot) == 8196 && offsetof(ft8gpu_hint_state, pad) == 8200, "ft8gpu_hint_state layout");
_Static_assert(sizeof(ft8gpu_hint_info) == 16 && offsetof(ft8gpu_hint_info, nhard) == 1 && offsetof(ft8gpu_hint_info, ntried) == 2 &&
               offsetof(ft8gpu_hint_info, iters) == 3 && offsetof(ft8gpu_hint_info, results) == 4 &&
               offsetof(ft8gpu_hint_info, index) == 8, "ft8gpu_hint_info layout");
_Static_assert(sizeof(ft8gpu_hint_params) == 20 && offsetof(ft8gpu_hint_params, max_bad_per_64) == 4 &&
               offsetof(ft8gpu_hint_params, max_hard_errors) == 8 && offsetof(ft8gpu_hint_params, max_age) == 12 &&
               offsetof(ft8gpu_hint_params, use_phase) == 16, "ft8gpu_hint_params layout");
#else
static_assert(sizeof(ft8gpu_hint_entry) == 16 && offsetof(ft8gpu_hint_entry, b) == 4 && offsetof(ft8gpu_hint_entry, stamp) == 8 &&
              offsetof(ft8gpu_hint_entry, kind) == 12 && offsetof(ft8gpu_hint_entry, used) == 13 &&
              offsetof(ft8gpu_hint_entry, phase) == 14, "ft8gpu_hint_entry layout");
static_assert(sizeof(ft8gpu_hint_state) == 8208 && offsetof(ft8gpu_hint_state, cursor) == 8192 &&
              offsetof(ft8gpu_hint_state, slot) == 8196 && offsetof(ft8gpu_hint_state, pad) == 8200, "ft8gpu_hint_state layout");
static_assert(sizeof(ft8gpu_hint_info) == 16 && offsetof(ft8gpu_hint_info, nhard) == 1 && offsetof(ft8gpu_hint_info, ntried) == 2 &&
              offsetof(ft8gpu_hint_info, iters) == 3 && offsetof(ft8gpu_hint_info, results) == 4 &&
              offsetof(ft8gpu_hint_info, index) == 8, "ft8gpu_hint_info layout");
static_assert(sizeof(ft8gpu_hint_params) == 20 && offsetof(ft8gpu_hint_params, max_bad_per_64) == 4 &&
              offsetof(ft8gpu_hint_params, max_hard_errors) == 8 && offsetof(ft8gpu_hint_params, max_age) == 12 &&
              offsetof(ft8gpu_hint_params, use_phase) == 16, "ft8gpu_hint_params layout");
#endif
/* stage entry: mag [nframes][94208], cands / status_in / status_out / info [nframes][max_candidates], counts [nframes],
 * states [nframes] (the state of the receiver each frame belongs to; 16-byte aligned in the device form); host or device
 * pointers by `flags`, params in host memory.  Records below counts[f] are written, records at and behind it are not
 * touched.  status_out may be status_in. */
int ft8gpu_hint_candidates(ft8gpu_ctx *ctx, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                           const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_hint_state *states,
                           const ft8gpu_hint_params *params, ft8gpu_decode_status *status_out, ft8gpu_hint_info *info,
                           int flags);
/* stage entry of the update rule: msgs [nstreams][nslots][50], n_msgs [nstreams][nslots], state [nstreams], one object per
 * receiver, read at entry and written at exit; host or device pointers by `flags` (device form: msgs and state 16-byte
 * aligned).  The host form stages whole receivers, or runs of slots of one receiver, at most max_frames frames at a time;
 * the result does not depend on the cut. */
int ft8gpu_hint_update(ft8gpu_ctx *ctx, const ft8gpu_message *msgs, const int32_t *n_msgs, int nstreams, int nslots,
                       ft8gpu_hint_state *state, int flags);
/* The whole path over iq [nstreams][nslots][2][48000], for the frame of receiver r at slot t:
 *   1. the records [0, n1) are byte for byte those of ft8gpu_decode_messages;
 *   2. ft8gpu_hint_candidates runs in place on that frame's BP status records, against the receiver's state as the slots
 *      0 .. t - 1 left it;
 *   3. the append step of the multi-pass path adds, in candidate order, every unique gained message not yet among the
 *      frame's records, up to 50 in all; pad[2] of such a record is 3 (1 is match, 2 is combine);
 *   4. the update rule runs over the frame's final records.
 * n_by_stage [nstreams][nslots][2] (NULL: not written): the count after BP and after the hint stage.  nslots slots in one
 * call leave the bytes that nslots calls of one slot leave, in msgs, n_msgs and the state.  Not composed with AP, OSD,
 * match or multi-pass. */
int ft8gpu_decode_messages_hinted(ft8gpu_ctx *ctx, const float *iq, int nstreams, int nslots, ft8gpu_hint_state *state,
                                  const ft8gpu_hint_params *params, ft8gpu_message *msgs, int32_t *n_msgs,
                                  int32_t *n_by_stage, int flags);
/* Host helpers of the table (plain C, no GPU). */
void ft8gpu_hint_reset(ft8gpu_hint_state *state);
/* insert(kind, a, b, phase) of the update rule at state->slot; a and b are stored & 0x1FFFFFFF, phase & 1; kind 1, 2 or 3,
 * else -1 */
int  ft8gpu_hint_insert(ft8gpu_hint_state *state, int kind, uint32_t a, uint32_t b, int phase);
/* the same from a pattern of ft8gpu_ap_from_text with FIELD1 or CALL2 (or both) known and THIRD `?`: "K1ABC ? ?" lists a
 * caller's own call, "? W9XYZ ?", "K1ABC W9XYZ ?".  The field that is `?` is stored as 0.  -1: not such a pattern */
int  ft8gpu_hint_insert_text(ft8gpu_hint_state *state, const char *pattern, int phase);
/* the hypothesis of an entry as ft8gpu_ap_candidates takes it; -1 (and *out all zero) if kind is not 1, 2 or 3 */
int  ft8gpu_hint_hypothesis(const ft8gpu_hint_entry *entry, ft8gpu_ap_hypothesis *out);

/* ---- soft-bit memory: the soft bits of undecoded candidates summed over a receiver's slots ---------------------------------
 * (DESIGN.md "Soft-bit memory"; not in the reference, where every 15 s slot starts from nothing.)  A station that repeats its
 * message at the same audio frequency and clock offset, every time just below BP's threshold, is never decoded at all: the
 * call hash table, the expected messages and AP need a decode or a guess.  A receiver therefore keeps the normalised soft bits
 * of the candidates BP failed on, and a failing candidate of a later slot at the same position is decoded once more from the
 * renormalised sum.  Nothing about the message is assumed.  The rule is exact: float32 operations in a stated order.
 *
 * State.  One ft8gpu_softmem_state per receiver, caller-owned, host or device memory like the arrays of the call.  entry[i]:
 * cand = the candidate the entry was last stored from, used != 0 = live, count = the number of slots summed into llr
 * (saturating at 255), stamp = the value of `slot` when written, llr[0..173] = the running sum of the per-slot normalised soft
 * bits ([174], [175] zero).  cursor (read modulo 128) is where the next entry goes, slot the number of slots consumed, pad is
 * zero.  An entry is expired when max_age != 0 and (uint32_t)(slot - stamp) > max_age; max_age = 0 never expires.
 *
 * Combining (ft8gpu_combine_candidates; the states are read only).
 *   A candidate qualifies as for OSD, AP and matching: ok == 0 and ldpc_errors != 0.  One that does not gets status_out =
 *   status_in and an all-zero info record.
 *   own[0..173] = the soft bits the LDPC kernel starts from (ft8_extract_likelihood, ftx_normalize_logl).  A non-finite
 *   own[i]: result 6, the rest of the info record zero.
 *   Positions: T = 2 * time_offset + time_sub, F = 2 * freq_offset + freq_sub of the candidate; Te, Fe of an entry's cand.
 *   Live entries: used != 0 and not expired at state.slot.  A live entry is a partner when |T - Te| <= 1 and |F - Fe| <= 1.
 *   No partner: result 0, the info record all zero.
 *   nagree = the number of i < 174 with (own[i] > 0) == (entry.llr[i] > 0)  (a NaN is not > 0).  The best partner has the
 *   largest nagree; ties go to the smaller |T - Te| + |F - Fe|, then to the smaller index.  info.index, info.nagree and
 *   info.count (the entry's count) are the best partner's, accepted or not.  Only the best partner is tried.
 *   nagree < min_agree: result 8, BP does not run.
 *   s[i] = entry.llr[i] + own[i] (one float32 addition), x = ftx_normalize_logl(s): sum and sum of squares accumulated in
 *   index order in float32 (sum += s[i]; sum2 += s[i] * s[i], each operation rounded), variance = (sum2 - sum * sum * (1.0f /
 *   174)) * (1.0f / 174), x[i] = s[i] * sqrtf(24.0f / variance).  A non-finite x[i] (a sum of zero variance, a NaN or an
 *   infinity in the entry): result 6.
 *   bp_decode(x, ldpc_iters) runs, bit-exact to the LDPC kernel's iteration.  The first failing check names the result:
 *   7 no codeword within ldpc_iters, 5 all-zero, 3 CRC, 4 unpack77 < 0, else 1 = accepted.  (2 is not used: there is no
 *   hard-error gate.  bp_decode leaves at an all-zero word before it counts its parity errors, so 5 is kept for the
 *   numbering and cannot be reached.)  info.nhard = the number of positions where the codeword differs from x > 0, and 0
 *   without a codeword; diagnostic only.
 *   On acceptance the status record becomes that of a BP success, exactly as OSD, AP and matching write it (ok = 1,
 *   ldpc_errors = 0, both CRC fields, unpack_status, a91, text; iters as it was); otherwise it is unchanged.
 *
 * Update (ft8gpu_softmem_update; one slot: frame f belongs to states[f], read at entry and written at exit, pairwise
 * distinct).  In candidate order, the first store_per_slot candidates below counts[f] whose FINAL status record still has
 * ok == 0 and ldpc_errors != 0 and whose own is finite are stored.  A candidate on which BP ran (info.result 3, 4, 5 or 7)
 * stores llr[i] = entry[info.index].llr[i] + own[i] -- the s of combining -- with count = min(255, info.count + 1); every
 * other stored candidate stores own with count = 1.  The k-th stored candidate goes to entry[cursor % 128] with cand = the
 * candidate, used = 1, pad = 0, stamp = slot, llr[174] = llr[175] = 0, then cursor = cursor % 128 + 1.  Every sum is formed
 * from the state as it was at entry, also when the ring overwrites the partner in the same slot.  Afterwards slot
 * increments, also for a frame that stores nothing. */
#define FT8GPU_SOFTMEM_ENTRIES 128
typedef struct {
    ft8gpu_candidate cand;   /*  0  the candidate the entry was stored from (its last slot) */
    uint8_t  used;           /*  8 */
    uint8_t  count;          /*  9  slots summed into llr, saturating at 255 */
    uint16_t pad;            /* 10  zero */
    uint32_t stamp;          /* 12  value of `slot` when written */
    float    llr[176];       /* 16  running sum of the per-slot normalised soft bits; [174], [175] zero */
} ft8gpu_softmem_entry;
typedef struct {
    ft8gpu_softmem_entry entry[FT8GPU_SOFTMEM_ENTRIES];   /*     0 */
    uint32_t cursor;                                      /* 92160 */
    uint32_t slot;                                        /* 92164 */
    uint32_t pad[2];                                      /* 92168  zero */
} ft8gpu_softmem_state;
typedef struct {
    uint8_t result;          /* 0 not attempted or no partner, 1 accepted, 3, 4, 5, 7 the failing check, 6 non-finite soft bits, 8 nagree < min_agree */
    uint8_t nagree;          /* the best partner's values, accepted or not */
    uint8_t index;
    uint8_t count;
    uint8_t nhard;           /* codeword against x > 0; 0 without a codeword */
    uint8_t pad[3];          /* zero */
} ft8gpu_combine_info;
typedef struct {
    int32_t  min_agree;          /* 0 .. 174; FT8GPU_COMBINE_MIN_AGREE is the recommended value */
    uint32_t max_age;            /* slots; 0 = entries never expire */
    int32_t  store_per_slot;     /* 0 .. 128; FT8GPU_COMBINE_STORE_PER_SLOT is the recommended value.  Above 64 a partner two slots
                                  * back is overwritten before it is needed: the measured gain halves (see that constant) */
} ft8gpu_combine_params;
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_softmem_entry) == 720 && offsetof(ft8gpu_softmem_entry, used) == 8 && offsetof(ft8gpu_softmem_entry, count) == 9 &&
               offsetof(ft8gpu_softmem_entry, pad) == 10 && offsetof(ft8gpu_softmem_entry, stamp) == 12 &&
               offsetof(ft8gpu_softmem_entry, llr) == 16, "ft8gpu_softmem_entry layout");
_Static_assert(sizeof(ft8gpu_softmem_state) == 92176 && offsetof(ft8gpu_softmem_state, cursor) == 92160 &&
               offsetof(ft8gpu_softmem_state, slot) == 92164 && offsetof(ft8gpu_softmem_state, pad) == 92168, "ft8gpu_softmem_state layout");
_Static_assert(sizeof(ft8gpu_combine_info) == 8 && offsetof(ft8gpu_combine_info, nagree) == 1 && offsetof(ft8gpu_combine_info, index) == 2 &&
               offsetof(ft8gpu_combine_info, count) == 3 && offsetof(ft8gpu_combine_info, nhard) == 4, "ft8gpu_combine_info layout");
_Static_assert(sizeof(ft8gpu_combine_params) == 12 && offsetof(ft8gpu_combine_params, max_age) == 4 &&
               offsetof(ft8gpu_combine_params, store_per_slot) == 8, "ft8gpu_combine_params layout");
#else
static_assert(sizeof(ft8gpu_softmem_entry) == 720 && offsetof(ft8gpu_softmem_entry, used) == 8 && offsetof(ft8gpu_softmem_entry, count) == 9 &&
              offsetof(ft8gpu_softmem_entry, pad) == 10 && offsetof(ft8gpu_softmem_entry, stamp) == 12 &&
              offsetof(ft8gpu_softmem_entry, llr) == 16, "ft8gpu_softmem_entry layout");
static_assert(sizeof(ft8gpu_softmem_state) == 92176 && offsetof(ft8gpu_softmem_state, cursor) == 92160 &&
              offsetof(ft8gpu_softmem_state, slot) == 92164 && offsetof(ft8gpu_softmem_state, pad) == 92168, "ft8gpu_softmem_state layout");
static_assert(sizeof(ft8gpu_combine_info) == 8 && offsetof(ft8gpu_combine_info, nagree) == 1 && offsetof(ft8gpu_combine_info, index) == 2 &&
              offsetof(ft8gpu_combine_info, count) == 3 && offsetof(ft8gpu_combine_info, nhard) == 4, "ft8gpu_combine_info layout");
static_assert(sizeof(ft8gpu_combine_params) == 12 && offsetof(ft8gpu_combine_params, max_age) == 4 &&
              offsetof(ft8gpu_combine_params, store_per_slot) == 8, "ft8gpu_combine_params layout");
#endif
/* Recommended values, from profiles/combine_gain.json (tools/combine_gain.py: 96 receivers x 4 slots of 20 and of 30 CQ stations
 * per slot at -24 .. 0 dB, every station repeating two slots later at its own frequency and clock offset, and 96 receivers x 4
 * slots of noise; a sweep over min_agree 88 .. 130 in steps of 6 and store_per_slot 16 .. 128; BP alone decodes 4025 / 5022 of
 * the 7680 / 11520 planted messages).
 * min_agree: no point of the sweep accepts a message that was not on the air, on any row, so the recommended gate is the
 * smallest swept one, 88 -- one above the 87 of 174 positions two unrelated words agree in on average.  What keeps a wrong word
 * out is BP itself with the CRC and unpack77 behind it; the gate only spares BP runs (21.0 / 26.6 per frame at 88 and
 * store_per_slot 48, 19.5 / 24.7 at 118), and from 118 on it costs messages: 99 / 129 gained at 88 .. 106, 94 / 125 at 118,
 * 86 / 116 at 124, 59 / 97 at 130.  On noise hardly a candidate finds a partner (0.05 BP runs per frame at 88).
 * store_per_slot: the gain is not monotone.  At 88 the two CQ rows together gain 157, 198, 218, 228, 230 at 16, 24, 32, 48,
 * 64 and 116, 117 at 96, 128: the partner of a repeating station lies two slots back, and a ring of 128 entries that takes more
 * than 64 candidates per slot has overwritten it by then (candidates come in descending sync score, so the first ones stored
 * are the likeliest signals).  The smallest swept value within 2 % of the gain at 128 is therefore 16, which gives away a third
 * of what 64 gains; the constant is the smallest value within 2 % of the largest gain, 48 (228 of 230). */
#define FT8GPU_COMBINE_MIN_AGREE 88
#define FT8GPU_COMBINE_STORE_PER_SLOT 48
/* stage entry: mag [nframes][94208], cands / status_in / status_out / info [nframes][max_candidates], counts [nframes],
 * states [nframes] (the state of the receiver each frame belongs to; 16-byte aligned in the device form); host or device
 * pointers by `flags`.  min_agree in [0, 174]; ldpc_iters is the context's.  Records below counts[f] are written, records
 * at and behind it are not touched.  status_out may be status_in. */
int ft8gpu_combine_candidates(ft8gpu_ctx *ctx, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                              const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_softmem_state *states,
                              uint32_t max_age, int min_agree, ft8gpu_decode_status *status_out, ft8gpu_combine_info *info,
                              int flags);
/* stage entry of the update rule, one slot of nframes receivers: status = the final status records, info = the records
 * ft8gpu_combine_candidates wrote for the same frames and the same entry states (info.result, index and count are read;
 * an index is taken modulo 128), states [nframes] in-out (16-byte aligned in the device form).  store_per_slot in [0, 128]. */
int ft8gpu_softmem_update(ft8gpu_ctx *ctx, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                          const ft8gpu_decode_status *status, const ft8gpu_combine_info *info, int nframes,
                          ft8gpu_softmem_state *states, int store_per_slot, int flags);
/* The whole path over iq [nstreams][nslots][2][48000], for the frame of receiver r at slot t:
 *   1. the records [0, n1) are byte for byte those of ft8gpu_decode_messages;
 *   2. ft8gpu_combine_candidates runs in place on that frame's BP status records, against the receiver's state as the slots
 *      0 .. t - 1 left it;
 *   3. the append step of the multi-pass path adds, in candidate order, every unique gained message not yet among the
 *      frame's records, up to 50 in all; pad[2] of such a record is 2;
 *   4. ft8gpu_softmem_update runs on the frame's final status records.
 * n_by_stage [nstreams][nslots][2] (NULL: not written): the count after BP and after combining.  nslots slots in one call
 * leave the bytes that nslots calls of one slot leave, in msgs, n_msgs and the state.  Host or device pointers by `flags`
 * (device form: iq, msgs and state 16-byte aligned); the host form stages whole receivers, or runs of slots of one receiver,
 * at most max_frames frames at a time.  Not composed with AP, OSD, multi-pass or matching. */
int ft8gpu_decode_messages_combined(ft8gpu_ctx *ctx, const float *iq, int nstreams, int nslots, ft8gpu_softmem_state *state,
                                    const ft8gpu_combine_params *params, ft8gpu_message *msgs, int32_t *n_msgs,
                                    int32_t *n_by_stage, int flags);
/* all zero, as a receiver starts (plain C, no GPU) */
void ft8gpu_softmem_reset(ft8gpu_softmem_state *state);

/* ---- refined time and frequency: every message record located in the I/Q samples (DESIGN.md "Refined time and frequency") ----
 * freq_hz and dt_s of ft8gpu_message are the centre of the candidate's cell on the sync grid, 3.125 Hz by 256 samples.  The stage
 * below correlates the frame's samples with the message's own 79 tones on a grid of 32 samples, and at the best offset with
 * the tones 3.125 and 6.25 Hz to either side and with a tone the message leaves empty.  It writes powers only; the host helper
 * ft8gpu_refined_estimate turns them into seconds, hertz and decibels.  This text is the rule; tests/ft8_spec_refine.py
 * restates it in numpy, and the device output equals the restatement byte for byte.
 *
 * Inputs: the frame x[j] = (I[j], Q[j]), j < 48000, with x[j] = 0 for every other j; a record's cand and a91.
 *   T = 2 * time_offset + time_sub,  F = 2 * freq_offset + freq_sub
 *   tone[m], m < 79: the Costas tones {3,1,4,0,6,5,2} at m = 0..6, 36..42, 72..78; data symbol d = m - 7 (m < 36) or m - 14 is
 *     the Gray map {0,1,3,2,5,6,4,7} of codeword bits 3d .. 3d+2, MSB first; codeword bit i < 91 is bit i of a91 as stored
 *     (byte i / 8, MSB first), bit 91 + r the parity of a91 AND generator row r (ft8_encode's rule; for a decoded message
 *     the stored CRC is the encoder's)
 *   w[i] = (cos, -sin)(2 pi i / 1024), i < 1024, in float32: the waterfall's twiddle table
 *   k_m = F + 2 * tone[m]
 * Arithmetic, float32, one IEEE operation each, nothing fused:
 *   y(k, j) = x[j] * w[(k * j) mod 1024] = (xr * wr - xi * wi,  xr * wi + xi * wr)       (mod: the non-negative residue)
 *   g(k, q) = y(k, 32q) + ... + y(k, 32q + 31): both components summed in ascending j from +0
 *   s_m(e)  = 256 * T + FT8GPU_REFINE_LEAD + 512 * m + 32 * e                            (the first sample of symbol m)
 *   c(m, k, e) = g(k, q0) + ... + g(k, q0 + 15) in ascending q from +0,  q0 = s_m(e) / 32 (exact)
 *   P(u, e) = the sum over m = 0 .. 78, ascending from +0, of (re * re + im * im) of c(m, k_m + u, e)
 * The lead of 256 samples is the waterfall's geometry: row T multiplies the samples 256 T .. 256 T + 1023 by a window that
 * peaks at 256 T + 512, so it is centred on a symbol that starts at 256 T + 256.  (ft8o_synth_cpfsk and ft8gpu_synth_frames
 * confirm it: a signal started at sample S is found on the row T nearest (S - 256) / 256, and the refined offset then puts
 * s_0 on S.  dt_s of ft8gpu_message, 256 T / 3200, is therefore 0.08 s less than the start time t0_s of such a signal.)
 * Time search:  pt_all[e + 16] = P(0, e), e = -16 .. 16; e_best = the first e in ascending order whose power is strictly
 * greater than every earlier one (-16 when none is).  The range is +-512 samples because the record's candidate is the first
 * that carried the message, not the best one.
 * At e_best:  pf[u + 2] = P(u, e_best), u = -2 .. 2 (pf[2] is pt_all[e_best + 16]);  noise = the same sum with
 * k = F + 2 * ((tone[m] + 4) & 7) in place of k_m: the tone four away, which this message leaves empty in that symbol.
 * Samples: any float32 values give defined output, infinities and NaNs included.  Subnormal products, sums and powers are kept,
 * never flushed to zero, and a sum that overflows is the IEEE infinity.  The decisions (e_best, valid, the padding) are exact
 * for every input.  A comparison with a NaN is false, so a NaN power is never taken as a maximum over an earlier value, and no
 * later value is taken over a NaN in P(0, -16), where the scan starts (e_best is -16 then).  A float output that is a NaN by
 * this rule is a NaN in every implementation, with unspecified sign and payload (inf - inf has its sign bit set on x86 and
 * clear on gfx950); every other output is byte for byte. */
#define FT8GPU_REFINE_LEAD    256     /* samples from the first sample of waterfall row T to the symbol it is centred on */
#define FT8GPU_REFINE_STEP     32      /* samples per time-search step */
#define FT8GPU_REFINE_RANGE    16      /* the search covers e = -16 .. 16 */
typedef struct {
    int16_t e_best;          /*  0 */
    uint8_t valid;           /*  2  1 once written */
    uint8_t pad0;            /*  3  zero */
    float   pt[3];           /*  4  P(0, e_best - 1), P(0, e_best), P(0, e_best + 1); 0.0f where e lies outside [-16, 16] */
    float   pf[5];           /* 16 */
    float   noise;           /* 36 */
    uint8_t pad[8];          /* 40  zero */
} ft8gpu_refined;
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_refined) == 48 && offsetof(ft8gpu_refined, valid) == 2 && offsetof(ft8gpu_refined, pad0) == 3 &&
               offsetof(ft8gpu_refined, pt) == 4 && offsetof(ft8gpu_refined, pf) == 16 && offsetof(ft8gpu_refined, noise) == 36 &&
               offsetof(ft8gpu_refined, pad) == 40, "ft8gpu_refined layout");
#else
static_assert(sizeof(ft8gpu_refined) == 48 && offsetof(ft8gpu_refined, valid) == 2 && offsetof(ft8gpu_refined, pad0) == 3 &&
              offsetof(ft8gpu_refined, pt) == 4 && offsetof(ft8gpu_refined, pf) == 16 && offsetof(ft8gpu_refined, noise) == 36 &&
              offsetof(ft8gpu_refined, pad) == 40, "ft8gpu_refined layout");
#endif
/* stage entry: iq [nframes][2][48000], msgs / refined [nframes][50], n_msgs [nframes] (taken as 0 when negative, 50 when
 * larger); host or device pointers by `flags` (device form: iq 16-byte aligned).  refined[f][i] is written for i < n_msgs[f];
 * records at and behind the count are not touched.  A record need not be a decode: any cand and a91 give defined output. */
int ft8gpu_refine_messages(ft8gpu_ctx *ctx, const float *iq, const ft8gpu_message *msgs, const int32_t *n_msgs, int nframes,
                           ft8gpu_refined *refined, int flags);
/* ft8gpu_decode_messages, unchanged (msgs and n_msgs are byte for byte what it returns alone), then the stage on its records */
int ft8gpu_decode_messages_refined(ft8gpu_ctx *ctx, const float *iq, int nframes, ft8gpu_message *msgs, int32_t *n_msgs,
                                   ft8gpu_refined *refined, int flags);
/* Host helper (plain C, no GPU): seconds, hertz and decibels from one record pair; 0, or -1 when an argument is NULL or
 * refined->valid is 0 (nothing is written then).  vertex(a, b, c) = 0.5 (a - c) / (a - 2 b + c) clamped to [-0.5, 0.5], and 0
 * when a - 2 b + c >= 0 (no maximum, equal values included) or a value is not finite; evaluated in double.
 *   time:  v = vertex(pt), 0 when e_best - 1 or e_best + 1 lies outside [-16, 16];
 *          dt_s = (256 T + FT8GPU_REFINE_LEAD + 32 (e_best + v)) / 3200: the start time of the signal within the frame, so a
 *          signal ft8gpu_synth_frames starts at t0_s reports t0_s
 *   freq:  u* = the first largest of pf[1 .. 3], v = vertex(pf[u* - 1 .. u* + 1]); freq_hz = 3.125 (F + (u* - 2) + v): the
 *          frequency of tone 0
 *   snr:   snr_db = 10 log10(max(pf[2] - noise, FLT_MIN) / noise * 6.25 / 2500) clamped to [-30, 49], the range of
 *          ft8gpu_message.snr_db; noise <= 0 or not finite: 49 when pf[2] > 0, else -30
 * Bias, stated rather than hidden: the correlation of a 512-sample symbol against a tone df away is sinc^2(df / 6.25 Hz), and
 * pf samples it every half lobe width.  A parabola through three such points reads a true offset d (in steps of 3.125 Hz,
 * |d| <= 0.5) too close to the grid point: exact at d = 0 and +-0.5, short by 0.031 step at |d| = 0.1, by 0.056 at 0.2 and by
 * at most 0.069 step, 0.22 Hz, at |d| = 0.3.  In time |c|^2 falls off as (1 - |t| / 512 samples)^2 when the neighbouring
 * symbols carry other tones, a cusp no parabola fits: the vertex is short by 0.046 step at |d| = 0.1 and by at most 0.09
 * step of 32 samples, 2.9 samples, at |d| = 0.3.  Both are a tenth of the grid's error.  The SNR has a ceiling of its own: a
 * signal d steps off the grid leaks sinc^2(4 + d / 2) of its power into the empty tone, up to -25 dB, and a window up to 16
 * samples off the symbol takes in up to (16 / 512)^2, -30 dB, of a neighbouring symbol that uses that tone, so `noise` holds
 * signal once the signal is some 25 dB above the noise in 6.25 Hz: above about 0 dB the estimate reads low.
 * profiles/refine_accuracy.json has the measured errors. */
int ft8gpu_refined_estimate(const ft8gpu_message *msg, const ft8gpu_refined *refined, float *dt_s, float *freq_hz, float *snr_db);
/* ft8gpu_format_messages with the refined values: "%3d %5.2f %6.1f ~  %s\n" of the rounded snr_db, dt_s, freq_hz and text;
 * a record whose refined->valid is 0 prints its message's own snr_db, dt_s and freq_hz in the same format */
int ft8gpu_format_messages_refined(const ft8gpu_message *msgs, const ft8gpu_refined *refined, int32_t n, char *out, size_t cap);

/* ---- subtraction in the I/Q samples: decode again after the decoded signals are cancelled in the frame itself -----------------
 * (DESIGN.md "Subtraction in the I/Q samples").  Every record's waveform is rebuilt from its tones at the place the refine
 * stage found, searched once more on a grid of 0.78125 Hz by 8 samples, scaled by a smoothed complex amplitude and subtracted
 * from the float samples.  This text is the rule; tests/ft8_spec_subtract.py restates it in numpy, and the device output equals
 * the restatement byte for byte.  float32 throughout, one IEEE operation per step, nothing fused, every sum sequential in the
 * stated order from +0, every phase an exact table index formed in uint32 (4096 divides 2^32, so wrapping is harmless).
 *
 * Inputs: the frame x[j], zero outside 0 .. 47999; a record's cand and a91; its ft8gpu_refined record R.  T, F and tone[m] are
 * those of the refine rule.  u* = the first largest of R.pf[1 .. 3] (ft8gpu_refined_estimate's choice), as an index 1 .. 3.
 * (a) w4[i] = (cos, -sin)(2 pi i / 4096), i < 4096, each the float of the double value (ft8gpu_subtract_twiddles): a step of
 *     3200 / 4096 = 0.78125 Hz.  w4[4 i] is w[i] of the refine rule.
 * (b) Reference phase of a start sample S and a base index k4:  K_m = k4 + 8 tone[m];  Theta_0 = 0,
 *     Theta_(m+1) = (Theta_m + 512 K_m) mod 4096 (which is (512 m k4) mod 4096, the tones' share being whole turns);  for
 *     s_m = S + 512 m <= j < s_m + 512:  theta(j) = (Theta_m + K_m (j - s_m)) mod 4096  -- the continuous phase of CPFSK up to
 *     a constant.  z(j) = x[j] * w4[theta(j)] = (xr wr - xi wi, xr wi + xi wr).
 *     seg(S, k4, q), q = 0 .. 1263: the sum of z over j = S + 32 q .. S + 32 q + 31, ascending from +0.
 *     P(S, k4) = the sum over m = 0 .. 78, ascending from +0, of re^2 + im^2 of (seg(16 m) + ... + seg(16 m + 15), ascending
 *     from +0).
 * (c) Fine search.  S_0 = 256 T + FT8GPU_REFINE_LEAD + 32 R.e_best.  Frequency first:  pf[d + 2] = P(S_0, 4 (F + u* - 2) + d),
 *     d = -2 .. 2;  d* = the first d in ascending order whose power is strictly greater than every earlier one (-2 when none
 *     is);  k4* = 4 (F + u* - 2) + d*.  Then time:  pt[t + 2] = P(S_0 + 8 t, k4*), t = -2 .. 2;  t* likewise;
 *     S* = S_0 + 8 t*, a multiple of 8.
 * (d) Amplitude.  G(q) = seg(S*, k4*, q).  A(q) = (G(p_lo) + ... + G(p_hi)) * inv[n], both components summed ascending from
 *     +0, p_lo = max(0, q - 8), p_hi = min(1263, q + 8), n = p_hi - p_lo + 1, inv[n] = (float)(1.0 / (32 n)) from a host
 *     table (the device multiplies, it never divides).  Segments outside the frame hold zeros and still count in n.
 * (e) Subtraction, for the records i = first[f] .. n_msgs[f] - 1 of frame f in that order: for every j inside record i's 79
 *     symbols (S*_i <= j < S*_i + 40448) and inside the frame, with q = (j - S*_i) / 32 and w = w4[theta_i(j)]:
 *       x'r[j] = x'r[j] - (Ar wr + Ai wi);   x'i[j] = x'i[j] - (Ai wr - Ar wi)                      (A = A_i(q); A conj(w))
 *     Every A_i comes from the INPUT frame, not from a partly subtracted one; only this accumulation is ordered.  Samples
 *     outside every record are copied bit for bit.
 * A record with R.valid == 0 is skipped (its info is all zero); every other cand, a91 and R give defined output.
 * Samples: any float32 values give defined output, infinities and NaNs included.  Subnormal products, sums, powers and
 * amplitudes are kept, never flushed to zero (powers that underflow to +0 under amplitudes that do not: d* = t* = -2 and the
 * record is still subtracted), and a sum that overflows is the IEEE infinity.  The decisions (u*, k4, s_best, d_best, t_best,
 * valid, the padding) are exact for every input.  A comparison with a NaN is false, so a NaN is never taken as a maximum over
 * an earlier value -- in R.pf[2] or R.pf[3], in pf or in pt -- and no later value is taken over a NaN in the position a scan
 * starts from (R.pf[1], pf[0], pt[0]).  A float output (pf, pt, a sample of iq_out) that is a NaN by this rule is a NaN in every
 * implementation, with unspecified sign and payload; every other output is byte for byte, and a sample outside every record is
 * copied with the bits it has, a NaN's sign and payload included. */
#define FT8GPU_SUBTRACT_TABLE   4096    /* entries of w4 */
#define FT8GPU_SUBTRACT_SMOOTH  8       /* the amplitude is averaged over q - 8 .. q + 8: 17 segments of 32 samples */
#define FT8GPU_SUBTRACT_RANGE   2       /* both fine searches cover -2 .. 2 */
#define FT8GPU_SUBTRACT_TSTEP   8       /* samples per step of the fine time search */
typedef struct {
    int32_t k4;              /*  0  k4* */
    int32_t s_best;          /*  4  S* */
    int8_t  d_best;          /*  8  d* */
    int8_t  t_best;          /*  9  t* */
    uint8_t valid;           /* 10  1 when the record was subtracted, 0 when it was skipped (everything else zero then) */
    uint8_t pad0;            /* 11  zero */
    float   pf[5];           /* 12 */
    float   pt[5];           /* 32 */
    uint8_t pad[12];         /* 52  zero */
} ft8gpu_subtract_info;
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_subtract_info) == 64 && offsetof(ft8gpu_subtract_info, s_best) == 4 &&
               offsetof(ft8gpu_subtract_info, d_best) == 8 && offsetof(ft8gpu_subtract_info, t_best) == 9 &&
               offsetof(ft8gpu_subtract_info, valid) == 10 && offsetof(ft8gpu_subtract_info, pad0) == 11 &&
               offsetof(ft8gpu_subtract_info, pf) == 12 && offsetof(ft8gpu_subtract_info, pt) == 32 &&
               offsetof(ft8gpu_subtract_info, pad) == 52, "ft8gpu_subtract_info layout");
#else
static_assert(sizeof(ft8gpu_subtract_info) == 64 && offsetof(ft8gpu_subtract_info, s_best) == 4 &&
              offsetof(ft8gpu_subtract_info, d_best) == 8 && offsetof(ft8gpu_subtract_info, t_best) == 9 &&
              offsetof(ft8gpu_subtract_info, valid) == 10 && offsetof(ft8gpu_subtract_info, pad0) == 11 &&
              offsetof(ft8gpu_subtract_info, pf) == 12 && offsetof(ft8gpu_subtract_info, pt) == 32 &&
              offsetof(ft8gpu_subtract_info, pad) == 52, "ft8gpu_subtract_info layout");
#endif
/* host helper (plain C, no GPU): out[2 i], out[2 i + 1] = w4[i], 8192 floats */
void ft8gpu_subtract_twiddles(float *out);
/* stage entry: iq / iq_out [nframes][2][48000] (iq_out may be iq), msgs / refined / info [nframes][50], first / n_msgs
 * [nframes] (each clamped to [0, 50]); host or device pointers by `flags` (device form: iq and iq_out 16-byte aligned).
 * iq_out[f] = iq[f] with the records [first[f], n_msgs[f]) subtracted; info[f][i] is written for those records and not touched
 * elsewhere; info may be NULL. */
int ft8gpu_subtract_messages(ft8gpu_ctx *ctx, const float *iq, const ft8gpu_message *msgs, const ft8gpu_refined *refined,
                             const int32_t *first, const int32_t *n_msgs, int nframes, float *iq_out,
                             ft8gpu_subtract_info *info, int flags);
/* Multi-pass decoding with subtraction.  Pass 1 is ft8gpu_decode_messages, unchanged, on x_1 = iq.  Pass p + 1, for every frame
 * that gained records in pass p and holds fewer than 50: the records first written in pass p are refined on x_p
 * (ft8gpu_refine_messages) and subtracted from it, x_(p+1); the waterfall, sync search, candidate heap and LDPC decode run on
 * x_(p+1) with the context's params; ft8gpu_append_messages' rule appends the new unique messages (snr_db from this pass's
 * waterfall against the pass-1 baseline).  Every other frame keeps its x_p and is not decoded again.  passes in
 * [1, FT8GPU_MAX_PASSES]; msgs, n_msgs, n_by_pass as ft8gpu_decode_messages_passes; residual [nframes][2][48000] (NULL: not
 * written) receives every frame's last x_p.  iq is never written.  Host or device pointers, chunked by max_frames; the host
 * reads one int per later pass and stops early when no frame is left. */
int ft8gpu_decode_messages_subtracted(ft8gpu_ctx *ctx, const float *iq, int nframes, int passes, ft8gpu_message *msgs,
                                      int32_t *n_msgs, int32_t *n_by_pass, float *residual, int flags);

/* ---- GFSK reference: the subtraction rule with the waveform a station sends -------------------------------------------------------
 * (DESIGN.md "Subtraction in the I/Q samples", "GFSK reference".)  The rule above rebuilds a record as CPFSK, tone steps
 * abrupt.  A `shape` selects the reference: FT8GPU_SUBTRACT_CPFSK is the rule above, unchanged.  FT8GPU_SUBTRACT_GFSK is the same
 * rule but for (b') and (e'); tests/ft8_spec_subtract_gfsk.py restates it and the device output equals that byte for byte.
 * (b') Reference phase of a start sample S and a base index k4.  Q = Q_512[0 .. 1536], the pulse table of ft8gpu_gfsk_pulse(512, .)
 *     (the device uses its host's table, as the synthesiser does);  e[0] = tone[0], e[j] = tone[j - 1] for j = 1 .. 79,
 *     e[80] = tone[78].  For the local sample n' = j - S in [0, 40448), m = n' div 512, k = n' mod 512, in wrapping uint32:
 *       phi = (k4 << 20) * n' + e[m] * Q[k + 1024] + e[m + 1] * Q[k + 512] + e[m + 2] * Q[k]
 *       theta(j) = ((phi + 2^19) >> 20) & 4095
 *     -- the synthesiser's phase ("GFSK synthesis") at step = k4 * 2^20, rounded to the w4 table.  z, seg and P, both fine
 *     searches with their first-strict-maximum rule, G, A and inv, and the NaN clauses are those of (b), (c) and (d) with this
 *     theta.
 * (e') Subtraction.  r = the ramp of ft8gpu_gfsk_ramp(512, .), 64 entries.  env(n') = r[n'] for n' < 64, r[40447 - n'] for
 *     n' >= 40384, 1 otherwise.  Where env(n') != 1 the amplitude in (e) is (Ar * env, Ai * env), two float32 products formed
 *     before the products with w; elsewhere A is used as it is (no multiplication by 1.0f is part of the rule).  The ramp is
 *     NOT applied in the estimate: A stays the plain mean of (d).
 * r[0] = 0, so a record's first sample keeps its value -- unless A(0) is infinite there: inf * 0 is a NaN by IEEE, and so is
 * the sample. */
#define FT8GPU_SUBTRACT_CPFSK   0       /* shape: abrupt tone steps, the rule of "subtraction in the I/Q samples" */
#define FT8GPU_SUBTRACT_GFSK    1       /* shape: (b') and (e') */
/* ft8gpu_subtract_messages and ft8gpu_decode_messages_subtracted with the shape in front of the flags.  shape 0 gives the bytes
 * of those entries; a shape outside {0, 1} fails before anything is enqueued.  The GFSK tables are uploaded on the first call
 * with shape 1 and freed at ft8gpu_destroy.  The refine stage of the pass loop is the same for both shapes. */
int ft8gpu_subtract_messages_shaped(ft8gpu_ctx *ctx, const float *iq, const ft8gpu_message *msgs, const ft8gpu_refined *refined,
                                    const int32_t *first, const int32_t *n_msgs, int nframes, float *iq_out,
                                    ft8gpu_subtract_info *info, int shape, int flags);
int ft8gpu_decode_messages_subtracted_shaped(ft8gpu_ctx *ctx, const float *iq, int nframes, int passes, ft8gpu_message *msgs,
                                             int32_t *n_msgs, int32_t *n_by_pass, float *residual, int shape, int flags);

/* ---- demodulation from the I/Q samples: undecoded candidates demodulated again from the frame itself ----------------------------
 * (DESIGN.md "Demodulation from the I/Q samples"; not in the reference.)  OSD, AP, matching and combining all start from the
 * soft bits of ft8_extract_likelihood: one byte per waterfall cell in half-decibel steps, a 1024-sample Hann window over
 * 512-sample symbols, a grid of 256 samples by 3.125 Hz, one symbol at a time.  For a candidate BP has given up on, this stage
 * goes back to the float samples: a fine Costas sync within the candidate's cell, a matched 512-sample correlation per tone with
 * a phase that is continuous over the signal, and max-log soft bits over blocks of one, two and three symbols (WSJT-X ft8b's
 * nsym = 1, 2, 3), each set tried with bp_decode.  This text is the rule; tests/ft8_spec_demod.py restates it in numpy, and the
 * device output equals the restatement byte for byte.  float32 throughout, one IEEE operation per step, nothing fused, every
 * phase an exact table index formed in uint32 (4096 divides 2^32, so wrapping is harmless).
 *
 * Inputs: the frame x[j] = (I[j], Q[j]), j < 48000, zero for every other j; a candidate with T = 2 * time_offset + time_sub and
 * F = 2 * freq_offset + freq_sub; w4 of the subtraction rule (ft8gpu_subtract_twiddles).  Complex products are
 * (a * b) = (ar * br - ai * bi,  ar * bi + ai * br), with b the table entry.
 * A candidate qualifies as for OSD, AP, matching and combining: ok == 0 and ldpc_errors != 0.  Of a frame's qualifying
 * candidates, in candidate order, the first max_per_frame are attempted; every other record below counts[f] gets status_out =
 * status_in and an all-zero info record.
 * (a) Correlation.  C(m, t; S, k4), the correlation of symbol m (m < 79) of a signal that starts at sample S with tone t at table
 *     step k4 + 8 t, is formed by 64 lanes l:  n = 512 m + l + 64 a, a < 8;
 *       y_a = x[S + n] * w4[(k4 * n) mod 4096]                       (the base frequency, phase counted from the signal's start)
 *       U_t = the sum over a of y_a * exp(-2 pi i t a / 8), as the radix-2 DFT below
 *       V_t(l) = U_t * w4[(8 t l) mod 4096]
 *       C = V_t summed over the lanes by the xor butterfly: for mask = 1, 2, 4, 8, 16, 32 in turn, v(l) = v(l) + v(l xor mask)
 *           for every lane at once, both components (addition commutes, so all lanes end with the same value)
 *     This is x[S + n] times exp(-2 pi i (k4 + 8 t) n / 4096) because 8 t * (512 m + 64 a + l) = 8 t l + 512 t a modulo 4096.  For
 *     a CPFSK signal that starts at S with tone 0 at k4, every symbol's correlation at its own tone has the same phase, the
 *     signal's initial one (8 t * 512 m is a whole number of turns; the subtraction rule's Theta recurrence is the same fact),
 *     which is what makes sums across symbols coherent.
 *     DFT, with c = 0.70710677f (0x3F3504F3) and every line one operation per component:
 *       p_a = y_a + y_(a+4),  q_a = y_a - y_(a+4),  a < 4
 *       q'_0 = q_0;  q'_1 = ((q_1r + q_1i) * c, (q_1i - q_1r) * c);  q'_2 = (q_2i, -q_2r);
 *       q'_3 = ((q_3i - q_3r) * c, -((q_3r + q_3i) * c))
 *       DFT4(v): e0 = v0 + v2, e1 = v0 - v2, o0 = v1 + v3, o1 = v1 - v3;  out0 = e0 + o0,  out1 = (e1r + o1i, e1i - o1r),
 *                out2 = e0 - o0,  out3 = (e1r - o1i, e1i + o1r)
 *       U_(2s) = DFT4(p)_s,  U_(2s+1) = DFT4(q')_s
 * (b) Fine sync.  S(e) = 256 T + FT8GPU_REFINE_LEAD + 32 e.  Psync(e, d) = the sum over the 21 Costas symbols (m = 0..6, 36..42,
 *     72..78, ascending from +0) of re * re + im * im of C(m, costas[m mod 36]; S(e), 4 F + d).  Time first: e = -4 .. 4 at d = 0;
 *     e* = the first e in ascending order whose power is strictly greater than every earlier one (-4 when none is).  Then
 *     frequency: d = -2 .. 2 at e*, d* likewise.  That covers the candidate's own cell, +-128 samples and +-1.5625 Hz.
 *     psync = Psync(e*, d*); a NaN is stored as 0x7FC00000.  (Every hypothesis is correlated anew from the samples with its own
 *     phase origin S(e); segment sums on the absolute index, which refine slides over e, would give every e another phase
 *     reference than Z has and a second definition of C.)
 * (c) Spectra.  Z[m][t] = C(m, t; S(e*), 4 F + d*), m < 79, t < 8.
 * (d) Three sets of soft bits, n = 1, 2, 3.  Each half has 29 data symbols, m = 7 + i or 43 + i, i < 29, and is cut from i = 0
 *     into consecutive blocks of n symbols, the last one shorter (n = 2: 14 pairs and a single; n = 3: 9 triples and a pair).  For
 *     a block of b symbols m1 .. mb and each of the 8^b tone tuples:  s = Z[m1][t1] + ... + Z[mb][tb], added in symbol order,
 *     A = sqrtf(sr * sr + si * si), the correctly rounded root.  The 3 b bits of a tuple are the inverse Gray map of each tone,
 *     MSB first, symbols in order; data symbol i of half h owns codeword bits 87 h + 3 i .. + 2.
 *       llr[bit] = max(A over the tuples with the bit set) - max(A over the tuples with it clear)
 *     -- the sign of ft8_extract_likelihood.  Every A is >= +0 or not finite, so the maxima do not depend on an order.  A set
 *     with an A that is not finite (infinite or NaN) has result 6.  x = ftx_normalize_logl(llr) exactly as the soft-bit memory
 *     writes it (sum and sum of squares in index order); a non-finite x[i]: result 6.
 * (e) Decoding.  For the sets named in `sets` (bit n - 1), in ascending n: bp_decode(x, ldpc_iters), bit-exact to the LDPC
 *     kernel's iteration.  The first failing check names the set's result: 6 non-finite, 7 no codeword within ldpc_iters,
 *     5 all-zero (kept for the numbering and never produced: bp_decode leaves at an all-zero word before it counts, so such a
 *     word ends in 7), 2 nhard > max_hard_errors (nhard = the positions where the codeword differs from x > 0), 3 CRC,
 *     4 unpack77 < 0, else 1 = accepted.  The first accepted
 *     set ends the candidate; otherwise result is the last attempted set's.  info.set is the set `result` speaks of, info.nhard
 *     that set's (0 without a codeword).  On acceptance the status record becomes that of a BP success, exactly as OSD, AP,
 *     matching and combining write it; otherwise it is unchanged. */
#define FT8GPU_DEMOD_TSTEP     32      /* samples per step of the fine time search */
#define FT8GPU_DEMOD_TRANGE    4       /* e = -4 .. 4 */
#define FT8GPU_DEMOD_FRANGE    2       /* d = -2 .. 2, in steps of 0.78125 Hz */
typedef struct {
    uint8_t result;          /*  0  0 not attempted, 1 accepted, 2 .. 7 the failing check of `set` */
    uint8_t set;             /*  1  1 .. 3, or 0 */
    uint8_t nhard;           /*  2 */
    int8_t  e_best;          /*  3  e* */
    int8_t  d_best;          /*  4  d* */
    uint8_t pad0[3];         /*  5  zero */
    float   psync;           /*  8  Psync(e*, d*) */
    uint8_t pad[4];          /* 12  zero */
} ft8gpu_demod_info;
typedef struct {
    int32_t sets;            /* 1 .. 7: bit n - 1 = set n is tried; FT8GPU_DEMOD_SETS is the recommended value */
    int32_t max_hard_errors; /* 0 .. 174; FT8GPU_DEMOD_MAX_HARD_ERRORS is the recommended value */
    int32_t max_per_frame;   /* 0 .. max_candidates: the qualifying candidates attempted per frame */
} ft8gpu_demod_params;
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_demod_info) == 16 && offsetof(ft8gpu_demod_info, set) == 1 && offsetof(ft8gpu_demod_info, nhard) == 2 &&
               offsetof(ft8gpu_demod_info, e_best) == 3 && offsetof(ft8gpu_demod_info, d_best) == 4 &&
               offsetof(ft8gpu_demod_info, pad0) == 5 && offsetof(ft8gpu_demod_info, psync) == 8 &&
               offsetof(ft8gpu_demod_info, pad) == 12, "ft8gpu_demod_info layout");
_Static_assert(sizeof(ft8gpu_demod_params) == 12 && offsetof(ft8gpu_demod_params, max_hard_errors) == 4 &&
               offsetof(ft8gpu_demod_params, max_per_frame) == 8, "ft8gpu_demod_params layout");
#else
static_assert(sizeof(ft8gpu_demod_info) == 16 && offsetof(ft8gpu_demod_info, set) == 1 && offsetof(ft8gpu_demod_info, nhard) == 2 &&
              offsetof(ft8gpu_demod_info, e_best) == 3 && offsetof(ft8gpu_demod_info, d_best) == 4 &&
              offsetof(ft8gpu_demod_info, pad0) == 5 && offsetof(ft8gpu_demod_info, psync) == 8 &&
              offsetof(ft8gpu_demod_info, pad) == 12, "ft8gpu_demod_info layout");
static_assert(sizeof(ft8gpu_demod_params) == 12 && offsetof(ft8gpu_demod_params, max_hard_errors) == 4 &&
              offsetof(ft8gpu_demod_params, max_per_frame) == 8, "ft8gpu_demod_params layout");
#endif
/* Recommended values, from profiles/demod_gain.json (tools/demod_gain.py, on the CPU with the oracle's stages and the
 * restatement: the 96 CQ frames of 20 stations at -22 .. 0 dB of the OSD, AP and match figures, where BP alone decodes 1046 of
 * the 1920 planted messages and leaves 7119 failing candidates; one station per frame at -24 .. -16 dB in steps of 1 dB, 64
 * frames each, start and frequency off the grid; 96 frames of noise; gates 20, 25, 30, 36, 40, 45, 50, 60, 174; every mask).
 * max_hard_errors: no row accepts a message that was not on the air at any gate under any mask, and a gate only costs messages
 * (107, 119, 120 gained on the CQ frames at 20, 25, 30 and 120 from there to 174: a word BP converges to lies within 30
 * positions of its soft bits), so the largest swept gate, 174 -- no gate -- is the recommended one.  What keeps a wrong word out is BP itself with the CRC and unpack77 behind
 * it; on noise (942 failing candidates) nothing is accepted.
 * sets: the CQ frames gain 63, 93, 99 with set 1, 2, 3 alone, 99, 110, 116 with masks 3, 5, 6 and 120 with all three; the
 * smallest mask within 2 % of 120 is 7.  Sets 2 and 3 are not idle: the coherent blocks gain half as much again as set 1.
 * One station per frame, decoded fraction BP / set 1 / set 2 / set 3 / all: -21 dB 0 / .03 / .16 / .14 / .16; -20 dB .09 /
 * .28 / .52 / .56 / .64; -19 dB .23 / .80 / .78 / .72 / .88; -18 dB .77 / 1 / 1 / .98 / 1; all 1 from -17 dB, all 0 to -23 dB
 * but for one of 64 at -22 dB with set 3: the half-decode point moves from about -18.5 dB to about -20.2 dB. */
#define FT8GPU_DEMOD_MAX_HARD_ERRORS 174
#define FT8GPU_DEMOD_SETS 7
/* stage entry: iq [nframes][2][48000], cands / status_in / status_out / info [nframes][max_candidates], counts [nframes]; host
 * or device pointers by `flags` (device form: iq 16-byte aligned).  ldpc_iters is the context's.  Records below counts[f] are
 * written, records at and behind it are not touched.  status_out may be status_in.  Any candidate gives defined output. */
int ft8gpu_demod_candidates(ft8gpu_ctx *ctx, const float *iq, const ft8gpu_candidate *cands, const int32_t *counts,
                            const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_demod_params *params,
                            ft8gpu_decode_status *status_out, ft8gpu_demod_info *info, int flags);
/* The whole path over iq [nframes][2][48000]:
 *   1. the records [0, n1) are byte for byte those of ft8gpu_decode_messages;
 *   2. ft8gpu_demod_candidates runs in place on the frame's BP status records;
 *   3. the append step of the multi-pass path adds, in candidate order, every unique gained message not yet among the frame's
 *      records, up to 50 in all; pad[3] of such a record is the accepted set (1 .. 3).
 * n_by_stage [nframes][2] (NULL: not written): the count after BP and after the stage.  Host or device pointers by `flags`
 * (device form: iq and msgs 16-byte aligned), chunked by max_frames.  Composed with AP on its own soft bits below
 * (ft8gpu_decode_messages_demod_ap); not composed with multi-pass, OSD, matching, call hints or combining: feeding these soft
 * bits to those stages is left to a later change, and ft8gpu_demod_soft's array is the interface they would use. */
int ft8gpu_decode_messages_demod(ft8gpu_ctx *ctx, const float *iq, int nframes, const ft8gpu_demod_params *params,
                                 ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags);

/* ---- a-priori decoding on the soft bits demodulated from the I/Q samples --------------------------------------------------------
 * (DESIGN.md "A-priori decoding on the demodulated soft bits"; not in the reference.)  The demodulation above is the only stage
 * that improves the soft bits themselves; ft8gpu_demod_soft hands them out, and ft8gpu_ap_soft_candidates runs the a-priori rule
 * on them.  tests/ft8_spec_apsoft.py restates both, and the device output equals the restatement byte for byte.
 *
 * The soft-bit array: soft [nframes][max_candidates][3][FT8GPU_SOFT_STRIDE] float32, 2112 bytes per candidate; row n - 1 belongs
 * to set n, elements 174 and 175 of a row are +0.
 * ft8gpu_demod_soft is ft8gpu_demod_candidates with one more output: status_out and info are byte for byte those of
 * ft8gpu_demod_candidates with the same arguments.  For every record below counts[f], row n - 1 holds x, the output of
 * ftx_normalize_logl that set n's bp_decode ran on, where the candidate was attempted, set n is named in `sets`, no earlier set
 * was accepted and the set's result is not 6 (the accepted set's own row is written too); every other row is 176 times +0
 * (candidates not attempted, sets not named or not reached, non-finite sets).  Records at and behind the count keep the
 * caller's bytes, in all three arrays.  Host or device pointers by `flags` (device form: iq and soft 16-byte aligned). */
#define FT8GPU_SOFT_STRIDE 176
int ft8gpu_demod_soft(ft8gpu_ctx *ctx, const float *iq, const ft8gpu_candidate *cands, const int32_t *counts,
                      const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_demod_params *params,
                      ft8gpu_decode_status *status_out, ft8gpu_demod_info *info, float *soft, int flags);
/* AP on a soft-bit array.  A candidate qualifies as for AP: ok == 0 and ldpc_errors != 0.  The sets named in `sets` (1 .. 7,
 * bit n - 1 = set n) are walked in ascending n.  A row with a non-finite value among its 174, or with apmag = max |row[i]| == 0,
 * is unusable: nothing is tried on it and its code is 6 (in results[n - 1][0]).  Within a usable row the hypotheses run in table
 * order, each exactly by the per-hypothesis rule of ft8gpu_ap_candidates with llr = the row as it stands -- nothing is
 * normalised again: forced positions at +-apmag, bp_decode(llr_k, ldpc_iters) bit-exact to the LDPC kernel's iteration, nhard
 * on the unmasked positions against h = row > 0, and the codes 7, 8, 5, 2, 3, 4, 1 in that order.  The first accepted
 * (set, hypothesis) ends the candidate, and the status record becomes that of a BP success as AP writes it; otherwise it is
 * unchanged.  result, nhard, hyp, iters speak of the accepted (set, hypothesis) or of the last one tried, `set` names its set;
 * if no set is usable, result = 6 and set = 0.  A candidate that does not qualify gets its record copied and an all-zero info
 * record; records at and behind counts[f] are not touched.  status_out may be status_in.  Any contents of soft give defined
 * output (elements 174 and 175 of a row are not read).  hyps [nhyp], always in host memory, are validated as
 * ft8gpu_ap_candidates validates them; nhyp in [1, 4], max_hard_errors in [0, 174], ldpc_iters is the context's.  Host or
 * device pointers by `flags` (device form: soft 16-byte aligned). */
typedef struct {
    uint8_t result;          /*  0  0 not attempted, 1 accepted, 2..5, 7, 8 as ft8gpu_ap_info, 6 no usable set */
    uint8_t nhard, hyp, iters;   /* of (set, hyp) */
    uint8_t set;             /*  4  1 .. 3: the accepted set, or the last one tried; 0 when none was */
    uint8_t pad[3];          /*     zero */
    uint8_t results[3][FT8GPU_AP_MAX_HYPOTHESES];   /*  8  the code of every (set, hypothesis) tried, 0 for the others;
                                                            a set that is unusable has 6 in results[n-1][0] */
} ft8gpu_apsoft_info;
/* Recommended max_hard_errors, from profiles/demod_ap_gain.json (tools/demod_ap_gain.py, on the CPU with the oracle's stages and
 * the restatements, on the rows of tools/demod_gain.py behind the demodulation at its recommended values; gates 20, 25, 30, 36,
 * 40, 45, 50, 60, 174; "CQ ? ?" alone, and with three call hypotheses nobody on the air carries).  On the 96 CQ frames of 20
 * stations (1046 of 1920 by BP, +120 by the demodulation, 4840 candidates still failing) AP on these soft bits gains 35, 48, 48,
 * 49 planted messages at gates 20, 25, 30, 36 and 49 from there to 174.  One station per frame, 64 frames each, gained behind
 * the demodulation at gate 36 and above: -23 dB 2, -22 dB 2 (demodulation 1), -21 dB 14 (10), -20 dB 11 (35, BP 6), -19 dB 8
 * (41, BP 15: all 64 decoded), none needed from -18 dB; at 20 and 25 the -21 dB row gains 10 and 13.  No row accepts a message
 * that was not on the air at any gate under either table -- not on the 96 noise frames (942 failing candidates) either -- so by
 * the rule of FT8GPU_DEMOD_MAX_HARD_ERRORS the largest swept gate, 174 -- no gate -- is the recommended one: a gate only costs
 * messages here, and what keeps a wrong word out is BP under the forced bits with the CRC and unpack77 behind it.  The three
 * unrelated call hypotheses change no figure of the sweep. */
#define FT8GPU_APSOFT_MAX_HARD_ERRORS 174
int ft8gpu_ap_soft_candidates(ft8gpu_ctx *ctx, const float *soft, const int32_t *counts, const ft8gpu_decode_status *status_in,
                              int nframes, int sets, const ft8gpu_ap_hypothesis *hyps, int nhyp, int max_hard_errors,
                              ft8gpu_decode_status *status_out, ft8gpu_apsoft_info *info, int flags);
/* The whole path over iq [nframes][2][48000]: steps 1 to 3 of ft8gpu_decode_messages_demod (through the kernel that writes the
 * soft bits); then ft8gpu_ap_soft_candidates runs in place on the status records with sets = demod.sets, the append step adds
 * its unique gained messages in candidate order, and pad[1] = 1 + the accepted hypothesis, pad[3] = the accepted set on them.
 * n_by_stage [nframes][3] (NULL: not written): the count after BP, after the demodulation and after AP.  nhyp = 0: no AP --
 * the messages, counts and first two columns of ft8gpu_decode_messages_demod, column 2 equal to column 1.  Chunked by
 * max_frames; the soft array of a chunk (max_frames x max_candidates x 2112 bytes) is the context's, allocated on the first
 * call with nhyp > 0 -- a failed allocation returns -1 with the error text and leaves the context usable. */
typedef struct {
    ft8gpu_demod_params demod;
    int32_t nhyp;                   /* 0 (no AP) .. FT8GPU_AP_MAX_HYPOTHESES */
    int32_t ap_max_hard_errors;     /* 0 .. 174; FT8GPU_APSOFT_MAX_HARD_ERRORS is the recommended value */
    ft8gpu_ap_hypothesis hyps[FT8GPU_AP_MAX_HYPOTHESES];
} ft8gpu_demod_ap_params;
int ft8gpu_decode_messages_demod_ap(ft8gpu_ctx *ctx, const float *iq, int nframes, const ft8gpu_demod_ap_params *params,
                                    ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags);
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_apsoft_info) == 20 && offsetof(ft8gpu_apsoft_info, nhard) == 1 && offsetof(ft8gpu_apsoft_info, hyp) == 2 &&
               offsetof(ft8gpu_apsoft_info, iters) == 3 && offsetof(ft8gpu_apsoft_info, set) == 4 &&
               offsetof(ft8gpu_apsoft_info, pad) == 5 && offsetof(ft8gpu_apsoft_info, results) == 8, "ft8gpu_apsoft_info layout");
_Static_assert(sizeof(ft8gpu_demod_ap_params) == 100 && offsetof(ft8gpu_demod_ap_params, nhyp) == 12 &&
               offsetof(ft8gpu_demod_ap_params, ap_max_hard_errors) == 16 && offsetof(ft8gpu_demod_ap_params, hyps) == 20,
               "ft8gpu_demod_ap_params layout");
#else
static_assert(sizeof(ft8gpu_apsoft_info) == 20 && offsetof(ft8gpu_apsoft_info, nhard) == 1 && offsetof(ft8gpu_apsoft_info, hyp) == 2 &&
              offsetof(ft8gpu_apsoft_info, iters) == 3 && offsetof(ft8gpu_apsoft_info, set) == 4 &&
              offsetof(ft8gpu_apsoft_info, pad) == 5 && offsetof(ft8gpu_apsoft_info, results) == 8, "ft8gpu_apsoft_info layout");
static_assert(sizeof(ft8gpu_demod_ap_params) == 100 && offsetof(ft8gpu_demod_ap_params, nhyp) == 12 &&
              offsetof(ft8gpu_demod_ap_params, ap_max_hard_errors) == 16 && offsetof(ft8gpu_demod_ap_params, hyps) == 20,
              "ft8gpu_demod_ap_params layout");
#endif

/* ---- 12 kHz audio: a resampler in front of the decoder ------------------------------------------------------------------------
 * (DESIGN.md "Audio front end"; not in the reference, whose frames come from the RTL-SDR front end or from .iq / .c2 files.)
 * Recordings, WSJT-X .wav saves and web receivers deliver 12 000 sps real audio.  A band of such a clip becomes one frame of the
 * decoder: mixed down from the band's centre, low-pass filtered, resampled by 4/15 to 3200 sps and moved back to the band's lower
 * edge.  The decoder reads FFT bins 0 .. 511 of a frame, 1600 Hz, so the usual 200 .. 3100 Hz passband takes two bands.
 * The rule is exact: float32, one IEEE operation per step, nothing fused; every sum is sequential from +0 in the stated order;
 * every index is integer arithmetic.
 *
 * Input.  a[n], 0 <= n < nsamples, 1 <= nsamples <= FT8GPU_AUDIO_NSAMPLES, zero outside.  FT8GPU_AUDIO_S16: a[n] = (float)pcm[n] *
 * 2^-15 (exact); FT8GPU_AUDIO_F32: the caller's floats as they are.
 * Band.  base_bin in [0, FT8GPU_AUDIO_MAX_BASE], in units of 6.25 Hz: the band covers 6.25 base_bin .. 6.25 base_bin + 1600 Hz of
 * the audio (704 is the last base whose band ends at or below 6000 Hz).
 * Mixer.  wm[i] = (cos, -sin)(2 pi i / 1920), each the float of the double value (ft8gpu_audio_mixer);
 *   z[n] = a[n] * wm[(n * (base_bin + 128)) mod 1920], two products.  The mixer frequency is the band's centre, 6.25 base_bin + 800
 *   Hz; 12000 / 6.25 = 1920, so the table is periodic and the phase exact.
 * Taps.  h[k], k = 0 .. 158, and h[159] = 0 (ft8gpu_audio_taps): with d = k - 79, in double,
 *   h[k] = (float)(((8 * (3200 / 48000)) * sinc((3200 * d) / 48000) * I0(8 * sqrt(1 - (d / 80)^2))) / I0(8)),
 *   sinc(u) = sin(pi u) / (pi u) and 1 at u = 0;  I0(x) = 1 + sum over k = 1 .. 39 of T_k, T_0 = 1, T_k = T_(k-1) * (x / (2 k))^2.
 *   A Kaiser low-pass (beta 8) at the 48 kHz up-sampled rate with its cutoff at 1600 Hz; the gain is 4 for the zero stuffing times
 *   2, so that a real cosine of amplitude A arrives as a complex tone of amplitude A.  Passband (0 .. 800 Hz either side of the
 *   centre) within -0.0004 .. +0.0007 dB; stopband (2400 Hz and beyond, the only offsets that alias into the bins the decoder
 *   reads) at most -82.6 dB.
 * Resampler.  For m = 0 .. 47999: t = 15 m + 79, r = t mod 4, N = t div 4;
 *   y[m] = sum over j = 0 .. 39, ascending, of h[r + 4 j] * z[N - j], real and imaginary parts separately, each term a product
 *   and then an add.  The filter is centred, so a record's dt_s refers to the clip's own time axis.
 * Back to the band's lower edge.  x[m] = y[m] * j^m, exactly: m mod 4 = 0: (yr, yi); 1: (-yi, yr); 2: (-yr, -yi); 3: (yi, -yr).
 *   Negation flips the sign bit, also that of a zero.  The frame is planar, [2][48000].
 * Any float input is defined: infinities, NaNs and subnormals are kept, not flushed.  An output that is a NaN by this rule is a NaN
 * in every implementation (sign and payload unspecified); every other output is the same bytes everywhere.  Every clip starts from
 * reset: no filter state is carried from one clip into the next. */
#define FT8GPU_AUDIO_RATE      12000
#define FT8GPU_AUDIO_NSAMPLES  180000  /* 15 s */
#define FT8GPU_AUDIO_TAPS      160
#define FT8GPU_AUDIO_MIX       1920
#define FT8GPU_AUDIO_MAX_BANDS 4
#define FT8GPU_AUDIO_MAX_BASE  704
#define FT8GPU_AUDIO_S16       0       /* pcm: int16_t [nclips][nsamples] */
#define FT8GPU_AUDIO_F32       1       /* pcm: float   [nclips][nsamples] */
/* the tables of the rule (host, plain C): h[0 .. 159], and wm as 1920 (cos, -sin) pairs */
void ft8gpu_audio_taps(float out[FT8GPU_AUDIO_TAPS]);
void ft8gpu_audio_mixer(float out[2 * FT8GPU_AUDIO_MIX]);
/* stage entry: pcm [nclips][nsamples] of `format`, base_bin [nbands] (host memory in both pointer forms) -> iq_out
 * [nclips][nbands][2][48000].  Host or device pointers by `flags` (device form: iq_out 16-byte aligned), clips in chunks of
 * max_frames.  nbands outside [1, 4], a base outside [0, 704], an unknown format and nsamples outside [1, 180000] are refused
 * before anything is enqueued. */
int ft8gpu_audio_frames(ft8gpu_ctx *ctx, const void *pcm, int format, int nclips, int nsamples, const int32_t *base_bin,
                        int nbands, float *iq_out, int flags);
/* The whole path: the frames of every (clip, band) go through the ft8gpu_decode_messages path, at most max_frames at a time, in a
 * frame buffer the context allocates on the first call (max_frames frames; a failed allocation leaves the context usable) and
 * frees at ft8gpu_destroy.  Then the bands of a clip are merged: walking the bands in the caller's order and a band's records in
 * their order, a record whose 12 a91 bytes equal those of a record already kept for the clip is dropped; a kept record is the
 * band's record with freq_hz = (cand.freq_offset + base_bin + (float)cand.freq_sub / 2) * 6.25f (the integer add first) and
 * pad[0] = the band's index; the walk stops at 50 * nbands records.  msgs [nclips][50 * nbands], n_msgs [nclips]; slots at and
 * behind n_msgs[c] are left untouched.  Arguments are refused as by ft8gpu_audio_frames. */
int ft8gpu_decode_audio(ft8gpu_ctx *ctx, const void *pcm, int format, int nclips, int nsamples, const int32_t *base_bin,
                        int nbands, ft8gpu_message *msgs, int32_t *n_msgs, int flags);
/* Reads a RIFF/WAVE file of PCM (format tag 1), mono, 16 bit, 12000 Hz into out[0 .. cap): *nsamples = min(samples in the file,
 * cap).  Chunks other than "fmt " and "data" (LIST, ...) are skipped, odd-sized chunks are padded to even.  Everything else is
 * refused with a line on stderr that names what was found: 0 = ok, -1 = refused (*nsamples = 0). */
int ft8gpu_read_wav(const char *path, int16_t *out, int32_t cap, int32_t *nsamples);

/* ---- wideband RX: many channels from one 2.4 Msps capture ----------------------------------------------------------------------
 * (DESIGN.md "Wideband RX"; not in the reference, whose rtlsdr_callback keeps one 1.6 kHz band of a capture -- that one is
 * ft8gpu_rx_decimate.)  A 2.4 Msps capture holds 2.4 MHz of spectrum; every channel the caller names becomes one frame of the
 * decoder, and the capture's bytes are read once for all of them.  The rule is exact: stage A is integer arithmetic, stage B
 * float32 with one IEEE operation per step, nothing fused, every sum sequential from +0 in the stated order.
 *
 * Input.  raw: unsigned bytes, I and Q interleaved, at FT8GPU_WIDE_RATE.  x[n] = (raw[2n] - 128) + i (raw[2n+1] - 128) as
 *   integers (raw ^ 0x80 read as int8), 0 <= n < npairs, zero outside.  npairs is a positive multiple of 8, at most
 *   FT8GPU_WIDE_MAX_PAIRS; every capture is 16-byte aligned.
 * Channel.  freq_bin in units of 6.25 Hz from the capture's centre, |freq_bin| <= FT8GPU_WIDE_MAX_BIN (+-1.1 MHz).  The frame's
 *   0 Hz is the centre + 6.25 freq_bin, and the decoder's bins 0 .. 511 are the 1600 Hz above it (a USB dial frequency).
 *   F = freq_bin + 128 is the band's centre; c = floor((F + 32) / 64); q = F - 64 c, in [-32, 31].
 * Stage A, integers.  w1[i] = (lrint(32767 cos(2 pi i / 6000)), -lrint(32767 sin(2 pi i / 6000))) as int16, computed in double
 *   (ft8gpu_wide_mixer1).  u[n] = x[n] * w1[(n c) mod 6000] (the mathematical mod), a complex integer product: it mixes down by
 *   400 c Hz, and each component is below 2^23.  g[0 .. 496] is the four-fold convolution of a 125-sample boxcar (symmetric about
 *   j = 248, sum 125^4).  v[m] = sum over j of g[j] * u[125 m + 248 - j] in int64: a fourth-order CIC decimating by 125 to
 *   19 200 sps, centred on sample 125 m.  |v| < 2^52: nothing wraps, and the value is the same however it is summed.
 * Stage B, float32.  vf[m] = ((float)Re v[m] * c0, (float)Im v[m] * c0), the conversion rounding to nearest even,
 *   c0 = (float)(1 / (32767 * 125^4 * 128)).  w2[i] = (cos, -sin)(2 pi i / 3072), each the float of the double value
 *   (ft8gpu_wide_mixer2).  z[m] = vf[m] * w2[(m q) mod 3072]: zr = vr * wr - vi * wi, zi = vr * wi + vi * wr, four products, one
 *   subtraction, one addition.
 *   Taps (ft8gpu_wide_taps), in double: t[k] = (sinc((3200 * d) / 19200) * I0(9 * sqrt(1 - (d / 46)^2))) / I0(9) for k = 0 .. 92,
 *   d = k - 46, and 0 outside (sinc and I0 as in the audio stage above); hh[i] = ((1 + 2 a) * t[i-1] - a * t[i]) - a * t[i-2],
 *   i = 0 .. 94, a = 0.1685 (the CIC's droop compensation); s = the sum of hh, i ascending from 0; h[i] = (float)(hh[i] / s);
 *   h[95] = 0.  95 taps centred on 47.
 *   y[p] = sum over k = 0 .. 94, ascending, of h[k] * z[6 p + 47 - k], real and imaginary parts separately, each term a product
 *   and then an add, for 0 <= p < 48000.  Output p is centred on input sample 750 p: a record's dt_s is on the capture's time axis.
 *   out[p] = y[p] * j^p as swaps and negations: p mod 4 = 0: (yr, yi); 1: (-yi, yr); 2: (-yr, -yi); 3: (yi, -yr), where -a is
 *   0 - a, so that a zero stays +0.  All 48000 outputs follow the rule; where the window holds no sample they are +0.
 *   The frame is planar, [2][48000].  normalise != 0 then scales the frame by (float)(0.5 / (double)max(1e-24f, peak)), peak the
 *   largest |value| of both planes: the peak normalisation of ft8gpu_rx_decimate.
 * Whole chain, float taps times the exact response of g, over every q: at most -84 dB at or beyond 2400 Hz from the band's centre
 * (the only offsets that alias into the bins the decoder reads), within +-0.057 dB up to 800 Hz (the CIC's tilt at the 200 Hz
 * residual of |q| = 32; +-0.0003 dB at q = 0).  Every capture starts from zero state. */
#define FT8GPU_WIDE_RATE         2400000
#define FT8GPU_WIDE_MAX_PAIRS    36000000   /* 15 s */
#define FT8GPU_WIDE_MIX1         6000
#define FT8GPU_WIDE_MIX2         3072
#define FT8GPU_WIDE_TAPS         96
#define FT8GPU_WIDE_MAX_CHANNELS 16
#define FT8GPU_WIDE_MAX_BIN      176000
/* the tables of the rule (host, plain C): w1 as 6000 int16 pairs, w2 as 3072 float pairs, h[0 .. 95] */
void ft8gpu_wide_mixer1(int16_t out[2 * FT8GPU_WIDE_MIX1]);
void ft8gpu_wide_mixer2(float out[2 * FT8GPU_WIDE_MIX2]);
void ft8gpu_wide_taps(float out[FT8GPU_WIDE_TAPS]);
/* stage entry: raw [ncaptures][2 * npairs], freq_bin [nchannels] (host memory in both pointer forms) -> iq
 * [ncaptures][nchannels][2][48000].  Host or device pointers by `flags` (device form: raw and iq 16-byte aligned), captures in
 * chunks of max_frames.  Refused before anything is enqueued, the outputs untouched: a NULL context or array, nchannels outside
 * [1, 16], a freq_bin beyond +-176000, npairs zero, not a multiple of 8 or above 36 000 000, a misaligned raw (device form).
 * The 19 200 sps planes between the stages are allocated on the first call (a failed allocation is reported and leaves the
 * context usable) and freed at ft8gpu_destroy. */
int ft8gpu_wide_frames(ft8gpu_ctx *ctx, const uint8_t *raw, int ncaptures, size_t npairs, const int32_t *freq_bin,
                       int nchannels, float *iq, int normalise, int flags);
/* The whole path: the frames capture * nchannels + channel, normalised, go through the ft8gpu_decode_messages path, at most
 * max_frames at a time.  Then the channels of a capture are merged: walking the channels in the caller's order and a channel's
 * records in their order, a record is dropped if its 12 a91 bytes equal those of a record already kept for the capture whose
 * channel lies less than 256 bins away (the bands overlap); a kept record is the channel's record with freq_hz =
 * (cand.freq_offset + freq_bin + (float)cand.freq_sub / 2) * 6.25f (the integer add first; exact, on the capture's axis relative
 * to its centre, possibly negative) and pad[0] = the channel's index; the walk stops at 50 * nchannels records.
 * msgs [ncaptures][50 * nchannels], n_msgs [ncaptures]; records at and behind n_msgs[c] are left untouched.  Arguments are
 * refused as by ft8gpu_wide_frames. */
int ft8gpu_decode_wide(ft8gpu_ctx *ctx, const uint8_t *raw, int ncaptures, size_t npairs, const int32_t *freq_bin,
                       int nchannels, ft8gpu_message *msgs, int32_t *n_msgs, int flags);

/* ---- PCM front end: 48 .. 768 ksps real or complex samples, many channels from one capture -------------------------------------
 * (DESIGN.md "PCM front end"; not in the reference.)  Sound cards deliver 48 kHz real audio; Hermes-Lite 2, Red Pitaya, Airspy
 * HF+, SDRplay and Flex DAX-IQ deliver complex baseband at 48 .. 768 ksps, and SDR programs save it as two-channel .wav files.
 * Every channel the caller names becomes one frame of the decoder; a capture's samples are read once for all of them.  The rule is
 * exact: float32, one IEEE operation per step, nothing fused; every sum is sequential from +0 in the stated order; every index is
 * integer arithmetic.
 *
 * Input.  rate = 3200 D, D one of 15, 30, 60, 120, 240 (ft8gpu_pcm_decimation); M = D / 3.  format = FT8GPU_PCM_S16 or
 *   FT8GPU_PCM_F32, plus FT8GPU_PCM_COMPLEX or not.  Real: pcm [ncaptures][nsamples], x[n] = (a[n], 0).  Complex: I and Q
 *   interleaved, pcm [ncaptures][2 * nsamples], x[n] = (a[2n], a[2n+1]).  S16: a = (float)s * 2^-15 (exact); F32: the caller's
 *   floats as they are.  1 <= nsamples <= FT8GPU_PCM_MAX_SAMPLES_PER_D * D (15 s); x is zero outside 0 <= n < nsamples.  A capture
 *   need not start at any alignment beyond that of its sample type.
 * Channel.  freq_bin in units of 6.25 Hz from the input's 0 Hz (the centre of complex input, the audio axis of real input); the
 *   frame's bins 0 .. 511 are the 1600 Hz above it.  Complex: -256 D <= freq_bin <= 256 D - 256; real: 0 <= freq_bin <= 256 D -
 *   256.  F = freq_bin + 128 is the band's centre; c = floor((F + 16) / 32); q = F - 32 c, in [-16, 15].
 * Stage A, at 3200 D sps.  w1[i] = (cos, -sin)(2 pi i / (16 D)), each the float of the double value, i = 0 .. 16 D - 1
 *   (ft8gpu_pcm_mixer1): 200 Hz per step.  u[n] = x[n] * w1[(n c) mod 16 D] (the mathematical mod).  Complex input:
 *   ur = xr * wr - xi * wi, ui = xr * wi + xi * wr, four products, one subtraction, one addition.  Real input: ur = xr * wr,
 *   ui = xr * wi, two products.
 *   Taps (ft8gpu_pcm_taps_a), in double: t[k] = (sinc((8000 * d) / (3200 D)) * I0(9 * sqrt(1 - (d / (4 M))^2))) / I0(9), d = k -
 *   4 M, k = 0 .. 8 M (sinc and I0 as in the audio stage above); s = the sum of t, k ascending from 0; hA[k] = (float)(t[k] / s).
 *   A Kaiser low-pass (beta 9) with its cutoff at 4000 Hz, 8 M + 1 taps centred on 4 M.
 *   v[m] = sum over k = 0 .. 8 M, ascending, of hA[k] * u[M m + 4 M - k], real and imaginary parts separately, each term a product
 *   and then an add, for 0 <= m < 144000; v is zero outside that range.  9600 sps, output m centred on input sample M m.
 * Stage B, at 9600 sps.  w2[i] = (cos, -sin)(2 pi i / 1536) (ft8gpu_pcm_mixer2); z[m] = v[m] * w2[(m q) mod 1536]: zr = vr * wr -
 *   vi * wi, zi = vr * wi + vi * wr.
 *   Taps (ft8gpu_pcm_taps_b): the same formula with sinc((3200 * d) / 9600) and d / 23, d = k - 23, k = 0 .. 46; hB[47] = 0.
 *   y[p] = sum over k = 0 .. 46, ascending, of hB[k] * z[3 p + 23 - k], for 0 <= p < 48000.
 *   out[p] = y[p] * j^p as swaps and negations: p mod 4 = 0: (yr, yi); 1: (-yi, yr); 2: (-yr, -yi); 3: (yi, -yr), where -a is
 *   0 - a, so that a zero stays +0: a silent capture gives +0 everywhere.  Output p is centred on input sample D p: a record's
 *   dt_s is on the capture's time axis.
 *   The frame is planar, [2][48000].  normalise != 0 then scales the frame by (float)(0.5 / (double)max(1e-24f, peak)), peak the
 *   largest |value| of both planes: the peak normalisation of ft8gpu_rx_decimate.
 * Any float input is defined: infinities, NaNs and subnormals are kept, not flushed.  An output that is a NaN by this rule is a NaN
 * in every implementation (sign and payload unspecified); every other output is the same bytes everywhere.  Every capture starts
 * from zero state.
 * Whole chain, float taps, every D, q = -16, 0, 15, every 3.125 Hz of the input band (tests/test_pcm_cpu.py), with the taps of this header's own I0 series: at most
 * -91.4 dB at or beyond 2400 Hz from the band's centre (the only offsets that alias into the bins the decoder reads; -91.4 dB at
 * D = 15, -92.0 .. -92.1 dB at the other rates), within -0.0070 .. +0.0005 dB up to 800 Hz from it.  With 6 M + 1 taps in stage A
 * the passband would droop to -0.116 dB, hence 8 M + 1. */
#define FT8GPU_PCM_S16           0          /* int16_t samples */
#define FT8GPU_PCM_F32           1          /* float samples */
#define FT8GPU_PCM_COMPLEX       2          /* added to either: I and Q interleaved */
#define FT8GPU_PCM_MAX_SAMPLES_PER_D 48000  /* nsamples <= 48000 D: 15 s */
#define FT8GPU_PCM_MAX_SAMPLES   11520000   /* 15 s at 768 ksps */
#define FT8GPU_PCM_MAX_D         240
#define FT8GPU_PCM_MIX2          1536
#define FT8GPU_PCM_TAPS_B        48
#define FT8GPU_PCM_MAX_CHANNELS  16
/* rate -> D (15, 30, 60, 120 or 240), 0 for a rate the front end does not take */
int  ft8gpu_pcm_decimation(int rate);
/* the tables of the rule (host, plain C): w1 as 16 D float pairs, w2 as 1536 float pairs, hA[0 .. 8 M] (exactly 8 M + 1 floats are
 * written, no padding; returns 8 M + 1, or -1 for an unknown D), hB[0 .. 47].  An unknown D writes nothing. */
void ft8gpu_pcm_mixer1(int D, float *out);
void ft8gpu_pcm_mixer2(float out[2 * FT8GPU_PCM_MIX2]);
int  ft8gpu_pcm_taps_a(int D, float *out);
void ft8gpu_pcm_taps_b(float out[FT8GPU_PCM_TAPS_B]);
/* stage entry: pcm [ncaptures][nsamples] (complex: [2 * nsamples]) of `format`, freq_bin [nchannels] (host memory in both pointer
 * forms) -> iq [ncaptures][nchannels][2][48000].  Host or device pointers by `flags` (device form: pcm aligned to its sample type,
 * iq 16-byte aligned), captures in chunks of max_frames.  Refused before anything is enqueued, the outputs untouched: a NULL
 * context or array, an unknown format or rate, nchannels outside [1, 16], a freq_bin out of range for the format, nsamples
 * outside [1, 48000 D], a misaligned pointer (device form).  The 9600 sps planes between the stages are allocated on the first
 * call (a failed allocation is reported and leaves the context usable) and freed at ft8gpu_destroy. */
int  ft8gpu_pcm_frames(ft8gpu_ctx *ctx, const void *pcm, int format, int rate, int ncaptures, int nsamples,
                       const int32_t *freq_bin, int nchannels, float *iq, int normalise, int flags);
/* The whole path: the frames capture * nchannels + channel, normalised, go through the ft8gpu_decode_messages path, at most
 * max_frames at a time.  Then the channels of a capture are merged as ft8gpu_decode_wide merges them: a record is dropped if its
 * 12 a91 bytes equal those of a record already kept for the capture whose channel lies less than 256 bins away; a kept record
 * gets freq_hz = (cand.freq_offset + freq_bin + (float)cand.freq_sub / 2) * 6.25f and pad[0] = the channel's index; the walk
 * stops at 50 * nchannels records.  msgs [ncaptures][50 * nchannels], n_msgs [ncaptures]; records at and behind n_msgs[c] are
 * left untouched.  Arguments are refused as by ft8gpu_pcm_frames. */
int  ft8gpu_decode_pcm(ft8gpu_ctx *ctx, const void *pcm, int format, int rate, int ncaptures, int nsamples,
                       const int32_t *freq_bin, int nchannels, ft8gpu_message *msgs, int32_t *n_msgs, int flags);
/* Reads a RIFF/WAVE file: format tag 1 at 16 bit or tag 3 (IEEE float) at 32 bit, or tag 0xFFFE (extensible) carrying one of the
 * two; one channel (real) or two (I, Q); 48000, 96000, 192000, 384000 or 768000 Hz.  out gets the samples as the file holds them
 * (little-endian), truncated to cap_bytes and to 15 s; *format, *rate and *nsamples (per channel) describe them.
 * Chunks are skipped and padded as by ft8gpu_read_wav.  Everything else is refused with a line on stderr that names what was
 * found: 0 = ok, -1 = refused (*nsamples = 0, *format = -1, *rate = 0). */
int  ft8gpu_read_wav_pcm(const char *path, void *out, size_t cap_bytes, int *format, int *rate, int32_t *nsamples);

/* ---- tooling: encoder + synthetic frames (pack77 / ft8_encode / CPFSK synth of
 *      decoderSelfTest, rtlsdr_ft8d.c:924-955) --------------------------------------------- */
/* Message text -> 77 bits in 10 bytes (pack77, :927); 0 = ok, -1 = the text fits no message type.  Tokens are separated
 * by blanks.  Tried in this order:
 *   telemetry   one token of 18 hexadecimal digits (the first 0..7)                                       i3.n3 = 0.5
 *   type 1 / 2  FIELD1 CALL2 [GRID4 | R GRID4 | +NN | -NN | R+NN | R-NN | RRR | RR73 | 73]                  i3 = 1 / 2
 *               FIELD1 = CQ | CQ nnn | CQ aaaa | DE | QRZ | call; a call is a standard call sign, optionally with
 *               /R (type 1) or /P (type 2), or <CALL> (sent as a 22-bit hash: receivers without a hash table -- the
 *               reference's ft8_lib era -- print "<...>"); reports -30 .. +99
 *   type 4      <CALL> LONGCALL [RRR | RR73 | 73]  |  LONGCALL <CALL> [...]  |  CQ LONGCALL                    i3 = 4
 *               LONGCALL: up to 11 characters of [0-9A-Z/], sent in full; the bracketed call as a 12-bit hash
 *   free text   up to 13 characters of [ 0-9A-Z+-./?]                                                   i3.n3 = 0.0
 * (ft8_lib's pack77 of the reference's era packs the type 1 forms without suffixes, brackets, "R GRID4" and CQ
 * modifiers, and turns everything else into free text.) */
int  ft8gpu_pack77(const char *msg, uint8_t payload[10]);
/* the strict subset of it: "CALL1 CALL2 [GRID4]" with plain standard calls (CQ / DE / QRZ allowed first), else -1 */
int  ft8gpu_pack77_std(const char *msg, uint8_t payload[10]);
/* payload -> 79 tone numbers (ft8_encode, :934) */
void ft8gpu_encode(const uint8_t payload[10], uint8_t tones[FT8GPU_NN]);

typedef struct {
    uint8_t tones[FT8GPU_NN];
    uint8_t pad;
    float   f0_hz;        /* frequency of tone 0 */
    float   t0_s;         /* start time within the frame */
    float   amplitude;    /* linear amplitude (noise has unit power in 3200 Hz before normalisation) */
} ft8gpu_synth_signal;

/* Synthesises frames directly in HBM: complex AWGN (variance noise_sigma^2 per component) plus
 * nsig_per_frame CPFSK signals per frame (plain FSK as rtlsdr_ft8d.c:946-955), then peak-normalises
 * each frame to 0.5 as the decoder thread does (rtlsdr_ft8d.c:248-263).
 * signals: host array [nframes][nsig_per_frame]; iq_dev: device pointer [nframes][2][48000]. */
int ft8gpu_synth_frames(ft8gpu_ctx *ctx, const ft8gpu_synth_signal *signals, int nframes,
                        int nsig_per_frame, float noise_sigma, uint64_t seed, float *iq_dev);
/* The same for a shard of a larger job: frame k of this call is global frame first_frame + k, and the
 * noise of a frame depends on (seed, global frame index) only -- any partition of the job over ranks,
 * GPUs or calls synthesises the same frames.  ft8gpu_synth_frames == first_frame 0. */
int ft8gpu_synth_frames_at(ft8gpu_ctx *ctx, const ft8gpu_synth_signal *signals, int nframes,
                           int nsig_per_frame, float noise_sigma, uint64_t seed, uint64_t first_frame,
                           float *iq_dev);

/* ---- GFSK synthesis: the signal as it is on the air, as I/Q frames and as 12 kHz audio -------------------------------------------
 * (DESIGN.md "GFSK synthesis"; not in the reference, whose self-test frame is plain CPFSK.)  An FT8 transmitter sends GFSK: the
 * frequency pulse of a symbol is a rectangle of one symbol smoothed by a Gaussian with BT = 2, cut to three symbols, and the
 * amplitude is ramped over the first and the last eighth of a symbol.  This is WSJT-X's sampled pulse (gfsk_pulse, gen_ft8wave)
 * and its running sum.  The rule is exact: the phase is integer arithmetic, the rest float32 with one IEEE operation per step,
 * nothing fused, sums sequential from +0.
 *
 * Modes.  FT8GPU_GFSK_IQ: rate 3200, sps = 512 samples per symbol, output planar [2][48000] = (cos, sin).
 *         FT8GPU_GFSK_AUDIO: rate 12000, sps = 1920, output real = cos, nsamples in [1, 180000].
 * Pulse table Q_sps[0 .. 3 sps], uint32 in units of 2^-32 turn (ft8gpu_gfsk_pulse), in double:
 *   c = M_PI * sqrt(2.0 / log(2.0));  t_i = ((double)i - 1.5 * (double)sps) / (double)sps;
 *   p_i = 0.5 * (erf((2.0 * c) * (t_i + 0.5)) - erf((2.0 * c) * (t_i - 0.5))),  i = 0 .. 3 sps - 1;
 *   Q[k] = llrint((4294967296.0 * (p_0 + ... + p_(k-1), sequential from 0.0)) / (double)sps) mod 2^32.
 *   The pulses of neighbouring symbols sum to one, so Q[3 sps] is 0 mod 2^32 (the unreduced value is 2^32 for both sps).  Two
 *   libms may round erf differently: an entry may differ by one unit between two hosts.  The device uses the table of its host.
 * Twiddles (ft8gpu_gfsk_twiddles).  gc[i] = (cos, sin)(2.0 * M_PI * (double)i / 4096.0), gf[i] = (cos, sin)(2.0 * M_PI * (double)i /
 *   16777216.0), i = 0 .. 4095, each entry the float of the double value.
 * Ramp (ft8gpu_gfsk_ramp).  nr = sps / 8;  r[k] = (float)(0.5 * (1.0 - cos(M_PI * (double)k / (double)nr))), k = 0 .. nr - 1;
 *   env(n') = r[n'] for n' < nr;  r[79 sps - 1 - n'] for n' >= 79 sps - nr;  1 otherwise.  This is the mirrored form: WSJT-X's
 *   trailing ramp, 0.5 (1 + cos(pi k / nr)) from sample 79 sps - nr on, is this one a sample later.
 * Per signal (an ft8gpu_synth_signal).  start = lrintf(t0_s * (float)rate);  step = (uint32_t)llrint((double)f0_hz * 4294967296.0 /
 *   (double)rate), left to right, on the host; a negative f0_hz wraps (meaningful in the I/Q mode).  Extended tones: e[0] =
 *   tones[0], e[j] = tones[j - 1] for j = 1 .. 79, e[80] = tones[78].  For the local sample n' in [0, 79 sps), m = n' div sps,
 *   k = n' mod sps, in wrapping uint32 arithmetic
 *     phi = step * n' + e[m] * Q[k + 2 sps] + e[m + 1] * Q[k + sps] + e[m + 2] * Q[k]
 *   (the modulation index is 1, so symbols further back contribute whole turns and drop out);  ic = phi >> 20, jf = (phi >> 8) & 4095;
 *     co = gc[ic].c * gf[jf].c - gc[ic].s * gf[jf].s;   si = gc[ic].s * gf[jf].c + gc[ic].c * gf[jf].s
 *   (two products, then one subtraction or addition);  a = amplitude * env(n');  the contribution (a * co, a * si) goes to output
 *   sample start + n' where that lies inside the clip: a signal may begin before sample 0 and end behind the clip's end, and is
 *   cut there, not shifted.
 * Output sample.  The contributions of the clip's signals are summed in signal order from +0.  If noise_sigma > 0 the noise is
 *   added last.  If peak > 0: m = the largest |x| of the clip (both planes in the I/Q mode; a NaN is skipped as by fmaxf),
 *   m = max(m, 1e-24f), s = peak / m, x = x * s; with peak 0.5 this is the decoder thread's convention (rtlsdr_ft8d.c:248-263).
 *   FT8GPU_AUDIO_S16: rintf(x * 32768.0f), clamped to [-32768, 32767]; a NaN gives 0.
 * Noise.  The counter generator of ft8gpu_synth_frames, keyed by (seed, first + clip index, sample index), with its Box-Muller:
 *   one draw gives I and Q; the audio mode takes the cosine branch.  Noise is outside the exact contract (it need not match a
 *   CPU), but a clip's noise is the same bytes on the device for any chunking and any partition of a job by first_*.  With
 *   noise_sigma == 0 the generator is not evaluated and the output is the rule's bytes.
 * Refused before anything is enqueued (and before the context is looked at): f0_hz, t0_s or amplitude not finite; |f0_hz| >=
 *   rate, or f0_hz < 0 in the audio mode; |t0_s| > 60; a tone above 7; more than 64 signals per clip (0 is allowed); nsamples
 *   outside [1, 180000]; an unknown format; peak < 0 or noise_sigma < 0, or either not finite. */
#define FT8GPU_GFSK_IQ         0
#define FT8GPU_GFSK_AUDIO      1
#define FT8GPU_GFSK_SPS_IQ     512
#define FT8GPU_GFSK_SPS_AUDIO  1920
#define FT8GPU_GFSK_TWIDDLES   4096
#define FT8GPU_GFSK_MAX_SIGNALS 64
#define FT8GPU_GFSK_TILE       8192    /* output samples a workgroup of the kernel owns (not part of the rule; the tests aim at its seams) */
/* the tables of the rule (host, plain C).  sps is 512 or 1920: out[3 sps + 1] resp. out[sps / 8]; 0 = ok, -1 = another sps or NULL */
int ft8gpu_gfsk_pulse(int sps, uint32_t *out);
int ft8gpu_gfsk_ramp(int sps, float *out);
/* coarse = gc, fine = gf, each 4096 (cos, sin) pairs; a NULL table is left out */
void ft8gpu_gfsk_twiddles(float *coarse, float *fine);
/* signals: host array [nframes][nsig_per_frame] in both pointer forms; iq_out [nframes][2][48000], host or device memory by
 * `flags`, frames in chunks of max_frames.  Frame k of the call is global frame first_frame + k (its noise depends on seed and
 * the global index only).  Tables and buffers are allocated on the first GFSK call and freed at ft8gpu_destroy. */
int ft8gpu_synth_gfsk_frames(ft8gpu_ctx *ctx, const ft8gpu_synth_signal *signals, int nframes, int nsig_per_frame,
                             float noise_sigma, uint64_t seed, uint64_t first_frame, float peak, float *iq_out, int flags);
/* the same as 12 kHz audio: pcm_out [nclips][nsamples] of `format` (FT8GPU_AUDIO_S16 or FT8GPU_AUDIO_F32) */
int ft8gpu_synth_gfsk_audio(ft8gpu_ctx *ctx, const ft8gpu_synth_signal *signals, int nclips, int nsig_per_clip, int nsamples,
                            float noise_sigma, uint64_t seed, uint64_t first_clip, float peak, int format, void *pcm_out, int flags);
/* Writes pcm[0 .. nsamples) as a RIFF/WAVE file of PCM, mono, 16 bit, 12000 Hz with a 44-byte header, which ft8gpu_read_wav
 * reads back to the same samples.  nsamples >= 0.  0 = ok, -1 = NULL argument, negative count or the file could not be written
 * (a line on stderr says why). */
int ft8gpu_write_wav(const char *path, const int16_t *pcm, int32_t nsamples);

/* ---- Fading channel: the GFSK signal over one or two Rayleigh-fading HF paths ----------------------------------------------------
 * (DESIGN.md "Fading channel"; tests/ft8_spec_channel.py restates the rule and the device output at noise_sigma == 0 equals that
 * byte for byte.)  An ft8gpu_channel per signal, parallel to the ft8gpu_synth_signal array, gives every path of the signal a
 * complex gain that varies in time with a Gaussian Doppler spectrum, and an optional second path a delay.  The rule is exact in
 * the sense of "GFSK synthesis": integer phases, float32, one IEEE operation per step, nothing fused, sums sequential from +0.
 *
 * Gain process.  A (signal, path) has M = 16 sinusoids, evaluated on a grid of 100 points per second and interpolated linearly
 *   between them.  The grid step is S = 32 samples in the I/Q mode and S = 120 in the audio mode, so both modes have the same
 *   grid in time; a signal of 79 sps samples spans 1264 steps, grid points 0 .. 1264.
 * Taps (ft8gpu_channel_taps, host, plain C, no libm but the exact llrint).  q_m = FT8GPU_CHANNEL_QUANTILES[m], the standard normal
 *   quantile at (m + 0.5) / 16;  f_m = ((double)spread_hz / 2.0) * q_m  (spread_hz is two sigma of the Doppler spectrum);
 *     gstep_m = (uint32_t)(int64_t)llrint(f_m / 100.0 * 4294967296.0)      -- turns per grid step in units of 2^-32; negative wraps
 *     theta_m = (uint32_t)(mix(mix(seed ^ 0x4641444531) ^ mix((clip << 12) + (signal << 5) + (path << 4) + m)) >> 32)
 *   in uint64 arithmetic; clip is the global clip index (first_* + the clip's index in the call), signal the signal's index in
 *   its clip, path 0 or 1, and mix is splitmix64's step:
 *     mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9; x = (x ^ (x >> 27)) * 0x94D049BB133111EB; x ^ (x >> 31).
 * Path amplitudes (host).  g2 = path2_gain;  r = sqrtf(1.0f + g2 * g2);  w_0 = 1.0f / r;  w_1 = g2 / r: the mean power of a faded
 *   signal is that of the unfaded one.  With g2 == 0 there is no second path (it is skipped, not added as zeros).
 * Grid value of path p at grid point j, with gc and gf of "GFSK synthesis":  ph = theta_m + gstep_m * j in wrapping uint32
 *   arithmetic, ic = ph >> 20, jf = (ph >> 8) & 4095,
 *     co_m = gc[ic].c * gf[jf].c - gc[ic].s * gf[jf].s;   si_m = gc[ic].s * gf[jf].c + gc[ic].c * gf[jf].s     (as the carrier's)
 *     G[j] = w_p * (0.25f * (co_0 + co_1 + ... + co_15)),  the same with si:  each sum sequential from +0 in the order of m, then
 *   the product by 0.25f, then the product by w_p.
 * Per sample.  For the local sample n' in [0, 79 sps) of a path:  j = n' div S, k = n' mod S, t = (float)k / (float)S,
 *     Gr = G[j].c + (G[j + 1].c - G[j].c) * t,  Gi the same with .s    (a subtraction, a product, an addition)
 *   xr = a * co, xi = a * si are the unfaded rule's contribution at n' (a = amplitude * env(n')).  The path contributes
 *     re = xr * Gr - xi * Gi;   im = xr * Gi + xi * Gr            (two products, then one subtraction or addition)
 *   to output sample start + n' (path 0) or start + d + n' (path 1),  d = lrintf(delay_ms * (float)rate / 1000.0f), left to
 *   right, where that lies inside the clip: a path is cut at the clip's ends as a signal is.  Path 1 is the same waveform with
 *   its own taps.  The audio mode keeps re.
 * Output sample.  Signals are added in signal order from +0, within a signal path 0 before path 1.  A signal whose channel has
 *   mode == 0 is added by the unfaded rule, byte for byte, and its other fields are not looked at.  Noise, peak normalisation and
 *   the int16 form follow as in "GFSK synthesis"; the noise stays outside the exact contract.  spread_hz == 0 is no special
 *   case: every gstep is 0 and the gain is one constant Rayleigh draw per path (block fading).
 * Refused before anything is enqueued, for a channel with mode == 1: a field that is not finite, spread_hz outside [0, 20],
 *   delay_ms outside [0, 10], path2_gain outside [0, 4]; for any channel: mode > 1. */
typedef struct {
    float    spread_hz;   /* two-sided Doppler spread (2 sigma of a Gaussian Doppler spectrum) of each path, [0, 20] */
    float    delay_ms;    /* delay of the second path, [0, 10] */
    float    path2_gain;  /* amplitude of path 2 relative to path 1, [0, 4]; 0 = one path */
    uint32_t mode;        /* 0 = none: the signal is synthesised by the unfaded rule, byte for byte; 1 = faded */
} ft8gpu_channel;
#ifndef __cplusplus
_Static_assert(sizeof(ft8gpu_channel) == 16 && offsetof(ft8gpu_channel, delay_ms) == 4 && offsetof(ft8gpu_channel, path2_gain) == 8 &&
               offsetof(ft8gpu_channel, mode) == 12, "ft8gpu_channel layout");
#else
static_assert(sizeof(ft8gpu_channel) == 16 && offsetof(ft8gpu_channel, delay_ms) == 4 && offsetof(ft8gpu_channel, path2_gain) == 8 &&
              offsetof(ft8gpu_channel, mode) == 12, "ft8gpu_channel layout");
#endif
#define FT8GPU_CHANNEL_NONE    0u
#define FT8GPU_CHANNEL_FADED   1u
#define FT8GPU_CHANNEL_TAPS    16      /* M */
#define FT8GPU_CHANNEL_STEP_IQ     32  /* S: samples per grid step */
#define FT8GPU_CHANNEL_STEP_AUDIO  120
#define FT8GPU_CHANNEL_GRID    1265    /* grid points of one path: 79 sps / S + 1 */
/* the standard normal quantiles at (m + 0.5) / 16, m = 0 .. 15, to 15 decimals */
#define FT8GPU_CHANNEL_QUANTILES { \
    -1.862731867421651, -1.318010897303537, -1.009990169249582, -0.776421761147928, -0.579132162255556, -0.402250065321725, \
    -0.237202109328788, -0.078412412733112,  0.078412412733112,  0.237202109328788,  0.402250065321725,  0.579132162255556, \
     0.776421761147928,  1.009990169249582,  1.318010897303537,  1.862731867421651 }
/* initialisers for the usual HF conditions (spread / delay, two equal paths); conveniences, not part of the rule */
#define FT8GPU_CHANNEL_QUIET     { 0.1f, 0.5f, 1.0f, FT8GPU_CHANNEL_FADED }
#define FT8GPU_CHANNEL_MODERATE  { 0.5f, 1.0f, 1.0f, FT8GPU_CHANNEL_FADED }
#define FT8GPU_CHANNEL_DISTURBED { 1.0f, 2.0f, 1.0f, FT8GPU_CHANNEL_FADED }
#define FT8GPU_CHANNEL_FLUTTER   { 10.0f, 0.5f, 1.0f, FT8GPU_CHANNEL_FADED }
/* gstep[16], theta[16] of one (signal, path); either may be NULL.  0 = ok, -1 = spread_hz outside [0, 20] or not finite, or
 * path outside {0, 1} */
int ft8gpu_channel_taps(uint64_t seed, uint64_t clip, uint32_t signal, uint32_t path, float spread_hz, uint32_t *gstep, uint32_t *theta);
/* 0 if the entries below take the channel; else which field they refuse: 1 spread_hz, 2 delay_ms, 3 path2_gain, 4 mode */
int ft8gpu_channel_check(const ft8gpu_channel *ch);
/* The rule on the host, plain C, for one clip: signals [nsig] and channels [nsig] (NULL: all unfaded) -> out, the sum before
 * noise and normalisation, [2][48000] floats (FT8GPU_GFSK_IQ; nsamples is ignored) or [nsamples] (FT8GPU_GFSK_AUDIO).  `clip`
 * is the global clip index.  0 = ok, -1 = an argument the entries below refuse, or out of memory for the tables. */
int ft8gpu_channel_clip(int mode, const ft8gpu_synth_signal *signals, const ft8gpu_channel *channels, int nsig, int nsamples,
                        uint64_t seed, uint64_t clip, float *out);
/* ft8gpu_synth_gfsk_frames / _audio with channels, a host array [n][nsig] parallel to signals in both pointer forms.  channels ==
 * NULL is the unfaded entry; a call whose channels all have mode 0 gives its bytes, noise included.  The taps are keyed by seed
 * (the noise's) and the global clip index, so any chunking and any partition of a job by first_* gives the same clips.  The grid
 * values take 2 * 1265 * 8 bytes of device memory per signal of a chunk, allocated when first needed and freed at ft8gpu_destroy. */
int ft8gpu_synth_gfsk_frames_faded(ft8gpu_ctx *ctx, const ft8gpu_synth_signal *signals, const ft8gpu_channel *channels, int nframes,
                                   int nsig_per_frame, float noise_sigma, uint64_t seed, uint64_t first_frame, float peak,
                                   float *iq_out, int flags);
int ft8gpu_synth_gfsk_audio_faded(ft8gpu_ctx *ctx, const ft8gpu_synth_signal *signals, const ft8gpu_channel *channels, int nclips,
                                  int nsig_per_clip, int nsamples, float noise_sigma, uint64_t seed, uint64_t first_clip, float peak,
                                  int format, void *pcm_out, int flags);

/* ---- RX front end: rtlsdr_callback(), rtlsdr_ft8d.c:76-202 ------------
 * Whole raw RTL-SDR captures (unsigned 8-bit I,Q interleaved at 2.4 Msps) -> the 15 s / ~3200 sps
 * float frames the decoder consumes: fs/4 mixer, CIC (N = 2, comb delay 2, effective ratio 751),
 * 57-tap compensation FIR, scaling; every capture starts from the reset filter state (ft8gpu_rx_stream
 * below carries the state from one buffer into the next, as the reference's daemon does).  Samples past
 * npairs/751 are zero as after the decoder thread's tail zeroing (:243-246); normalise != 0 applies
 * its peak normalisation to 0.5 (:248-263), after which `iq` can go straight into ft8gpu_decode_batch.
 * raw: [ncaptures][2*npairs] bytes, npairs a multiple of 8, 16-byte aligned; iq: [ncaptures][2][48000]. */
int ft8gpu_rx_decimate(ft8gpu_ctx *ctx, const uint8_t *raw, int ncaptures, size_t npairs,
                       float *iq, int normalise, int flags);

/* The same front end on a continuous stream.  rtlsdr_callback() keeps its filter state in function statics and the
 * daemon never resets them: every 15 s buffer after the first starts from what the previous one left (36 000 000 pairs
 * mod 751 = 64, so the decimation grid of the second buffer is shifted, and every sample of it differs from a run
 * from reset).  ft8gpu_rx_state holds those statics, field for field: the two integrators per channel, the last comb
 * outputs, the comb delays, decimationIndex and the 56-float FIR histories (516 bytes, no padding). */
typedef struct {
    int32_t  Ix1, Ix2, Qx1, Qx2;                 /* integrators (wrapping 32-bit) */
    int32_t  Iy1, It1y, It1z, Qy1, Qt1y, Qt1z;   /* first comb: last output, delays */
    int32_t  Iy2, It2y, It2z, Qy2, Qt2y, Qt2z;   /* second comb */
    uint32_t decimationIndex;                    /* pairs consumed since the last output, 0..750 */
    float    firI[56], firQ[56];                 /* the last 56 comb outputs, oldest first */
} ft8gpu_rx_state;

/* all zero, as at program start */
void ft8gpu_rx_state_reset(ft8gpu_rx_state *st);

/* raw: [nstreams][nslots][2*npairs] bytes: nstreams independent receivers, each with nslots consecutive buffers of
 * npairs pairs (a positive multiple of 8; raw 16-byte aligned).  nstreams * nslots <= max_frames.  Buffers of different
 * length are served by successive calls with nslots = 1.
 * state: [nstreams], read at entry and written at exit: slot s + 1 of a stream continues from the state slot s left,
 * and the next call continues from `state`.  After the call state[k] equals, byte for byte, the reference's statics
 * after rtlsdr_callback() has consumed the same bytes from the same entry state.  Every byte is consumed (unlike
 * ft8gpu_rx_decimate, which stops after 48000 blocks).  An entry decimationIndex above 750 is refused.
 * iq: [nstreams][nslots][2][48000]: per slot the outputs the reference stores for it -- the decimation events inside
 * the slot's bytes, the first 48000 of them (:195-200) -- zeros behind them (:243-246), and with normalise != 0 the
 * per-slot peak normalisation (:248-263).  n_out: [nstreams][nslots] stored counts (iqIndex), or NULL.
 * flags: FT8GPU_HOST_PTRS / FT8GPU_DEVICE_PTRS for every array argument, state and n_out included.  The device form
 * reads the entry decimationIndex values back (one stream synchronisation) before it enqueues anything.
 * From a reset state and with nslots = 1 the frames are byte-identical to ft8gpu_rx_decimate's. */
int ft8gpu_rx_stream(ft8gpu_ctx *ctx, const uint8_t *raw, int nstreams, int nslots, size_t npairs,
                     ft8gpu_rx_state *state, float *iq, uint32_t *n_out, int normalise, int flags);

/* ---- spot reporting wire formats ------------------------------------
 * The bytes postSpots() (rtlsdr_ft8d.c:365-590) assembles for report.pskreporter.info:4739 (IPFIX:
 * 16-byte header, receiver and sender template sets, receiver record, one sender record per slot
 * of decodes[0..n_results)), built for a whole batch of spot lists at once; nothing is sent.
 * Reference behaviour kept: every slot below n_results is emitted, also the untouched slots of
 * non-CQ messages (:494-533); a record is started only while the sender block is <= 1200 bytes
 * (:497); SNR byte = (int8)snr - 20 (:511); both data blocks are zero-padded to 4 bytes.
 * Fenced: call / loc are read up to 12 / 6 characters (the reference's strlen has no bound). */
#define FT8GPU_DATAGRAM_STRIDE 1408        /* >= the largest datagram (168 + 1236 bytes) */
typedef struct {
    char     rcall[13];        /* dec_options.rcall, rtlsdr_ft8d.h:132 */
    char     rloc[7];          /* dec_options.rloc,  rtlsdr_ft8d.h:133 */
    char     app_version[32];  /* pskreporter_app_version, rtlsdr_ft8d.c:72 */
    uint32_t dial_freq;        /* dec_options.freq, added to every spot's audio offset (:507) */
    uint32_t unixtime;         /* header export time and spot time (:445, :531) unless unixtimes != NULL */
    uint32_t sequence;         /* 1 in the reference (:425) */
    uint32_t random_id;        /* :430-435 */
} ft8gpu_report_info;
/* decodes: [nframes][50], n_results: [nframes], unixtimes: [nframes] or NULL,
 * datagrams: [nframes][FT8GPU_DATAGRAM_STRIDE] (bytes past the length are zero), lengths: [nframes] */
int ft8gpu_pskreporter_datagrams(ft8gpu_ctx *ctx, const struct decoder_results *decodes,
                                 const int32_t *n_results, int nframes, const ft8gpu_report_info *info,
                                 const uint32_t *unixtimes, uint8_t *datagrams, int32_t *lengths, int flags);
/* the stdout table of printSpots() (:643-663) for one frame's spot list, into `out` (NUL-terminated,
 * truncated to cap); returns the untruncated length.  Host-side text formatting, no GPU involved. */
int ft8gpu_format_spots(const struct decoder_results *decodes, int32_t n_results, uint32_t dial_freq,
                        int year, int month, int mday, int hour, int minute, char *out, size_t cap);

/* device memory helpers so that a plain C caller needs no HIP headers; they act on the context's GPU
 * (whatever device is current in the calling thread) and order after the context's enqueued work */
void *ft8gpu_dev_alloc(ft8gpu_ctx *ctx, size_t bytes);
void  ft8gpu_dev_free(ft8gpu_ctx *ctx, void *p);
int   ft8gpu_memcpy_h2d(ft8gpu_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int   ft8gpu_memcpy_d2h(ft8gpu_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* Page-locked host memory (hipHostMalloc / hipHostFree) for the buffers handed to the FT8GPU_HOST_PTRS entries:
 * ft8gpu_decode_batch uploads in 512-frame chunks with asynchronous copies under the kernels of the previous chunk,
 * and ft8gpu_decode_batch_multi does the same on every GPU at once -- which only overlaps (and only reaches the
 * link rate, about 50 GB/s per GPU) from pinned memory; from malloc'ed memory every copy is staged and serialises with
 * the kernels.  The reference's own buffers are plain static arrays (rtlsdr_ft8d.c:274-278): a daemon decoding one frame
 * per 15 s does not need this, a replay that feeds thousands of frames does.  NULL + ft8gpu_last_error() on failure. */
void *ft8gpu_host_alloc(size_t bytes);
void  ft8gpu_host_free(void *p);

/* ---- drop-in symbols of the reference (rtlsdr_ft8d.h:155-156, :164) --------------------------
 * Link rtlsdr_ft8d.c against libft8gpu.so instead of its own ft8_subsystem/initFFTW/freeFFTW
 * (INTEGRATION.md).  They drive a process-global single-frame context on GPU 0
 * (env FT8GPU_DEVICE overrides). */
void initFFTW(void);
void freeFFTW(void);
void ft8_subsystem(float *iSamples, float *qSamples, uint32_t samples_len,
                   struct decoder_results *decodes, int32_t *n_results);

/* .iq / .c2 readers and writer with the reference's conventions (rtlsdr_ft8d.c:744-856):
 * interleaved float32 I,Q on disk, Q negated, peak-normalised to 0.5 on load. */
int32_t ft8gpu_read_raw_iq(float *iSamples, float *qSamples, const char *filename);
int32_t ft8gpu_read_c2(float *iSamples, float *qSamples, const char *filename, double *dialfreq);
int32_t ft8gpu_write_raw_iq(const float *iSamples, const float *qSamples, const char *filename);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* FT8GPU_H */
