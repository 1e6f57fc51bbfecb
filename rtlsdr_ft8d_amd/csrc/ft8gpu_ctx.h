// ft8gpu_ctx.h -- the context object and the helpers every host-side translation unit of the C ABI shares: api_context.hip,
// api_mem.hip, api_pipeline.hip, api_multi.hip, api_stages.hip, api_messages.hip, api_multipass.hip, api_osd.hip, api_ap.hip,
// api_glue.hip, api_rx_stream.hip, api_callhash.hip, api_match.hip, api_combine.hip, api_refine.hip, api_subtract.hip,
// api_demod.hip, api_audio.hip, api_gfsk.hip, api_wide.hip, api_pcm.hip.  Not installed.
#pragma once
#include "ctx_mem.h"
#include "ft8gpu_internal.h"

#include <functional>
#include <limits.h>
#include <mutex>
#include <stddef.h>

// ft8gpu_last_error(): thread-local text, written by ft8_fail() only (api_context.hip; declared in ctx_mem.h)
char *ft8_err_buffer();                       // the calling thread's buffer (kErrBytes), for hand-overs between threads
constexpr size_t kErrBytes = 512;

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return ft8_fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

const MemBackend *hip_mem();                  // api_mem.hip

struct ft8gpu_ctx {
    CtxMem mem{ hip_mem() };                 // owns every d_* / h_* buffer below: allocated through it, freed by its release_all()
    int device = 0;
    int num_cus = 256;
    int max_frames = 0;
    int cap_candidates = 0;
    ft8gpu_params params{ FT8GPU_K_MIN_SCORE, FT8GPU_K_MAX_CANDIDATES, FT8GPU_K_LDPC_ITERS };
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool timing = false;
    static constexpr int kTimingSlots = 32, kEvPerSlot = 16, kSideEv0 = 10;
    hipEvent_t ev[kTimingSlots][kEvPerSlot]{};   // ring of per-run stage events (no host sync while timing):
                                                 // 0..9 on the main stream, 10..15 on the side stream
    long runs = 0;                         // pipeline runs recorded since timing was enabled
    int slot_form[kTimingSlots]{};         // which form of the pipeline a slot recorded: 0 one launch per stage, 1 two parts
    hipStream_t side = nullptr;            // carries the serial kernels (heap, spots) of one half-batch
                                           // while the main stream works on the other half
    hipStream_t side2 = nullptr;           // heap replay of part B (beside the one of part A on `side`)
    hipEvent_t dep[4]{};                   // cross-stream dependencies (no timing)
    bool overlap_ok = false;               // main, side and side2 were SEEN to run kernels concurrently (probe_streams)
    int *d_probe = nullptr;                // two ints for that probe
    char overlap_why[160] = "";            // why the overlapped pipeline is off (empty when it is on)
    std::mutex mu;                         // every entry point holds it: concurrent callers of one context serialise
    unsigned debug_flags = 0;              // FT8GPU_DBG_* (test hooks, per context)
    hipStream_t copy = nullptr;            // host-buffer calls: uploads chunk k+1 while chunk k is decoded
    static constexpr int kCopyEvents = 4;
    hipEvent_t copied[kCopyEvents]{};

    Ft8Tables *d_tab = nullptr;
    float *d_iq = nullptr;                 // staging for host-pointer calls
    uint8_t *d_mag = nullptr;
    uint32_t *d_lists = nullptr;
    int32_t *d_list_counts = nullptr;
    ft8gpu_candidate *d_cands = nullptr;
    int32_t *d_counts = nullptr;
    ft8gpu_decode_status *d_status = nullptr;
    struct decoder_results *d_decodes = nullptr;
    int32_t *d_nres = nullptr;
    int16_t *d_scores = nullptr;           // lazily allocated (diagnostic)
    uint8_t *d_base = nullptr;             // messages path, lazily allocated on its first call: noise baseline [max_frames][512]
    MsgTables *d_msgtab = nullptr;         //   its constant tables
    ft8gpu_message *d_msgs = nullptr;      //   host-pointer staging of the records [max_frames][50]
    uint8_t *d_mag2 = nullptr;             // multi-pass, lazily allocated: the compact waterfall of a later pass [max_frames][94208]
    int32_t *d_map = nullptr;              //   its slot -> frame map [max_frames], the counts before the pass [max_frames],
    int32_t *d_nprev = nullptr;            //   the number of active frames (1) and its host copy (pinned)
    int32_t *d_nactive = nullptr;
    int32_t *h_nactive = nullptr;
    ft8gpu_candidate *d_cands2 = nullptr;  //   the pass's candidates / counts / statuses [max_frames][cap2]
    int32_t *d_counts2 = nullptr;
    ft8gpu_decode_status *d_status2 = nullptr;
    int cap2 = 0;
    int32_t *d_nbs = nullptr;              //   staging of n_by_pass / n_by_stage, whatever its width [max_frames][FT8GPU_MAX_PASSES][3]
    bool osd_tables = false;               // OSD, lazily on its first call: the constant tables are uploaded,
    ft8gpu_osd_info *d_osd_info = nullptr; //   the info records [max_frames][osd_cap] and the host form's staging of status_out,
    ft8gpu_decode_status *d_osd_out = nullptr;
    int osd_cap = 0;
    int32_t *d_nosd = nullptr;             //   the counts before the OSD append [max_frames]
    bool ap_tables = false;                // AP, lazily on its first call: the constant tables are uploaded,
    ft8gpu_ap_info *d_ap_info = nullptr;   //   the info records [max_frames][ap_cap] and the host form's staging of status_out,
    ft8gpu_decode_status *d_ap_out = nullptr;
    int ap_cap = 0;
    int32_t *d_nap = nullptr;              //   the counts before the AP append [max_frames]
    bool combine_tables = false;           // soft-bit memory: the constant tables are uploaded (on its first call)
    bool demod_tables = false;             // demodulation from the I/Q samples: likewise
    bool hint_tables = false;              // call hints: likewise
    bool apsoft_tables = false;            // AP on the demodulated soft bits: likewise, and lazily on the first call that needs it
    float *d_soft = nullptr;               //   a chunk's soft-bit array [max_frames][max_candidates][3][176] (grown as needed)
    size_t soft_cap = 0;
    struct SubTables *d_subtab = nullptr;  // subtraction in the I/Q samples, lazily on its first call: the constant tables,
    uint32_t *d_sub_scratch = nullptr;     //   what the estimate kernel leaves for the apply kernel [sub_frames][50][2560],
    int sub_frames = 0;
    float *d_sub_x = nullptr;              //   the frames being subtracted from [max_frames][2][48000] (staging of iq_out / residual),
    ft8gpu_refined *d_sub_ref = nullptr;   //   the refined records [max_frames][50], the info records of the host form,
    ft8gpu_subtract_info *d_sub_info = nullptr;
    int32_t *d_sub_nref = nullptr;         //   and the counts a pass refines and subtracts [max_frames]
    struct SubGfskTables *d_subgfsktab = nullptr;  // the GFSK reference's pulse table and ramp, on the first call with that shape
    struct AudioTables *d_audiotab = nullptr;  // audio front end, lazily on its first call: the constant tables,
    void *d_audio_pcm = nullptr;           //   host-pointer staging of the clips [max_frames][180000] floats,
    float *d_audio_iq = nullptr;           //   the frame buffer of the whole path and of the host form [max_frames][2][48000],
    ft8gpu_message *d_audio_bmsgs = nullptr;   // the bands' records [max_frames][4][50] and counts [max_frames][4],
    int32_t *d_audio_bn = nullptr;
    ft8gpu_message *d_audio_msgs = nullptr;    // and host-pointer staging of the merged records [max_frames][200]
    struct WideTables *d_widetab = nullptr;    // wideband RX, lazily on its first call: the constant tables,
    void *d_wide_planes = nullptr;         //   the 19 200 sps planes between its stages (a run of captures times the channels),
    void *d_wide_raw = nullptr;            //   host-pointer staging of a chunk's captures,
    float *d_wide_iq = nullptr;            //   the frame buffer of the whole path and of the host form [max_frames][2][48000],
    ft8gpu_message *d_wide_cmsgs = nullptr;    // the channels' records [captures][channels][50] and counts of a chunk,
    int32_t *d_wide_cn = nullptr;
    ft8gpu_message *d_wide_msgs = nullptr;     // and host-pointer staging of the merged records
    size_t wide_planes_cap = 0, wide_raw_cap = 0, wide_cmsgs_cap = 0, wide_cn_cap = 0, wide_msgs_cap = 0;
    struct GfskTables *d_gfsktab = nullptr;    // GFSK synthesiser, lazily on its first call: the constant tables,
    struct GfskHeader *d_gfsk_hdr = nullptr;   //   the signal headers of a call (grown as needed),
    size_t gfsk_hdr_cap = 0;
    struct GfskChannel *d_gfsk_ch = nullptr;   //   with channels: the signals' channel headers of a call and the grid values
    float2 *d_gfsk_grid = nullptr;             //   [chunk][nsig][2][1265] of a chunk's paths (both grown as needed),
    size_t gfsk_ch_cap = 0, gfsk_grid_cap = 0;
    float *d_gfsk_x = nullptr;             //   the floats before normalisation where the output is int16 [max_frames][180000],
    void *d_gfsk_out = nullptr;            //   host-pointer staging of the output [max_frames][180000] floats (I/Q: [2][48000]),
    float *d_gfsk_max = nullptr;           //   and the tiles' maxima [max_frames][22]
    ft8gpu_synth_signal *d_sigs = nullptr;
    size_t sigs_cap = 0;
    void *d_scratch[4]{};                  // four growable scratch blocks (ensure_scratch) for whichever entry holds the mutex:
    size_t scratch_cap[4]{};               //   the RX front end, call hash, match, combine, demod and refine say in place what they keep where
    uint8_t *d_rep = nullptr;              // host-pointer staging of the report stage
    int32_t *d_rep_len = nullptr;
    uint32_t *d_rep_time = nullptr;
    size_t rep_cap = 0, rep_len_cap = 0, rep_time_cap = 0;
    struct PcmTables *d_pcmtab = nullptr;  // PCM front end, lazily on its first call: the constant tables of every rate,
    void *d_pcm_planes = nullptr;          //   the 9600 sps planes between its stages (a run of captures times the channels),
    void *d_pcm_raw = nullptr;             //   host-pointer staging of a chunk's captures,
    float *d_pcm_iq = nullptr;             //   the frame buffer of the whole path and of the host form [max_frames][2][48000],
    ft8gpu_message *d_pcm_cmsgs = nullptr; //   the channels' records [captures][channels][50] and counts of a chunk,
    int32_t *d_pcm_cn = nullptr;
    ft8gpu_message *d_pcm_msgs = nullptr;  //   and host-pointer staging of the merged records
    size_t pcm_planes_cap = 0, pcm_raw_cap = 0, pcm_cmsgs_cap = 0, pcm_cn_cap = 0, pcm_msgs_cap = 0;
};

// Every ABI entry that touches a context holds its mutex (two host threads on one context serialise instead
// of racing on the staging buffers and the timing ring) and runs with the context's GPU current, restoring
// the caller's current device on the way out.
struct Entry {
    std::unique_lock<std::mutex> lock;
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit Entry(ft8gpu_ctx *c) : lock(c->mu) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != c->device) err = hipSetDevice(c->device); else prev = -1;
    }
    ~Entry() { if (prev >= 0) (void)hipSetDevice(prev); }
};

#define CHECK_COMMON(c, n)                                                              \
    if (!(c)) return ft8_fail("ctx is NULL");                                               \
    if ((n) < 0) return ft8_fail("nframes < 0");                                            \
    Entry entry_(c);                                                                    \
    HIP_TRY(entry_.err);

inline int force_ieee(const ft8gpu_ctx *c) { return (c->debug_flags & FT8GPU_DBG_FORCE_IEEE_DIV) ? 1 : 0; }

// One array argument of a stage entry: the caller's array (frame f at user + f * frame_bytes) and the context's staging
// buffer of the host form.  kIn is uploaded, kOut downloaded, kInOut both; kOutZeroed is cleared, then downloaded.
// user == nullptr: the argument is absent and the launch gets nullptr.
enum StageDir { kIn, kOut, kInOut, kOutZeroed };
struct StageArg { const void *user; void *stage; size_t frame_bytes; StageDir dir; };

// The frames [0, nframes) in chunks of at most max_frames: launch(n, p) runs the stage on the chunk [f0, f0 + n) with
// p[i] = user + f0 * frame_bytes (FT8GPU_DEVICE_PTRS) or the staging buffer (host form: uploaded before the launch,
// downloaded and synchronised after it).  launch returns 0, or -1 with the error set.
template <size_t N, class Launch>
int for_each_chunk(ft8gpu_ctx *c, int nframes, int flags, const StageArg (&a)[N], Launch launch) {
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    for (int f0 = 0; f0 < nframes; f0 += c->max_frames) {
        const int n = (nframes - f0 < c->max_frames) ? nframes - f0 : c->max_frames;
        char *user[N];
        void *p[N];
        for (size_t i = 0; i < N; ++i) {
            user[i] = a[i].user ? (char *)a[i].user + (size_t)f0 * a[i].frame_bytes : nullptr;
            p[i] = (dev || !user[i]) ? user[i] : a[i].stage;
        }
        if (!dev) {
            for (size_t i = 0; i < N; ++i) {
                if (!user[i]) continue;
                if (a[i].dir == kIn || a[i].dir == kInOut)
                    HIP_TRY(hipMemcpyAsync(p[i], user[i], n * a[i].frame_bytes, hipMemcpyHostToDevice, c->stream));
                if (a[i].dir == kOutZeroed) HIP_TRY(hipMemsetAsync(p[i], 0, n * a[i].frame_bytes, c->stream));
            }
        }
        if (launch(n, p)) return -1;
        if (dev) continue;
        for (size_t i = 0; i < N; ++i)
            if (user[i] && a[i].dir != kIn)
                HIP_TRY(hipMemcpyAsync(user[i], p[i], n * a[i].frame_bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// The array arguments every second-chance stage entry has (OSD, AP, match, combine, demod), as rows 0 .. 5 of a[]: the first
// input (mag, or iq for demod), cands, counts, status_in, then status_out and info with their staging buffers.  Records at and
// behind a frame's count keep the caller's bytes: both outputs are uploaded in the host form.  A stage's own arrays follow
// from row kCandRows.
constexpr int kCandRows = 6;
inline void cand_stage_rows(StageArg *a, const ft8gpu_ctx *c, const StageArg &first, const void *cands, const void *counts,
                            const void *status_in, void *status_out, void *out_stage, void *info, void *info_stage, size_t info_bytes) {
    const size_t mc = (size_t)c->params.max_candidates;
    a[0] = first;
    a[1] = { cands, c->d_cands, mc * sizeof(ft8gpu_candidate), kIn };
    a[2] = { counts, c->d_counts, sizeof(int32_t), kIn };
    a[3] = { status_in, c->d_status, mc * sizeof(ft8gpu_decode_status), kIn };
    a[4] = { status_out, out_stage, mc * sizeof(ft8gpu_decode_status), kInOut };
    a[5] = { info, info_stage, mc * info_bytes, kInOut };
}

// The pieces of [nstreams][nslots] frames that hold at most `bound` frames each: whole receivers (all their slots) while a
// receiver fits, else runs of consecutive slots of one receiver.  each(fn) calls fn(r0, rg, s0, ns, f0) piece by piece, in the
// order of the frames: rg receivers from r0, their slots [s0, s0 + ns), first frame f0 = r0 * nslots + s0; ns < nslots only
// with rg == 1.  fn returns 0 to go on.
constexpr long long kNoBound = LLONG_MAX;
struct Pieces {
    int nstreams, nslots, rg_max, ns_max;
    Pieces(int nstreams_, int nslots_, long long bound) : nstreams(nstreams_), nslots(nslots_) {
        const long long fit = bound / nslots;                        // whole receivers per piece
        ns_max = fit >= 1 ? nslots : (int)bound;
        rg_max = fit >= 1 ? (int)(fit < nstreams ? fit : nstreams) : 1;
    }
    template <class Fn>
    int each(Fn fn) const {
        for (int r0 = 0; r0 < nstreams; r0 += rg_max) {
            const int rg = nstreams - r0 < rg_max ? nstreams - r0 : rg_max;
            for (int s0 = 0; s0 < nslots; s0 += ns_max) {
                const int ns = nslots - s0 < ns_max ? nslots - s0 : ns_max;
                if (const int rc = fn(r0, rg, s0, ns, (size_t)r0 * nslots + s0)) return rc;
            }
        }
        return 0;
    }
};

// One chunk of a whole-path call, on the device: n frames, their records so far and, if wanted, their n_by_stage rows of
// passes * cols counts.
struct Chunk {
    ft8gpu_ctx *c;
    int n, passes, cols;
    ft8gpu_message *msgs;
    int32_t *n_msgs, *nbs;
    // nbs[f][col..] = n_msgs[f]: the count after a stage, carried into the columns of the stages that may not run
    int counts_to(int col) const {
        if (nbs) HIP_TRY(launch_pass_counts(n_msgs, nbs, n, passes * cols, col, c->stream));
        return 0;
    }
};
// One pass of a chunk: its waterfall, candidates, counts and statuses, its slot -> frame map (nullptr: slot f is frame f) and
// number of slots.  A Rescue runs on the pass's failures, in place; col is the first n_by_stage column of its stages.
struct PassSet {
    const uint8_t *mag;
    const ft8gpu_candidate *cands;
    const int32_t *counts;
    ft8gpu_decode_status *status;
    const int32_t *map;
    int nslots;
};
using Rescue = std::function<int(const Chunk &k, const PassSet &f, int col)>;
// One slot of a piece of the slot-major whole path: the slot's rg frames start at frame o of the pipeline's buffers; their
// records dm, counts pn and n_by_stage rows pb ([rg][2], column 0 filled); st: the rg receivers' states (device memory).
using SlotStages = std::function<int(size_t o, int rg, void *st, ft8gpu_message *dm, int32_t *pn, int32_t *pb)>;

// api_context.hip
int probe_streams(ft8gpu_ctx *c);             // (re)establishes c->overlap_ok for the current main stream
// api_pipeline.hip: the whole path on device pointers; all intermediates in the context's HBM buffers
int run_pipeline(ft8gpu_ctx *c, const float *d_iq, int n, struct decoder_results *d_dec, int32_t *d_nres);
// the same with the messages tail: noise baseline + message records instead of the spot collection
int run_pipeline_messages(ft8gpu_ctx *c, const float *d_iq, int n, ft8gpu_message *d_msgs, int32_t *d_nmsgs);
// api_messages.hip: allocates d_base / d_msgtab on the first messages call
int ensure_messages_buffers(ft8gpu_ctx *c);
// api_multipass.hip: allocates the multi-pass buffers on the first multi-pass call; the masking whole path behind
// ft8gpu_decode_messages_passes / _deep / _ap (checked arguments, buffers of the rescue stages in place): pass 1, then masking
// passes up to `passes`, `rescue` (may be empty) on every pass's failures
int ensure_multipass_buffers(ft8gpu_ctx *c);
int decode_messages_masked(ft8gpu_ctx *c, const float *iq, int nframes, int passes, int cols, ft8gpu_message *msgs, int32_t *n_msgs,
                           int32_t *n_by_stage, int flags, const Rescue &rescue);
// api_osd.hip: allocates the OSD buffers on the first OSD call; refuses arguments out of range; the OSD rescue step, whose
// count goes to column col
int ensure_osd_buffers(ft8gpu_ctx *c);
int check_osd_args(int order, int max_hard_errors);
int osd_step(const Chunk &k, const PassSet &f, int col, int order, int max_hard_errors);
// api_ap.hip: refuses hypotheses and gates out of range, with the error text set (also for AP on the demodulated soft bits)
int check_ap_args(const ft8gpu_ap_hypothesis *hyps, int nhyp, int max_hard_errors);
// api_match.hip: the slot-major whole path behind ft8gpu_decode_messages_expected / _combined
int decode_messages_slot_major(ft8gpu_ctx *c, const float *iq, int nstreams, int nslots, void *state, size_t state_bytes,
                               ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags, const SlotStages &slot);
// api_subtract.hip: uploads the subtraction's constant tables (d_subtab) on the first call that needs them
int ensure_subtract_tables(ft8gpu_ctx *c);
// ft8gpu_decode_batch with one more form: kIqOnDevice, frames resident on the context's GPU and records to host arrays
// (used by the multi-GPU entries; not part of the ABI, whose entry passes on FT8GPU_DEVICE_PTRS only)
constexpr int kIqOnDevice = 2;
int decode_batch(ft8gpu_ctx *c, const float *iq, int nframes, struct decoder_results *decodes, int32_t *n_results, int flags);
// api_glue.hip: the context's scratch blocks at these sizes or more (0: not needed).  The stream is synchronised only if one of
// them has to grow, since earlier launches may still use the old block.
int ensure_scratch(ft8gpu_ctx *c, size_t b0, size_t b1, size_t b2, size_t b3);
// the host form's staging, on the first call that needs it: the records; the frames and (msgs) the records; the n_by_stage rows
int ensure_msgs_staging(ft8gpu_ctx *c);
int ensure_host_staging(ft8gpu_ctx *c, bool msgs = true);
int ensure_counts_staging(ft8gpu_ctx *c);

// a lazily allocated pair of [max_frames][*cap] records follows cap_candidates when ft8gpu_set_params grows it
template <class A, class B>
int follow_cap(ft8gpu_ctx *c, A **a, B **b, int *cap, const char *what) {
    if (*cap >= c->cap_candidates) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));                       // the old pair may still be in use
    return c->mem.pair(a, b, cap, c->cap_candidates, (size_t)c->max_frames, what);
}

// a kernel file's constant tables, uploaded on the context's first call that needs them (the upload reads a static host object)
inline int tables_once(ft8gpu_ctx *c, bool *done, hipError_t (*init)(hipStream_t)) {
    if (!*done) { HIP_TRY(init(c->stream)); HIP_TRY(hipStreamSynchronize(c->stream)); }
    *done = true;
    return 0;
}
