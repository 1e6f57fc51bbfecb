// audio.hip -- the audio front end (include/ft8gpu.h "12 kHz audio"): 12 000 sps real clips -> the 3200 sps complex frames of the
// decoder, one frame per band of a clip, and the merge of the bands' records of the whole path.
//
// Frames kernel.  One workgroup of 256 threads handles one clip and kTilesPerGroup tiles of kTileOut = 768 outputs, each tile for
// every band of the clip in turn, so a tile's input is fetched once (16-byte loads, kept in registers as it lies in memory) and
// the mixer table is brought into LDS once per workgroup.  Per band the mixed samples z are staged in LDS as (re, im) pairs, one
// 8-byte LDS read per tap.  Wave w takes the outputs whose tap phase r = (15 m + 79) mod 4 is w, so the 40 taps h[w + 4 j] are
// uniform per wave (scalar loads), and a lane takes three consecutive outputs of that phase: their windows overlap (N moves by 15
// per output), so 70 staged samples serve 120 tap products.  Walking the window downwards feeds every output its taps in
// ascending j, the sequential sum of the rule.  Consecutive lanes' windows are 45 pairs apart, an odd stride, so the 32-lane
// groups of an 8-byte read meet 32 distinct bank pairs.  The mixer table is padded by one entry per 32: its index advances from
// lane to lane by a multiple of 32 for every base that is a multiple of 4.  The outputs are restaged through LDS so that a lane
// stores 16 contiguous bytes per plane.  46.6 KB of LDS let three workgroups share a CU, and the kernel is held to the 168
// registers of three waves per SIMD: it waits on LDS and on its loads more than it computes (measured: 4.2 ms per 8192 frames
// with two waves per SIMD, 2.8 ms with three).  The mixing, the tap products and the sums are plain C++; -ffp-contract=off keeps
// every product and add a single IEEE operation.
#include "audio.h"
#include "merge_dev.h"

namespace {

constexpr int kPerLane = 3;                                 // consecutive outputs of one phase per lane
constexpr int kPhaseOut = 64 * kPerLane;                    // outputs of one phase (one wave) per tile
constexpr int kTileOut = 4 * kPhaseOut;                     // 768 outputs per tile
constexpr int kTiles = (kNSamples + kTileOut - 1) / kTileOut;                    // 63, the last one partial
constexpr int kTilesPerGroup = 3;                           // tiles per workgroup
constexpr int kGroups = kTiles / kTilesPerGroup;            // 21 workgroups per clip
constexpr int kTileIn = 15 * kTileOut / 4;                  // 2880 input samples advance per tile
constexpr int kLead = 24;                                   // samples in front of a tile's N(m0) - 19: >= 20, a multiple of 8
constexpr int kStage = 3072;                                // staged samples per tile
constexpr int kSpan = 15 * (kPerLane - 1) + 40;             // 70 staged samples under a lane's three windows
constexpr int kMixEntries = FT8GPU_AUDIO_MIX + FT8GPU_AUDIO_MIX / 32;            // the padded table
static_assert(kTiles % kTilesPerGroup == 0, "whole groups of tiles");
// the last staged sample a tile reads: N - nb of its last output, phase 3
static_assert(15 * (kPhaseOut - 1) + ((15 * 3 + 79) >> 2) + kLead < kStage, "input tile fits the stage");
static_assert(19 + kLead - 39 >= 0 && kLead % 8 == 0 && kTileIn % 8 == 0, "first staged sample, 16-byte groups");
static_assert((15 * kPerLane) % 2 == 1 && 15 * (kPerLane - 1) + 39 + 1 == kSpan, "odd lane stride, the window under a lane's outputs");
static_assert(kNSamples % 4 == 0 && kTileOut % 4 == 0, "whole 16-byte stores");

// a thread's samples: group t + 256 u of G consecutive samples, u < U, while the group lies below kStage; G = 8 (S16) or 4 (F32)
template <int FMT> struct Fmt;
template <> struct Fmt<FT8GPU_AUDIO_S16> { static constexpr int G = 8, U = 2; using T = int16_t; };
template <> struct Fmt<FT8GPU_AUDIO_F32> { static constexpr int G = 4, U = 3; using T = float; };

// one dword of a clip as it lies in memory, sample by sample; a sample outside the clip is zero
__device__ inline uint32_t load_word(const int16_t *pcm, int n, int nsamples) {
    const uint32_t lo = (n >= 0 && n < nsamples) ? (uint16_t)pcm[n] : 0u;
    const uint32_t hi = (n + 1 >= 0 && n + 1 < nsamples) ? (uint16_t)pcm[n + 1] : 0u;
    return lo | hi << 16;
}
__device__ inline uint32_t load_word(const float *pcm, int n, int nsamples) { return (n >= 0 && n < nsamples) ? __float_as_uint(pcm[n]) : 0u; }
// sample e of a group's four dwords: int16 times 2^-15 (exact), or the float as it is
template <int FMT>
__device__ inline float sample(const uint32_t *w, int e) {
    if constexpr (FMT == FT8GPU_AUDIO_S16) return (float)(int16_t)((e & 1) ? w[e >> 1] >> 16 : w[e >> 1] & 0xffffu) * 3.0517578125e-05f;
    else return __uint_as_float(w[e]);
}

template <int FMT>
__global__ __launch_bounds__(256, 3)                        // three workgroups per CU by LDS: three waves per SIMD
void ft8_audio_frames_kernel(const void *__restrict__ pcm_, int nsamples, AudioBands bands, int g0, int g1,
                             const AudioTables *__restrict__ tab, float *__restrict__ out) {
    using T = typename Fmt<FMT>::T;
    constexpr int G = Fmt<FMT>::G, U = Fmt<FMT>::U;
    static_assert(G * 256 * (U - 1) < kStage && G * 256 * U >= kStage && kStage % G == 0, "the groups cover the stage");
    __shared__ __attribute__((aligned(16))) float2 zz[kStage];
    __shared__ __attribute__((aligned(16))) float xr[kTileOut], xi[kTileOut];
    __shared__ __attribute__((aligned(16))) float2 wm[kMixEntries];
    const int tid = threadIdx.x;
    const int group = blockIdx.x % kGroups;
    const int clip = g0 / bands.n + blockIdx.x / kGroups;
    const T *pcm = (const T *)pcm_ + (size_t)clip * nsamples;
    const bool aligned = ((uintptr_t)pcm & 15) == 0;

    for (int i = tid; i < FT8GPU_AUDIO_MIX; i += 256) wm[i + (i >> 5)] = tab->wm[i];
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave = the tap phase r
    const int q = (3 - w) & 3;                              // its outputs have m mod 4 = q: (15 q + 79) mod 4 = w
    const int cw = (15 * q + 79) >> 2;
    float h[40];
#pragma unroll
    for (int j = 0; j < 40; ++j) h[j] = tab->h[w + 4 * j];
    __syncthreads();

#pragma nounroll
    for (int tile = group * kTilesPerGroup; tile < (group + 1) * kTilesPerGroup; ++tile) {
        const int nb = kTileIn * tile - kLead;              // the clip sample staged at index 0
        // the thread's index again, opaque to the optimiser: what is derived from it below (LDS and clip offsets) is recomputed
        // per tile in a few instructions, not kept in registers across the loops, where it would cost the third wave per SIMD
        int t = tid;
        asm volatile("" : "+v"(t));
        // the input tile, once for all bands: 16 bytes per group as they lie in memory (converted when they are mixed: eight
        // registers for sixteen int16 samples)
        uint32_t raw[4 * U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i0 = G * (t + 256 * u);
            const int n = nb + i0;
            if (i0 >= kStage) {                             // (uniform per wave)
#pragma unroll
                for (int i = 0; i < 4; ++i) raw[4 * u + i] = 0u;
            } else if (aligned && n >= 0 && n + G <= nsamples) {
                const uint4 v = *(const uint4 *)(pcm + n);
                raw[4 * u] = v.x;
                raw[4 * u + 1] = v.y;
                raw[4 * u + 2] = v.z;
                raw[4 * u + 3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) raw[4 * u + i] = load_word(pcm, n + (G / 4) * i, nsamples);
            }
        }

#pragma nounroll
        for (int b = 0; b < bands.n; ++b) {
            const int g = clip * bands.n + b;
            if (g < g0 || g >= g1) continue;                // uniform
            const unsigned f = (unsigned)(bands.base[b] + 128);
            asm volatile("" : "+v"(t));                    // (again: the band loop's offsets are not worth registers either)
            // z[n] = a[n] * wm[(n f) mod 1920].  A sample outside the clip is a = +0 times some table entry (a group lies wholly on
            // one side of sample 0: kLead % 8 == 0), a zero of either sign: its tap products are zeros, and a sum that starts
            // from +0 is never -0, so adding them changes no bit of it -- the same outputs as with z = +0.
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i0 = G * (t + 256 * u);
                if (i0 >= kStage) continue;                 // (uniform per wave)
                const int n = nb + i0;
                float2 v[G];
                unsigned k = n >= 0 ? ((unsigned)n * f) % FT8GPU_AUDIO_MIX : 0u;
#pragma unroll
                for (int e = 0; e < G; ++e) {
                    const float2 c = wm[k + (k >> 5)];
                    const float av = sample<FMT>(raw + 4 * u, e);
                    v[e] = make_float2(av * c.x, av * c.y);
                    k += f;
                    if (k >= FT8GPU_AUDIO_MIX) k -= FT8GPU_AUDIO_MIX;
                }
#pragma unroll
                for (int e = 0; e < G; e += 2) *(float4 *)&zz[i0 + e] = make_float4(v[e].x, v[e].y, v[e + 1].x, v[e + 1].y);
            }
            __syncthreads();
            // y[m] = sum over j ascending of h[r + 4 j] * z[N - j] for m = m0 + q + 4 k, k = 3 lane + i: output i reads the staged
            // sample at zp[39 + d] as its tap j = 15 i - d
            {
                const float2 *zp = zz + (15 * kPerLane * (t & 63) + cw + kLead - 39);
                float sr[kPerLane], si[kPerLane];
#pragma unroll
                for (int i = 0; i < kPerLane; ++i) sr[i] = si[i] = 0.0f;
#pragma unroll
                for (int d = 15 * (kPerLane - 1); d >= -39; --d) {
                    if (d == 7 || d == -16) __builtin_amdgcn_sched_barrier(0);     // a third of the window's reads in flight at a time
                    const float2 z = zp[39 + d];
#pragma unroll
                    for (int i = 0; i < kPerLane; ++i) {
                        const int j = 15 * i - d;
                        if (j >= 0 && j < 40) {
                            sr[i] = sr[i] + h[j] * z.x;
                            si[i] = si[i] + h[j] * z.y;
                        }
                    }
                }
                // x[m] = y[m] * j^m, staged as [q][k]
#pragma unroll
                for (int i = 0; i < kPerLane; ++i) {
                    float pr, pi;
                    if (q == 0) { pr = sr[i]; pi = si[i]; }
                    else if (q == 1) { pr = -si[i]; pi = sr[i]; }
                    else if (q == 2) { pr = -sr[i]; pi = -si[i]; }
                    else { pr = si[i]; pi = -sr[i]; }
                    xr[q * kPhaseOut + kPerLane * (t & 63) + i] = pr;
                    xi[q * kPhaseOut + kPerLane * (t & 63) + i] = pi;
                }
            }
            __syncthreads();
            const int m = kTileOut * tile + 4 * t;
            if (t < kPhaseOut && m < kNSamples) {
                float *o = out + (size_t)(g - g0) * 2 * kNSamples + m;
                *(float4 *)o = make_float4(xr[t], xr[kPhaseOut + t], xr[2 * kPhaseOut + t], xr[3 * kPhaseOut + t]);
                *(float4 *)(o + kNSamples) = make_float4(xi[t], xi[kPhaseOut + t], xi[2 * kPhaseOut + t], xi[3 * kPhaseOut + t]);
            }
        }
    }
}

// One thread per clip: merge_dev.h's merge over the clip's bands; the bands of a clip overlap, so equal a91 is a duplicate
__global__ __launch_bounds__(64)
void ft8_audio_merge_kernel(const ft8gpu_message *__restrict__ band_msgs, const int32_t *__restrict__ band_n, int nclips,
                            AudioBands bands, ft8gpu_message *msgs, int32_t *__restrict__ n_msgs) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nclips) return;
    merge_parts<false>(band_msgs, band_n, c, bands.n, bands.base, msgs, n_msgs);
}

}  // namespace

hipError_t launch_audio_frames(const void *pcm, int format, int nsamples, const AudioBands &bands, int g0, int g1,
                               const AudioTables *tab, float *out, hipStream_t s) {
    if (g1 <= g0) return hipSuccess;
    const unsigned clips = (unsigned)((g1 - 1) / bands.n - g0 / bands.n + 1);
    if (format == FT8GPU_AUDIO_S16)
        ft8_audio_frames_kernel<FT8GPU_AUDIO_S16><<<dim3(clips * kGroups), dim3(256), 0, s>>>(pcm, nsamples, bands, g0, g1, tab, out);
    else
        ft8_audio_frames_kernel<FT8GPU_AUDIO_F32><<<dim3(clips * kGroups), dim3(256), 0, s>>>(pcm, nsamples, bands, g0, g1, tab, out);
    return hipGetLastError();
}

hipError_t launch_audio_merge(const ft8gpu_message *band_msgs, const int32_t *band_n, int nclips, const AudioBands &bands,
                              ft8gpu_message *msgs, int32_t *n_msgs, hipStream_t s) {
    ft8_audio_merge_kernel<<<dim3((unsigned)(nclips + 63) / 64), dim3(64), 0, s>>>(band_msgs, band_n, nclips, bands, msgs, n_msgs);
    return hipGetLastError();
}
