// gfsk.hip -- the GFSK synthesiser (include/ft8gpu.h "GFSK synthesis", DESIGN.md "GFSK synthesis"): FT8 signals as they are on
// the air, as 3200 sps planar I/Q frames or as 12 kHz real audio.
//   ft8_gfsk_kernel<Mode, Format>   grid (clip, tile): a workgroup of 1024 lanes owns kGfskTile consecutive output samples of one
//                                   clip, lane l the samples l, l + 1024, ... of the tile, so that adjacent lanes read adjacent
//                                   entries of the pulse table.  The clip's signal headers (step, start, amplitude, extended
//                                   tones) and the twiddle tables gc and gf are staged in LDS (70 KB: two workgroups, 32 waves,
//                                   per CU); the signals are walked in order, and one whose span misses the tile is skipped for
//                                   the whole tile.  gc and gf are indexed by the phase, which differs from lane to lane by
//                                   the signal's step: through the vector cache such a gather costs a tag look-up per lane
//                                   (measured: 20.2 against 4.4 ms for 4096 frames of 20 signals), in LDS a few bank conflicts.  Q and the ramp are
//                                   read through the cache: adjacent lanes, adjacent entries, and a pipe of its own beside LDS.
//   ft8_gfsk_faded_kernel<Mode, Format>   the same body with channels ("Fading channel"): a faded signal is walked once per path,
//                                   every sample's contribution multiplied by the path's complex gain, which is interpolated
//                                   between two adjacent grid values read through the cache (adjacent lanes, the same or adjacent
//                                   entries).  LDS grows by (delay, paths) per signal, 512 bytes: still two workgroups per CU.
//   ft8_gfsk_grid_kernel            the grid values of a chunk's faded paths, 1265 per (signal, path), 16 sinusoids each from gc
//                                   and gf in LDS, into HBM in front of the faded kernel.
//   ft8_gfsk_normalise_kernel<Format>   the second pass of peak normalisation: the clip's tile maxima -> one scale -> x * scale.
// The phase is integer arithmetic and every float step one IEEE operation (the build has -ffp-contract=off), so the output at
// noise_sigma == 0 is the rule's bytes.  The noise generator is the one of synth.hip, copied (its code object stays as it is).
#include "gfsk.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kPerLane = kGfskTile / kThreads;              // 8
constexpr int kNormThreads = 256, kNormTile = 2048, kNormPerLane = kNormTile / kNormThreads;   // the second pass: elementwise
static_assert(kGfskTile % kThreads == 0, "a lane owns a whole number of samples");

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// synth.hip's draw for (seed, global clip, sample): rad * (cos, sin)
__device__ __forceinline__ void noise_draw(uint64_t seed, uint64_t clip, int i, float sigma, float *ni, float *nq) {
    const uint64_t h = splitmix64(seed ^ splitmix64((clip << 20) + (uint64_t)i));
    const float u1 = ((float)(uint32_t)(h >> 40) + 1.0f) * (1.0f / 16777216.0f);   // (0, 1]
    const float u2 = (float)(uint32_t)((h >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);
    const float rad = sigma * sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    *ni = rad * cs;
    *nq = rad * sn;
}

__device__ __forceinline__ int16_t to_s16(float x) {
    float r = rintf(x * 32768.0f);
    r = r > 32767.0f ? 32767.0f : r;
    r = r < -32768.0f ? -32768.0f : r;
    return r == r ? (int16_t)(int)r : (int16_t)0;
}

// the body of both kernels; Faded: ch and grid are looked at, and a signal with ch.paths != 0 goes through its paths' gains
template <int Mode, int Format, bool Faded>
__device__ __forceinline__
void gfsk_tile(const GfskHeader *__restrict__ hdr, const GfskChannel *__restrict__ ch, const float2 *__restrict__ grid, int nsig, int nsamples,
               int ntiles, const GfskTables *__restrict__ tab, float noise_sigma, uint64_t seed, uint64_t first, void *__restrict__ out,
               float *__restrict__ tile_max) {
    constexpr bool kIq = Mode == FT8GPU_GFSK_IQ;
    constexpr int kSps = kIq ? FT8GPU_GFSK_SPS_IQ : FT8GPU_GFSK_SPS_AUDIO;
    constexpr int kSpan = FT8GPU_NN * kSps, kRamp = kSps / 8;
    __shared__ __attribute__((aligned(16))) float2 s_gc[FT8GPU_GFSK_TWIDDLES], s_gf[FT8GPU_GFSK_TWIDDLES];
    __shared__ uint32_t s_hdr[FT8GPU_GFSK_MAX_SIGNALS * (sizeof(GfskHeader) / 4)];
    __shared__ float s_max[kThreads / 64];
    __shared__ int2 s_ch[Faded ? FT8GPU_GFSK_MAX_SIGNALS : 1];              // (d, paths) of the clip's signals

    const int tid = threadIdx.x;
    const int clip = blockIdx.x / ntiles, tile = blockIdx.x - clip * ntiles;
    const int len = kIq ? kNSamples : nsamples;
    const int t0 = tile * kGfskTile;
    const uint32_t *src = (const uint32_t *)(hdr + (size_t)clip * nsig);
    for (int w = tid; w < nsig * (int)(sizeof(GfskHeader) / 4); w += kThreads) s_hdr[w] = src[w];
    if constexpr (Faded) {
        if (tid < nsig) s_ch[tid] = make_int2(ch[(size_t)clip * nsig + tid].d, (int)ch[(size_t)clip * nsig + tid].paths);
    }
    if (nsig > 0) {                                                         // the same for every lane
        const float4 *gc4 = (const float4 *)tab->gc, *gf4 = (const float4 *)tab->gf;
        for (int w = tid; w < FT8GPU_GFSK_TWIDDLES / 2; w += kThreads) {
            ((float4 *)s_gc)[w] = gc4[w];
            ((float4 *)s_gf)[w] = gf4[w];
        }
    }
    __syncthreads();
    const GfskHeader *sh = (const GfskHeader *)s_hdr;
    const uint32_t *__restrict__ Q = kIq ? tab->q_iq : tab->q_audio;
    const float *__restrict__ ramp = kIq ? tab->ramp_iq : tab->ramp_audio;

    float vi[kPerLane], vq[kPerLane];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) vi[j] = vq[j] = 0.0f;

    for (int s = 0; s < nsig; ++s) {
        if constexpr (!Faded) {                                             // the unfaded kernel's loop, kept as it was built
            const int start = sh[s].start;
            if (start >= t0 + kGfskTile || start + kSpan <= t0) continue;   // the same for every lane
            const uint32_t step = sh[s].step;
            const float amp = sh[s].amplitude;
            const uint8_t *e = sh[s].e;
#pragma unroll
            for (int j = 0; j < kPerLane; ++j) {
                const int n = t0 + tid + j * kThreads - start;              // the local sample n'
                if (n < 0 || n >= kSpan) continue;
                const int m = n / kSps, k = n - m * kSps;
                const uint32_t phi = step * (uint32_t)n + (uint32_t)e[m] * Q[k + 2 * kSps] + (uint32_t)e[m + 1] * Q[k + kSps] +
                                     (uint32_t)e[m + 2] * Q[k];
                const float2 c = s_gc[phi >> 20], f = s_gf[(phi >> 8) & 4095u];
                const float env = n < kRamp ? ramp[n] : (n >= kSpan - kRamp ? ramp[kSpan - 1 - n] : 1.0f);
                const float a = amp * env;
                vi[j] = vi[j] + a * (c.x * f.x - c.y * f.y);
                if (kIq) vq[j] = vq[j] + a * (c.y * f.x + c.x * f.y);
            }
        } else {                                                            // with channels: a faded signal once per path
            const int paths = s_ch[s].y;                                    // 0: the unfaded rule.  The same for every lane
#pragma unroll 1
            for (int p = 0; p < (paths == 2 ? 2 : 1); ++p) {
                const int start = p ? sh[s].start + s_ch[s].x : sh[s].start;
                if (start >= t0 + kGfskTile || start + kSpan <= t0) continue;   // the same for every lane
                const uint32_t step = sh[s].step;
                const float amp = sh[s].amplitude;
                const uint8_t *e = sh[s].e;
                const float2 *__restrict__ g = grid + (((size_t)clip * nsig + s) * 2 + p) * kGfskGrid;
#pragma unroll
                for (int j = 0; j < kPerLane; ++j) {
                    const int n = t0 + tid + j * kThreads - start;              // the local sample n' (of the path)
                    if (n < 0 || n >= kSpan) continue;
                    const int m = n / kSps, k = n - m * kSps;
                    const uint32_t phi = step * (uint32_t)n + (uint32_t)e[m] * Q[k + 2 * kSps] + (uint32_t)e[m + 1] * Q[k + kSps] +
                                         (uint32_t)e[m + 2] * Q[k];
                    const float2 c = s_gc[phi >> 20], f = s_gf[(phi >> 8) & 4095u];
                    const float env = n < kRamp ? ramp[n] : (n >= kSpan - kRamp ? ramp[kSpan - 1 - n] : 1.0f);
                    const float a = amp * env;
                    const float xr = a * (c.x * f.x - c.y * f.y), xi = a * (c.y * f.x + c.x * f.y);
                    if (paths) {                                               // the path's gain between its grid points jg and jg + 1
                        constexpr int kStep = kIq ? FT8GPU_CHANNEL_STEP_IQ : FT8GPU_CHANNEL_STEP_AUDIO;
                        const int jg = n / kStep;
                        const float t = (float)(n - jg * kStep) / (float)kStep;
                        const float2 g0 = g[jg], g1 = g[jg + 1];
                        const float gr = g0.x + (g1.x - g0.x) * t, gi = g0.y + (g1.y - g0.y) * t;
                        vi[j] = vi[j] + (xr * gr - xi * gi);
                        if (kIq) vq[j] = vq[j] + (xr * gi + xi * gr);
                    } else {
                        vi[j] = vi[j] + xr;
                        if (kIq) vq[j] = vq[j] + xi;
                    }
                }
            }
        }
    }

    float peak = 0.0f;
    const size_t base = (size_t)clip * (kIq ? 2 * (size_t)kNSamples : (size_t)nsamples);
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const int i = t0 + tid + j * kThreads;
        if (i >= len) continue;
        float xi = vi[j], xq = vq[j];
        if (noise_sigma > 0.0f) {
            float ni, nq;
            noise_draw(seed, first + (uint64_t)clip, i, noise_sigma, &ni, &nq);
            xi = xi + ni;
            xq = xq + nq;
        }
        if (kIq) {
            ((float *)out)[base + i] = xi;
            ((float *)out)[base + kNSamples + i] = xq;
            peak = fmaxf(peak, fmaxf(fabsf(xi), fabsf(xq)));
        } else {
            if (Format == FT8GPU_AUDIO_S16) ((int16_t *)out)[base + i] = to_s16(xi);
            else ((float *)out)[base + i] = xi;
            peak = fmaxf(peak, fabsf(xi));
        }
    }
    if (!tile_max) return;                                                  // the same for every lane
    for (int o = 32; o > 0; o >>= 1) peak = fmaxf(peak, __shfl_xor(peak, o, 64));
    if ((tid & 63) == 0) s_max[tid >> 6] = peak;
    __syncthreads();
    if (tid == 0) {
        float m = s_max[0];
        for (int w = 1; w < kThreads / 64; ++w) m = fmaxf(m, s_max[w]);
        tile_max[(size_t)clip * ntiles + tile] = m;
    }
}

template <int Mode, int Format>
__global__ __launch_bounds__(kThreads)
void ft8_gfsk_kernel(const GfskHeader *__restrict__ hdr, int nsig, int nsamples, int ntiles, const GfskTables *__restrict__ tab,
                     float noise_sigma, uint64_t seed, uint64_t first, void *__restrict__ out, float *__restrict__ tile_max) {
    gfsk_tile<Mode, Format, false>(hdr, nullptr, nullptr, nsig, nsamples, ntiles, tab, noise_sigma, seed, first, out, tile_max);
}

template <int Mode, int Format>
__global__ __launch_bounds__(kThreads, 8)                                   // 8 waves per SIMD: two workgroups per CU, as the unfaded kernel has
void ft8_gfsk_faded_kernel(const GfskHeader *__restrict__ hdr, const GfskChannel *__restrict__ ch, const float2 *__restrict__ grid, int nsig,
                           int nsamples, int ntiles, const GfskTables *__restrict__ tab, float noise_sigma, uint64_t seed, uint64_t first,
                           void *__restrict__ out, float *__restrict__ tile_max) {
    gfsk_tile<Mode, Format, true>(hdr, ch, grid, nsig, nsamples, ntiles, tab, noise_sigma, seed, first, out, tile_max);
}

// grid (clip, part): a workgroup owns kGfskTile consecutive entries of the clip's [nsig][2][kGfskGrid] grid values, lane l the
// entries l, l + 1024, ...; gc and gf in LDS as above, beside the taps of the at most kGridPairs (signal, path) pairs the part touches
constexpr int kGridPairs = (kGfskTile + kGfskGrid - 2) / kGfskGrid + 1;     // 8
constexpr int kTapWords = 2 * FT8GPU_CHANNEL_TAPS + 2;                      // gstep, theta, w, paths

__global__ __launch_bounds__(kThreads)
void ft8_gfsk_grid_kernel(const GfskChannel *__restrict__ ch, int nsig, int nparts, const GfskTables *__restrict__ tab, float2 *__restrict__ grid) {
    __shared__ __attribute__((aligned(16))) float2 s_gc[FT8GPU_GFSK_TWIDDLES], s_gf[FT8GPU_GFSK_TWIDDLES];
    __shared__ uint32_t s_tap[kGridPairs][kTapWords];
    const int tid = threadIdx.x;
    const int clip = blockIdx.x / nparts, part = blockIdx.x - clip * nparts;
    const int npairs = 2 * nsig, total = npairs * kGfskGrid;
    const int e0 = part * kGfskTile, pair0 = e0 / kGfskGrid;
    const float4 *gc4 = (const float4 *)tab->gc, *gf4 = (const float4 *)tab->gf;
    for (int w = tid; w < FT8GPU_GFSK_TWIDDLES / 2; w += kThreads) {
        ((float4 *)s_gc)[w] = gc4[w];
        ((float4 *)s_gf)[w] = gf4[w];
    }
    if (tid < kGridPairs * kTapWords) {
        const int lp = tid / kTapWords, w = tid - lp * kTapWords, pair = pair0 + lp;
        if (pair < npairs) {
            const GfskChannel &c = ch[(size_t)clip * nsig + (pair >> 1)];
            const int p = pair & 1;
            s_tap[lp][w] = w < FT8GPU_CHANNEL_TAPS ? c.gstep[p][w] : (w < 2 * FT8GPU_CHANNEL_TAPS ? c.theta[p][w - FT8GPU_CHANNEL_TAPS] :
                           (w == 2 * FT8GPU_CHANNEL_TAPS ? __float_as_uint(c.w[p]) : (uint32_t)(c.paths > (uint32_t)p)));
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
        const int e = e0 + tid + i * kThreads;
        if (e >= total) continue;
        const int pair = e / kGfskGrid, j = e - pair * kGfskGrid;
        const uint32_t *tap = s_tap[pair - pair0];
        if (!tap[2 * FT8GPU_CHANNEL_TAPS + 1]) continue;                    // a path the signal does not have
        float sc = 0.0f, ss = 0.0f;
#pragma unroll
        for (int m = 0; m < FT8GPU_CHANNEL_TAPS; ++m) {
            const uint32_t ph = tap[FT8GPU_CHANNEL_TAPS + m] + tap[m] * (uint32_t)j;
            const float2 c = s_gc[ph >> 20], f = s_gf[(ph >> 8) & 4095u];
            sc = sc + (c.x * f.x - c.y * f.y);
            ss = ss + (c.y * f.x + c.x * f.y);
        }
        const float w = __uint_as_float(tap[2 * FT8GPU_CHANNEL_TAPS]);
        grid[(size_t)clip * total + e] = make_float2(w * (0.25f * sc), w * (0.25f * ss));
    }
}

template <int Format>
__global__ __launch_bounds__(kNormThreads)
void ft8_gfsk_normalise_kernel(const float *x, const float *__restrict__ tile_max, int len, int ntiles, int nparts, float peak, void *out) {
    __shared__ float s_scale;
    const int tid = threadIdx.x;
    const int clip = blockIdx.x / nparts, part = blockIdx.x - clip * nparts;
    if (tid < 64) {
        float m = 0.0f;
        for (int t = tid; t < ntiles; t += 64) m = fmaxf(m, tile_max[(size_t)clip * ntiles + t]);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (tid == 0) s_scale = peak / fmaxf(m, 1e-24f);
    }
    __syncthreads();
    const float scale = s_scale;
    const size_t base = (size_t)clip * (size_t)len;
#pragma unroll
    for (int j = 0; j < kNormPerLane; ++j) {
        const int i = part * kNormTile + tid + j * kNormThreads;
        if (i >= len) continue;
        const float v = x[base + i] * scale;
        if (Format == FT8GPU_AUDIO_S16) ((int16_t *)out)[base + i] = to_s16(v);
        else ((float *)out)[base + i] = v;
    }
}

}  // namespace

hipError_t launch_gfsk(int mode, int format, const GfskHeader *hdr, int nclips, int nsig, int nsamples, const GfskTables *tab,
                       float noise_sigma, uint64_t seed, uint64_t first, void *out, float *tile_max, hipStream_t s) {
    if (nclips < 1) return hipSuccess;
    const bool iq = mode == FT8GPU_GFSK_IQ;
    if ((!iq && mode != FT8GPU_GFSK_AUDIO) || (format != FT8GPU_AUDIO_S16 && format != FT8GPU_AUDIO_F32) || (iq && format != FT8GPU_AUDIO_F32) ||
        nsig < 0 || nsig > FT8GPU_GFSK_MAX_SIGNALS || (!iq && (nsamples < 1 || nsamples > FT8GPU_AUDIO_NSAMPLES)))
        return hipErrorInvalidValue;
    const int ntiles = gfsk_tiles(mode, nsamples);
    const dim3 grid((unsigned)nclips * (unsigned)ntiles), block(kThreads);
    if (iq)
        hipLaunchKernelGGL((ft8_gfsk_kernel<FT8GPU_GFSK_IQ, FT8GPU_AUDIO_F32>), grid, block, 0, s, hdr, nsig, nsamples, ntiles, tab,
                           noise_sigma, seed, first, out, tile_max);
    else if (format == FT8GPU_AUDIO_S16)
        hipLaunchKernelGGL((ft8_gfsk_kernel<FT8GPU_GFSK_AUDIO, FT8GPU_AUDIO_S16>), grid, block, 0, s, hdr, nsig, nsamples, ntiles, tab,
                           noise_sigma, seed, first, out, tile_max);
    else
        hipLaunchKernelGGL((ft8_gfsk_kernel<FT8GPU_GFSK_AUDIO, FT8GPU_AUDIO_F32>), grid, block, 0, s, hdr, nsig, nsamples, ntiles, tab,
                           noise_sigma, seed, first, out, tile_max);
    return hipGetLastError();
}

hipError_t launch_gfsk_grid(const GfskChannel *ch, int nclips, int nsig, const GfskTables *tab, float2 *grid, hipStream_t s) {
    if (nclips < 1 || nsig == 0) return hipSuccess;
    if (nsig < 0 || nsig > FT8GPU_GFSK_MAX_SIGNALS) return hipErrorInvalidValue;
    const int nparts = (2 * nsig * kGfskGrid + kGfskTile - 1) / kGfskTile;
    hipLaunchKernelGGL(ft8_gfsk_grid_kernel, dim3((unsigned)nclips * (unsigned)nparts), dim3(kThreads), 0, s, ch, nsig, nparts, tab, grid);
    return hipGetLastError();
}

hipError_t launch_gfsk_faded(int mode, int format, const GfskHeader *hdr, const GfskChannel *ch, const float2 *grid, int nclips, int nsig,
                             int nsamples, const GfskTables *tab, float noise_sigma, uint64_t seed, uint64_t first, void *out,
                             float *tile_max, hipStream_t s) {
    if (nclips < 1) return hipSuccess;
    const bool iq = mode == FT8GPU_GFSK_IQ;
    if ((!iq && mode != FT8GPU_GFSK_AUDIO) || (format != FT8GPU_AUDIO_S16 && format != FT8GPU_AUDIO_F32) || (iq && format != FT8GPU_AUDIO_F32) ||
        nsig < 0 || nsig > FT8GPU_GFSK_MAX_SIGNALS || (!iq && (nsamples < 1 || nsamples > FT8GPU_AUDIO_NSAMPLES)))
        return hipErrorInvalidValue;
    const int ntiles = gfsk_tiles(mode, nsamples);
    const dim3 grd((unsigned)nclips * (unsigned)ntiles), block(kThreads);
    if (iq)
        hipLaunchKernelGGL((ft8_gfsk_faded_kernel<FT8GPU_GFSK_IQ, FT8GPU_AUDIO_F32>), grd, block, 0, s, hdr, ch, grid, nsig, nsamples, ntiles, tab,
                           noise_sigma, seed, first, out, tile_max);
    else if (format == FT8GPU_AUDIO_S16)
        hipLaunchKernelGGL((ft8_gfsk_faded_kernel<FT8GPU_GFSK_AUDIO, FT8GPU_AUDIO_S16>), grd, block, 0, s, hdr, ch, grid, nsig, nsamples, ntiles,
                           tab, noise_sigma, seed, first, out, tile_max);
    else
        hipLaunchKernelGGL((ft8_gfsk_faded_kernel<FT8GPU_GFSK_AUDIO, FT8GPU_AUDIO_F32>), grd, block, 0, s, hdr, ch, grid, nsig, nsamples, ntiles,
                           tab, noise_sigma, seed, first, out, tile_max);
    return hipGetLastError();
}

hipError_t launch_gfsk_normalise(int format, const float *x,const float *tile_max, int nclips, int len, int ntiles, float peak,
                                 void *out, hipStream_t s) {
    if (nclips < 1) return hipSuccess;
    if (len < 1 || ntiles < 1 || (format != FT8GPU_AUDIO_S16 && format != FT8GPU_AUDIO_F32)) return hipErrorInvalidValue;
    const int nparts = (len + kNormTile - 1) / kNormTile;
    const dim3 grid((unsigned)nclips * (unsigned)nparts), block(kNormThreads);
    if (format == FT8GPU_AUDIO_S16)
        hipLaunchKernelGGL(ft8_gfsk_normalise_kernel<FT8GPU_AUDIO_S16>, grid, block, 0, s, x, tile_max, len, ntiles, nparts, peak, out);
    else
        hipLaunchKernelGGL(ft8_gfsk_normalise_kernel<FT8GPU_AUDIO_F32>, grid, block, 0, s, x, tile_max, len, ntiles, nparts, peak, out);
    return hipGetLastError();
}
