// pcm.hip -- the PCM front end (include/ft8gpu.h "PCM front end"): 48 .. 768 ksps real or complex captures, int16 or float32 ->
// the 3200 sps complex frames of the decoder, one frame per channel of a capture, and the merge of the channels' records.
//
// Planes kernel (stage A and the second mixer), one instance per M = D / 3.  A workgroup of 256 threads takes T consecutive 9600
// sps outputs of one capture.  The M (T + 7) + 1 samples under them are fetched once, element by element (a capture may start at
// any sample-aligned address), converted to float and laid into LDS as two planes (re, im; zeros outside the capture); every
// channel of the call works from there: the capture comes from HBM once per call.  Per channel all threads mix the tile once,
// sample by sample, into a second pair of planes (the first mixer's table lies in LDS too; its phase advances by a fixed step
// per thread, so the loop has no division by the table's period).  Then one thread runs the 8 M + 1 taps of one component of one
// output in ascending order -- the real sums in the first T threads, the imaginary ones in the next T: each sum has one owner and
// its stated order.  Samples and taps come from LDS in rounds of 20, a round ahead of the sums.  A block of M samples takes S =
// M | 1 floats of a plane, so that threads whose windows start M samples apart read S floats apart -- an odd stride, every bank
// once.  T is 128 for M = 5 .. 40 and 64 for M = 80: four planes of (T + 8) S floats, the table and the taps are at most
// 127 136 B; at M = 80 more than 126 outputs' worth does not fit the CU's 160 KB whatever the layout (DESIGN.md "PCM front end").
//
// FIR kernel (stage B), as ft8_wide_fir_kernel: a workgroup takes 256 outputs of one frame, stages the 812 plane samples under
// them in LDS, a thread runs its 47 taps in ascending order, rotates by j^p and stores.
// -ffp-contract=off keeps every product and add a single IEEE operation.
#include "pcm.h"
#include "merge_dev.h"

namespace {

constexpr int kPlaneRate = 144000;                          // 9600 sps outputs of 15 s

constexpr int kPlaneThreads = 256;

template <int M, int T>
__global__ __launch_bounds__(kPlaneThreads)
void ft8_pcm_planes_kernel(const void *__restrict__ pcm, int format, int nsamples, int mlast, int row, PcmChannels ch,
                           const PcmTables *__restrict__ tab, float2 *__restrict__ planes) {
    constexpr int S = M | 1;                                // floats per block of M samples
    constexpr int NB = T + 8;                               // blocks under a tile: T - 1 + 8, and the one sample of the next
    constexpr int NREL = M * (T + 7) + 1;                   // samples under a tile
    constexpr int P = 48 * M;                               // the first mixer's period, 16 D
    static_assert(T % 64 == 0 && 2 * T <= kPlaneThreads, "a wave owns one component; both components fit the workgroup");
    __shared__ float raw[2][NB * S];
    __shared__ float mix[2][NB * S];
    __shared__ float2 w1[P];
    __shared__ float vout[2][T];
    __shared__ __attribute__((aligned(16))) float hs[8 * M + 8];   // tap k at 3 + k: tap 1 is 16-byte aligned
    const int tid = threadIdx.x;
    const int part = __builtin_amdgcn_readfirstlane(tid / T);   // 0: the real sums, 1: the imaginary ones, above: none
    const int t = tid - part * T;
    const int capture = blockIdx.y;
    const int m0 = (int)blockIdx.x * T;                     // the tile's first output
    const int n0 = M * (m0 - 4);                            // and first sample (may lie in front of the capture)
    const bool f32 = format & FT8GPU_PCM_F32, cplx = format & FT8GPU_PCM_COMPLEX;
    const int ncomp = cplx ? 2 : 1;
    const size_t first = (size_t)capture * (size_t)nsamples * (size_t)ncomp;    // the capture's first element

    for (int i = tid; i < P; i += kPlaneThreads) w1[i] = tab->w1[row][i];
    for (int i = tid; i < 8 * M + 1; i += kPlaneThreads) hs[3 + i] = tab->hA[row][i];
    // element i: component i & 1 of sample i >> 1 (real: the odd ones are 0).  Every load is unconditional, from a clamped index,
    // so that the loads of an unrolled round are in flight together.
    auto stage = [&](auto *src) {
#pragma unroll 8
        for (int i = tid; i < 2 * NREL; i += kPlaneThreads) {
            const int rel = i >> 1, comp = i & 1;
            const int n = n0 + rel;
            const bool in = n >= 0 && n < nsamples && comp < ncomp;
            const auto v = src[in ? first + (size_t)n * (size_t)ncomp + (size_t)comp : first];
            float a;
            if constexpr (sizeof(v) == sizeof(float)) a = v; else a = (float)v * 0x1p-15f;
            raw[comp][(rel / M) * S + rel % M] = in ? a : 0.0f;                  // x = 0 outside the capture
        }
    };
    if (f32) stage((const float *)pcm); else stage((const int16_t *)pcm);
    __syncthreads();

    const int n0m = ((n0 + tid) % P + P) % P;               // the thread's first sample mod 16 D

#pragma nounroll
    for (int cn = 0; cn < ch.n; ++cn) {
        const int cm = ch.c[cn];
        int k = (n0m * cm) % P;                             // (n c) mod 16 D
        const int step = (kPlaneThreads % P * cm) % P;
        const int m = m0 + tid;
        float2 w2 = make_float2(0.0f, 0.0f);                // the second mixer's entry, fetched under the filter
        if (tid < T && m <= mlast) w2 = tab->w2[((m % FT8GPU_PCM_MIX2) * (int)ch.q[cn]) % FT8GPU_PCM_MIX2];
        int blk = tid / M, r = tid % M;                     // the sample's block and place in it
#pragma unroll 4
        for (int rel = tid; rel < NREL; rel += kPlaneThreads) {   // u[n] = x[n] * w1[(n c) mod 16 D], once per sample
            const int at = blk * S + r;
            blk += kPlaneThreads / M;
            r += kPlaneThreads % M;
            if (r >= M) { r -= M; ++blk; }
            const float xr = raw[0][at], xi = raw[1][at];
            const float2 w = w1[k];
            float ur, ui;
            if (cplx) {
                ur = xr * w.x - xi * w.y;
                ui = xr * w.y + xi * w.x;
            } else {
                ur = xr * w.x;
                ui = xr * w.y;
            }
            mix[0][at] = ur;
            mix[1][at] = ui;
            k += step;
            if (k >= P) k -= P;
        }
        __syncthreads();
        // v[m] = sum over k ascending of hA[k] * u[M m + 4 M - k]: sample M m + 4 M is the first of block t + 8 of the tile
        if (part < 2) {
            // C taps at a time, the samples and taps of the next C loaded from LDS while these are summed
            constexpr int C = 20, NCH = 8 * M / C;               // C is a multiple of M, or M one of C
            static_assert((C % M == 0 || M % C == 0) && NCH % 2 == 0, "a round is whole blocks, or a block whole rounds");
            const float *p = mix[part] + t * S;
            float s = 0.0f;
            s = s + hs[3] * p[8 * S];
            float xa[C], ha[C], xb[C], hb[C];
            auto load = [&](float *x, float *h, int chunk) {                   // taps 1 + chunk C .. C + chunk C
                const float *hh = hs + 4 + chunk * C;
                if constexpr (C % M == 0) {                                    // C / M blocks, from block 7 - chunk C / M down
                    const float *src = p + (7 - chunk * (C / M)) * S + (M - 1);
#pragma unroll
                    for (int i = 0; i < C; ++i) { x[i] = src[-(i / M) * S - i % M]; h[i] = hh[i]; }
                } else {
                    const int b = 7 - chunk / (M / C), c = chunk % (M / C);
                    const float *src = p + b * S + (M - 1 - c * C);
#pragma unroll
                    for (int i = 0; i < C; ++i) { x[i] = src[-i]; h[i] = hh[i]; }
                }
            };
            load(xa, ha, 0);
#pragma nounroll
            for (int chunk = 0; chunk < NCH; chunk += 2) {
                load(xb, hb, chunk + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < C; ++i) s = s + ha[i] * xa[i];
                __builtin_amdgcn_sched_barrier(0);
                if (chunk + 2 < NCH) load(xa, ha, chunk + 2);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < C; ++i) s = s + hb[i] * xb[i];
                __builtin_amdgcn_sched_barrier(0);
            }
            vout[part][t] = s;
        }
        __syncthreads();                                    // the sums are there; the next channel may overwrite the mixed planes
        if (tid < T && m <= mlast) {
            const float sr = vout[0][tid], si = vout[1][tid];
            const float zr = sr * w2.x - si * w2.y, zi = sr * w2.y + si * w2.x;
            planes[((size_t)capture * ch.n + cn) * kPcmPlaneLen + (size_t)m] = make_float2(zr, zi);
        }
    }
}

constexpr int kFirTile = 256;
constexpr int kFirTaps = 47;
constexpr int kFirSpan = 3 * (kFirTile - 1) + kFirTaps;     // 812 plane samples under a tile's outputs
constexpr int kFirGrid = (kNSamples + kFirTile - 1) / kFirTile;

__global__ __launch_bounds__(kFirTile)
void ft8_pcm_fir_kernel(const float2 *__restrict__ planes, int mlast, const PcmTables *__restrict__ tab, float *__restrict__ out) {
    __shared__ float zr[kFirSpan], zi[kFirSpan];
    const int tid = threadIdx.x, frame = blockIdx.y;
    const int p = (int)blockIdx.x * kFirTile + tid;
    const int mb = 3 * (int)blockIdx.x * kFirTile - 23;      // the plane sample staged at index 0
    const float2 *z = planes + (size_t)frame * kPcmPlaneLen;
    for (int i = tid; i < kFirSpan; i += kFirTile) {
        const int m = mb + i;
        const float2 v = (m >= 0 && m <= mlast) ? z[m] : make_float2(0.0f, 0.0f);
        zr[i] = v.x;
        zi[i] = v.y;
    }
    __syncthreads();
    if (p >= kNSamples) return;
    float sr = 0.0f, si = 0.0f;
#pragma unroll
    for (int k = 0; k < kFirTaps; ++k) {                     // y[p] = sum over k ascending of hB[k] * z[3 p + 23 - k]
        const float h = tab->hB[k];
        sr = sr + h * zr[3 * tid + (kFirTaps - 1) - k];
        si = si + h * zi[3 * tid + (kFirTaps - 1) - k];
    }
    float pr, pi;                                           // out[p] = y[p] * j^p; -a is 0 - a: a zero stays +0
    switch (p & 3) {
    case 0: pr = sr; pi = si; break;
    case 1: pr = 0.0f - si; pi = sr; break;
    case 2: pr = 0.0f - sr; pi = 0.0f - si; break;
    default: pr = si; pi = 0.0f - sr; break;
    }
    float *o = out + (size_t)frame * 2 * kNSamples + p;
    o[0] = pr;
    o[kNSamples] = pi;
}

// the peak normalisation of ft8gpu_rx_decimate (rx.hip), one workgroup per frame, as wide.hip has it
__global__ __launch_bounds__(1024)
void ft8_pcm_normalise_kernel(float *__restrict__ iq) {
    __shared__ float s_max[16];
    float4 *f = (float4 *)(iq + (size_t)blockIdx.x * 2 * kNSamples);
    constexpr int n4 = 2 * kNSamples / 4;
    float pk = 0.0f;
    for (int i = threadIdx.x; i < n4; i += 1024) {
        const float4 v = f[i];
        pk = fmaxf(fmaxf(pk, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = pk;
    __syncthreads();
    pk = 0.0f;
    for (int i = 0; i < 16; ++i) pk = fmaxf(pk, s_max[i]);
    float maxSig = 1e-24f;
    if (pk > maxSig) maxSig = pk;
    const float sc = (float)(0.5 / (double)maxSig);
    for (int i = threadIdx.x; i < n4; i += 1024) {
        float4 v = f[i];
        v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
        f[i] = v;
    }
}

// One thread per capture: merge_dev.h's merge over the capture's channels, equal a91 a duplicate only between channels near
// enough to overlap
__global__ __launch_bounds__(64)
void ft8_pcm_merge_kernel(const ft8gpu_message *__restrict__ chan_msgs, const int32_t *__restrict__ chan_n, int ncaptures,
                          PcmChannels ch, ft8gpu_message *msgs, int32_t *__restrict__ n_msgs) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= ncaptures) return;
    merge_parts<true>(chan_msgs, chan_n, c, ch.n, ch.bin, msgs, n_msgs);
}

// the last m whose window holds a sample, M m - 4 M <= nsamples - 1, and at most the rule's last
int last_m(int M, int nsamples) {
    const int m = (nsamples - 1 + 4 * M) / M;
    return m < kPlaneRate - 1 ? m : kPlaneRate - 1;
}

template <int M, int T>
hipError_t planes(const void *pcm, int format, int row, int ncaptures, int nsamples, const PcmChannels &ch, const PcmTables *tab,
                  float2 *out, hipStream_t s) {
    const int mlast = last_m(M, nsamples);
    const unsigned tiles = (unsigned)((mlast + 1 + T - 1) / T);
    ft8_pcm_planes_kernel<M, T><<<dim3(tiles, (unsigned)ncaptures), dim3(kPlaneThreads), 0, s>>>(pcm, format, nsamples, mlast, row, ch, tab, out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pcm_planes(const void *pcm, int format, int D, int ncaptures, int nsamples, const PcmChannels &ch,
                             const PcmTables *tab, float2 *out, hipStream_t s) {
    if (ncaptures < 1) return hipSuccess;
    switch (D) {
    case 15: return planes<5, 128>(pcm, format, 0, ncaptures, nsamples, ch, tab, out, s);
    case 30: return planes<10, 128>(pcm, format, 1, ncaptures, nsamples, ch, tab, out, s);
    case 60: return planes<20, 128>(pcm, format, 2, ncaptures, nsamples, ch, tab, out, s);
    case 120: return planes<40, 128>(pcm, format, 3, ncaptures, nsamples, ch, tab, out, s);
    case 240: return planes<80, 64>(pcm, format, 4, ncaptures, nsamples, ch, tab, out, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_pcm_fir(const float2 *planes, int D, int nsamples, int nframes, const PcmTables *tab, float *out, int normalise,
                          hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    ft8_pcm_fir_kernel<<<dim3(kFirGrid, (unsigned)nframes), dim3(kFirTile), 0, s>>>(planes, last_m(D / 3, nsamples), tab, out);
    if (normalise) ft8_pcm_normalise_kernel<<<dim3((unsigned)nframes), dim3(1024), 0, s>>>(out);
    return hipGetLastError();
}

hipError_t launch_pcm_merge(const ft8gpu_message *chan_msgs, const int32_t *chan_n, int ncaptures, const PcmChannels &ch,
                            ft8gpu_message *msgs, int32_t *n_msgs, hipStream_t s) {
    ft8_pcm_merge_kernel<<<dim3((unsigned)(ncaptures + 63) / 64), dim3(64), 0, s>>>(chan_msgs, chan_n, ncaptures, ch, msgs, n_msgs);
    return hipGetLastError();
}
