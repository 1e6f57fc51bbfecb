// wide.hip -- the wideband RX front end (include/ft8gpu.h "wideband RX"): 2.4 Msps unsigned 8-bit I/Q captures -> the 3200 sps
// complex frames of the decoder, one frame per channel of a capture, and the merge of the channels' records of the whole path.
//
// Planes kernel (stage A and the second mixer).  g, the four-fold convolution of a 125-sample boxcar, is a cubic on each of its
// four segments of 125, so v[m] is a fixed integer combination of what four integrators in cascade, started from zero, hold
// after each of the four 125-sample blocks under its window (block b = samples 125 b - 1 .. 125 b + 123): the CIC recursion, cut
// into blocks.  With N = M - 1, M the 4 x 4 matrix that carries the integrators over 125 samples without input, the fourth
// difference of the decimated fourth integrator is
//     v[m] = e4' ( I[m+1] + (N - 3) I[m] + (3 - 2N + N^2) I[m-1] + (-1 + N - N^2 + N^3) I[m-2] ),
// the state before block m-2 dropping out because N^4 = 0; the rows e4'(...) are the constants kA below.  A lane takes one block:
// 125 complex products with the first mixer, the first integrator in int32 (below 2^30), the other three in int64.  A wave takes
// 64 consecutive blocks, which give 61 outputs (three 64-bit lane shifts per component), so consecutive waves overlap by three
// blocks.  The wave's 16 000 bytes are fetched once, 16 bytes per lane and load, into its own part of LDS (raw ^ 0x80, zeros
// outside the capture), and every channel of the call reads them from there: the capture comes from HBM once per call.  The first
// mixer's table lies in LDS too (24 KB of int16 pairs); the second one is read once per output from the table in memory.  Eight
// waves and 152 KB of LDS per workgroup, one workgroup per CU.  The kernel is bound by its integer arithmetic, about 30 VALU
// operations per sample and channel, not by the bytes.
//
// FIR kernel (stage B).  A workgroup takes 256 outputs of one frame: the 1625 plane samples under them are staged in LDS as two
// float planes, a thread runs its 95 taps in ascending order (the taps are uniform: scalar loads), rotates by j^p and stores.
// -ffp-contract=off keeps every product and add a single IEEE operation.
#include "wide.h"
#include "merge_dev.h"

namespace {

constexpr int kR1 = 125;                                    // first decimation
constexpr int kVPerTile = 61;                               // outputs of a wave's 64 blocks
constexpr int kWaves = 8;
constexpr int kTilesPerWave = 2;
constexpr int kStageUnits = 1001;                           // 16-byte units that cover 16 000 bytes at any alignment
constexpr int kStageBytes = 16 * kStageUnits;
static_assert(64 * 2 * kR1 + 14 <= kStageBytes, "a wave's blocks fit its stage at every offset");
constexpr float kC0 = (float)(1.0 / (32767.0 * 244140625.0 * 128.0));

// e4' A_s, s = 0 .. 3 (block m + 1 - s), over the integrators 1 .. 4
constexpr long long kA[4][4] = { { 0, 0, 0, 1 }, { 333375, 7875, 125, -3 }, { 1302000, -125, -250, 3 }, { 317750, -7750, 125, -1 } };

__device__ inline long long combine(int s, long long i1, long long i2, long long i3, long long i4) {
    return kA[s][0] * i1 + kA[s][1] * i2 + kA[s][2] * i3 + kA[s][3] * i4;
}

__global__ __launch_bounds__(64 * kWaves)
void ft8_wide_planes_kernel(const uint8_t *__restrict__ raw, int capture_bytes, int mlast, int ntiles, WideChannels ch,
                            const WideTables *__restrict__ tab, float2 *__restrict__ planes) {
    __shared__ __attribute__((aligned(16))) uint32_t w1[FT8GPU_WIDE_MIX1];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][kStageBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int capture = blockIdx.y;
    const uint8_t *base = raw + (size_t)capture * (size_t)capture_bytes;
    for (int i = tid; i < FT8GPU_WIDE_MIX1; i += 64 * kWaves) w1[i] = ((const uint32_t *)tab->w1)[i];

#pragma nounroll
    for (int it = 0; it < kTilesPerWave; ++it) {
        const int tile = ((int)blockIdx.x * kTilesPerWave + it) * kWaves + wave;
        const int m0 = kVPerTile * tile - 1;                 // the wave's first output
        const int b0 = m0 - 2;                               // and first block
        const int first = 2 * (kR1 * b0 - 1);                // the byte of its first sample (may lie in front of the capture)
        const int aligned = (first >> 4) * 16;               // floor to a 16-byte unit
        __syncthreads();                                     // the table is there; the stage's readers of the last round are done
        if (tile < ntiles) {
            for (int j = lane; j < kStageUnits; j += 64) {
                const int at = aligned + 16 * j;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);        // x = 0 outside the capture
                if (at >= 0 && at + 16 <= capture_bytes) {   // (a unit lies wholly inside or outside: npairs is a multiple of 8)
                    v = *(const uint4 *)(base + at);
                    v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
                }
                *(uint4 *)(stage[wave] + 16 * j) = v;
            }
        }
        __syncthreads();
        if (tile >= ntiles) continue;                        // (uniform per wave)
        const uint16_t *sp = (const uint16_t *)(stage[wave] + (first - aligned) + 2 * kR1 * lane);
        const int n0 = kR1 * (b0 + lane) - 1;                // the lane's first sample
        const int n0m = (n0 % FT8GPU_WIDE_MIX1 + FT8GPU_WIDE_MIX1) % FT8GPU_WIDE_MIX1;
        const int m = m0 + lane;

#pragma nounroll
        for (int cn = 0; cn < ch.n; ++cn) {
            const int cm = ch.c[cn];
            int k = (n0m * cm) % FT8GPU_WIDE_MIX1;           // (n c) mod 6000
            int s1r = 0, s1i = 0;
            long long s2r = 0, s2i = 0, s3r = 0, s3i = 0, s4r = 0, s4i = 0;
#pragma unroll 5
            for (int i = 0; i < kR1; ++i) {
                const uint32_t t = sp[i];
                const int xr = (int8_t)(t & 0xffu), xi = (int8_t)(t >> 8);
                const uint32_t w = w1[k];
                const int wr = (int16_t)(w & 0xffffu), wi = (int32_t)w >> 16;
                s1r += xr * wr - xi * wi;
                s1i += xr * wi + xi * wr;
                s2r += s1r; s2i += s1i;
                s3r += s2r; s3i += s2i;
                s4r += s3r; s4i += s3i;
                k += cm;
                if (k >= FT8GPU_WIDE_MIX1) k -= FT8GPU_WIDE_MIX1;
            }
            // v[m] = (block m-2: this lane) + (m-1: lane + 1) + (m: lane + 2) + (m+1: lane + 3)
            long long vr = combine(3, s1r, s2r, s3r, s4r), vi = combine(3, s1i, s2i, s3i, s4i);
            vr += __shfl_down(combine(2, s1r, s2r, s3r, s4r), 1, 64);
            vi += __shfl_down(combine(2, s1i, s2i, s3i, s4i), 1, 64);
            vr += __shfl_down(combine(1, s1r, s2r, s3r, s4r), 2, 64);
            vi += __shfl_down(combine(1, s1i, s2i, s3i, s4i), 2, 64);
            vr += __shfl_down(s4r, 3, 64);
            vi += __shfl_down(s4i, 3, 64);
            if (lane < kVPerTile && m <= mlast) {
                const float fr = (float)vr * kC0, fi = (float)vi * kC0;
                const int mm = (m + FT8GPU_WIDE_MIX2) % FT8GPU_WIDE_MIX2;        // m >= -1
                const float2 w = tab->w2[(mm * (int)ch.q[cn]) % FT8GPU_WIDE_MIX2];
                const float zr = fr * w.x - fi * w.y, zi = fr * w.y + fi * w.x;
                planes[((size_t)capture * ch.n + cn) * kWidePlaneLen + (size_t)(kWidePlanePad + m)] = make_float2(zr, zi);
            }
        }
    }
}

constexpr int kFirTile = 256;
constexpr int kFirTaps = 95;
constexpr int kFirSpan = 6 * (kFirTile - 1) + kFirTaps;     // 1625 plane samples under a tile's outputs
constexpr int kFirGrid = (kNSamples + kFirTile - 1) / kFirTile;

__global__ __launch_bounds__(kFirTile)
void ft8_wide_fir_kernel(const float2 *__restrict__ planes, int mlast, const WideTables *__restrict__ tab, float *__restrict__ out) {
    __shared__ float zr[kFirSpan], zi[kFirSpan];
    const int tid = threadIdx.x, frame = blockIdx.y;
    const int p = (int)blockIdx.x * kFirTile + tid;
    const int mb = 6 * (int)blockIdx.x * kFirTile - 47;      // the plane sample staged at index 0
    const float2 *z = planes + (size_t)frame * kWidePlaneLen + kWidePlanePad;
    for (int i = tid; i < kFirSpan; i += kFirTile) {
        const int m = mb + i;
        const float2 v = (m >= -1 && m <= mlast) ? z[m] : make_float2(0.0f, 0.0f);
        zr[i] = v.x;
        zi[i] = v.y;
    }
    __syncthreads();
    if (p >= kNSamples) return;
    float sr = 0.0f, si = 0.0f;
#pragma unroll 5
    for (int k = 0; k < kFirTaps; ++k) {                     // y[p] = sum over k ascending of h[k] * z[6 p + 47 - k]
        const float h = tab->h[k];
        sr = sr + h * zr[6 * tid + (kFirTaps - 1) - k];
        si = si + h * zi[6 * tid + (kFirTaps - 1) - k];
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

// the peak normalisation of ft8gpu_rx_decimate (rx.hip), one workgroup per frame
__global__ __launch_bounds__(1024)
void ft8_wide_normalise_kernel(float *__restrict__ iq) {
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

// One thread per capture: merge_dev.h's merge over the capture's channels; channels may lie anywhere in the capture, so equal
// a91 is a duplicate only between channels near enough to overlap
__global__ __launch_bounds__(64)
void ft8_wide_merge_kernel(const ft8gpu_message *__restrict__ chan_msgs, const int32_t *__restrict__ chan_n, int ncaptures,
                           WideChannels ch, ft8gpu_message *msgs, int32_t *__restrict__ n_msgs) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= ncaptures) return;
    merge_parts<true>(chan_msgs, chan_n, c, ch.n, ch.bin, msgs, n_msgs);
}

int last_m(size_t npairs) { return (int)((npairs - 1 + 248) / kR1); }

}  // namespace

hipError_t launch_wide_planes(const uint8_t *raw, int ncaptures, size_t npairs, const WideChannels &ch, const WideTables *tab,
                              float2 *planes, hipStream_t s) {
    if (ncaptures < 1) return hipSuccess;
    const int mlast = last_m(npairs);
    const int ntiles = (mlast + 2 + kVPerTile - 1) / kVPerTile;                  // outputs m = -1 .. mlast
    const unsigned groups = (unsigned)((ntiles + kWaves * kTilesPerWave - 1) / (kWaves * kTilesPerWave));
    ft8_wide_planes_kernel<<<dim3(groups, (unsigned)ncaptures), dim3(64 * kWaves), 0, s>>>(raw, (int)(2 * npairs), mlast, ntiles, ch, tab, planes);
    return hipGetLastError();
}

hipError_t launch_wide_fir(const float2 *planes, size_t npairs, int nframes, const WideTables *tab, float *out, int normalise,
                           hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    ft8_wide_fir_kernel<<<dim3(kFirGrid, (unsigned)nframes), dim3(kFirTile), 0, s>>>(planes, last_m(npairs), tab, out);
    if (normalise) ft8_wide_normalise_kernel<<<dim3((unsigned)nframes), dim3(1024), 0, s>>>(out);
    return hipGetLastError();
}

hipError_t launch_wide_merge(const ft8gpu_message *chan_msgs, const int32_t *chan_n, int ncaptures, const WideChannels &ch,
                             ft8gpu_message *msgs, int32_t *n_msgs, hipStream_t s) {
    ft8_wide_merge_kernel<<<dim3((unsigned)(ncaptures + 63) / 64), dim3(64), 0, s>>>(chan_msgs, chan_n, ncaptures, ch, msgs, n_msgs);
    return hipGetLastError();
}
