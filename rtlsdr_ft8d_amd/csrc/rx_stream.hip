// rx_stream.hip -- the RX front end of rx.hip on a continuous stream: rtlsdr_callback() (rtlsdr_ft8d.c:76-202) keeps its
// integrators, comb delays, decimationIndex and FIR history in function statics, and the daemon never resets them, so
// every 15 s buffer after the first continues from the state the previous one left.  Here one stream of a call
// (nslots consecutive buffers of npairs pairs) is ONE long capture of T = nslots * npairs pairs that starts from an
// entry state (ft8gpu_rx_state, the reference's statics) and leaves an exit state.
//
// What changes against rx.hip's reduction (same block sums (A, W), same scan, same FIR order):
//   * the decimation grid is shifted by the entry decimationIndex d0: output event e of the call fires after pair
//     751 (e + 1) - d0, block b covers pairs [751 b - d0, 751 (b + 1) - d0) clipped to [0, T).  Pairs outside the clip
//     count as zero SAMPLES, which add nothing to A and W, so every block keeps the length 751 in the recurrence
//         P2_b = P2_{b-1} + 751 * P1_{b-1} + W_b
//     when the scan is seeded with P2 = Ix2 - d0 * Ix1 (the d0 absent pairs of block 0 would each have added Ix1), and
//     the true integrator after a trailing partial block of `rem` pairs is P2_padded - (751 - rem) * P1;
//   * the scan starts from the entry integrators and walks a stream of any length tile by tile with a carry;
//   * the first outputs take their comb delays and FIR history from the entry state.  With X_k the second integrator
//     at event k, the combs are Y_k = X_k - X_{k-2}, y_k = Y_k - Y_{k-2}; the entry state gives X_{-1} = It1y,
//     X_{-2} = It1z, Y_{-1} = It2y, Y_{-2} = It2z, and setting X_{-3} = It1y - It2y, X_{-4} = It1z - It2z makes
//     y_k = (X_k - X_{k-2}) - (X_{k-2} - X_{k-4}) hold for every k >= 0 (ring arithmetic mod 2^32);
//   * an output lands in the slot that holds the pair it fires on, at its index among that slot's events, if that is
//     below 48000; peaks are kept per slot; tail zeroing and normalisation run per slot;
//   * the exit state is written by the device (by the scan workgroup, which is the only reader of `state` after the
//     block kernel: the FIR and finish kernels read a copy of the entry state).
// Byte offsets and pair positions are 64-bit: a stream of a few hundred slots passes 4 GiB.
#include "rx_dev.h"

namespace {

constexpr int kStateWords = (int)(sizeof(ft8gpu_rx_state) / 4);   // 129
constexpr int kEntryStride = 132;                                 // words per entry-state copy (16-byte multiple)
// Partial peaks of a frame and channel: two per 256 stored samples.  The samples [256 j, 256 j + 256) of a slot come from
// at most two consecutive FIR workgroups (their tiles are aligned to the call's events, not to the slot's), which write
// the partials 2 j and 2 j + 1 by the parity of their tile index -- a handful of atomics per address (one atomicMax per
// slot and channel was measured at 0.21 ms for 16 full slots: 750 serialised memory-side atomics per address).
constexpr int kPeakParts = 2 * ((kNSamples + 255) / 256);         // 376
static_assert(sizeof(ft8gpu_rx_state) == 516, "ft8gpu_rx_state is the reference's statics, unpadded");

// second integrator (I, Q) after block k of a stream: group entry state + local running value (rx.hip's fir kernel)
__device__ __forceinline__ void integ2(const int4 *__restrict__ cb, const int4 *__restrict__ cs, int k, uint32_t &pI, uint32_t &pQ) {
    const int4 b = cb[k >> 4], l = cs[k];
    const uint32_t w = (uint32_t)kR * (uint32_t)((k & 15) + 1);
    pI = (uint32_t)b.y + w * (uint32_t)b.x + (uint32_t)l.y;
    pQ = (uint32_t)b.w + w * (uint32_t)b.z + (uint32_t)l.w;
}
// X_k for k in [-4, -1] from the entry state (see the head of the file); st = the state's words
__device__ __forceinline__ void integ2_entry(const uint32_t *st, int k, uint32_t &pI, uint32_t &pQ) {
    // words: 0 Ix1, 1 Ix2, 2 Qx1, 3 Qx2, 4 Iy1, 5 It1y, 6 It1z, 7 Qy1, 8 Qt1y, 9 Qt1z, 10 Iy2, 11 It2y, 12 It2z, 13 Qy2, 14 Qt2y, 15 Qt2z
    const int odd = k & 1;                                   // k = -1, -3: the y delays; k = -2, -4: the z delays
    const uint32_t xI = odd ? st[5] : st[6], xQ = odd ? st[8] : st[9];
    const uint32_t yI = odd ? st[11] : st[12], yQ = odd ? st[14] : st[15];
    pI = k >= -2 ? xI : xI - yI;
    pQ = k >= -2 ? xQ : xQ - yQ;
}

// Block sums of a stream.  rx.hip's block kernel with the grid shifted by d0 and both ends of the stream clipped: the
// six 16-byte loads of a lane are still issued before the first is consumed; a short block (the first, the trailing
// one) has fewer than 80 units, so every unit of a lane is tested against the block's last one.
__global__ __launch_bounds__(256)
void ft8_rxs_block_kernel(const uint8_t *__restrict__ raw, const ft8gpu_rx_state *__restrict__ state, long long T, int nbmax,
                          int4 *__restrict__ sums, int4 *__restrict__ gtot) {
    const int stream = blockIdx.y;
    const int quarter = threadIdx.x >> 4, ql = threadIdx.x & 15;
    const int b = blockIdx.x * 16 + quarter;                 // decimation block of this quarter wave
    const int d0 = (int)state[stream].decimationIndex;
    const int nblocks = (int)((T + d0) / kR) + 1;            // with the trailing partial block (possibly empty)
    const uint8_t *base = raw + (size_t)stream * (size_t)T * 2;
    const long long end_pair = (long long)kR * (b + 1) - d0, first_pair = end_pair - kR;   // nominal
    const long long cfirst = first_pair < 0 ? 0 : first_pair, cend = end_pair > T ? T : end_pair;
    int aI = 0, wI = 0, aQ = 0, wQ = 0;
    if (b < nblocks && cend > cfirst) {
        const long long u0 = (cfirst * 2) >> 4, u1 = (cend * 2 - 1) >> 4;   // 16-byte units touched: u1 - u0 <= 94
        const int nu = (int)(u1 - u0);
        const int rf = (int)(cfirst - 8 * u0), re = (int)(cend - 8 * u0);   // the block's pairs relative to unit u0: [rf, re)
        uint4 v[6];
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int j = min(ql + 16 * t, nu);
            v[t] = *reinterpret_cast<const uint4 *>(base + (size_t)(u0 + j) * 16);
        }
        // W as in rx.hip: weight of a pair = (nominal end of the block) - (its position), whatever the clip
        int uI = 0, uQ = 0, rI = 0, rQ = 0;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int j = ql + 16 * t;
            if (j <= nu) {
                const int n0 = 8 * j;                                            // first pair of the unit, relative
                uint32_t k0 = ~0u, k1 = ~0u;
                if (n0 < rf || n0 + 8 > re) {                                    // boundary unit: clear outsiders
                    k0 = pair_mask(rf - n0, re - n0);
                    k1 = pair_mask(rf - n0 - 4, re - n0 - 4);
                }
                group_sums(v[t].x, v[t].y, k0, 0x03020100, aI, uI, aQ, uQ);
                group_sums(v[t].z, v[t].w, k1, 0x07060504, aI, uI, aQ, uQ);
            }
            rI += aI;
            rQ += aQ;
        }
        const int wb0 = (int)(end_pair - 8 * u0) - 8 * ql;
        wI = (wb0 - 768) * aI + 128 * rI - uI;
        wQ = (wb0 - 768) * aQ + 128 * rQ - uQ;
    }
    aI = row_sum(aI);
    wI = row_sum(wI);
    aQ = row_sum(aQ);
    wQ = row_sum(wQ);
    // local running integrators over the 16 blocks of the workgroup, as in rx.hip (blocks past the stream's last are zero)
    __shared__ int4 s_blk[16];
    if (ql == 0) s_blk[quarter] = make_int4(aI, wI, aQ, wQ);
    __syncthreads();
    if (threadIdx.x < 64) {
        const int4 v = s_blk[threadIdx.x & 15];
        const uint32_t p1I = row_scan((uint32_t)v.x), p1Q = row_scan((uint32_t)v.z);
        const uint32_t p2I = row_scan((uint32_t)kR * (p1I - (uint32_t)v.x) + (uint32_t)v.y);
        const uint32_t p2Q = row_scan((uint32_t)kR * (p1Q - (uint32_t)v.z) + (uint32_t)v.w);
        const int bb = blockIdx.x * 16 + threadIdx.x;
        if (threadIdx.x < 16 && bb < nbmax) {
            const int4 r = make_int4((int)p1I, (int)p2I, (int)p1Q, (int)p2Q);
            sums[(size_t)stream * nbmax + bb] = r;
            if (threadIdx.x == 15 || bb == nbmax - 1) gtot[(size_t)stream * gridDim.x + blockIdx.x] = r;
        }
    }
}

// One workgroup per stream: keeps a copy of the entry state for the kernels that follow, clears the per-slot peaks,
// scans the group totals tile by tile (3072 groups per tile, carry in registers) from the entry integrators into the
// groups' entry states, and writes the exit state.
__global__ __launch_bounds__(1024)
void ft8_rxs_scan_kernel(const int4 *__restrict__ gtot, const int4 *__restrict__ sums, long long T, int nslots, int nbmax, int ngroups,
                         int4 *__restrict__ base, ft8gpu_rx_state *__restrict__ state, uint32_t *__restrict__ entry, uint32_t *__restrict__ peak) {
    __shared__ uint32_t s_wave[16][2];
    __shared__ uint32_t s_st[kStateWords];
    __shared__ uint32_t s_carry[4];
    __shared__ uint32_t s_x[2][64];
    const int stream = blockIdx.x, tid = threadIdx.x;
    uint32_t *stw = reinterpret_cast<uint32_t *>(state + stream);
    if (tid < kStateWords) {
        const uint32_t w = stw[tid];
        s_st[tid] = w;
        entry[(size_t)stream * kEntryStride + tid] = w;
    }
    for (int i = tid; i < 2 * kPeakParts * nslots; i += 1024) peak[(size_t)stream * 2 * kPeakParts * nslots + i] = 0u;
    __syncthreads();
    const uint32_t d0 = s_st[16];
    const int E = (int)((T + d0) / kR), rem = (int)((T + d0) % kR);        // outputs of the call; pairs of the trailing block
    const int4 *s = gtot + (size_t)stream * ngroups;
    int4 *out = base + (size_t)stream * ngroups;
    uint32_t c1I = s_st[0], c2I = s_st[1] - d0 * s_st[0], c1Q = s_st[2], c2Q = s_st[3] - d0 * s_st[2];
    constexpr int kPer = 3;
    for (int tile0 = 0; tile0 < ngroups; tile0 += 1024 * kPer) {
        const int g0 = min(tile0 + tid * kPer, ngroups);
        int4 t[kPer];
        uint32_t w[kPer];                                     // 751 * (blocks in the group)
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int g = g0 + i;
            t[i] = g < ngroups ? s[g] : make_int4(0, 0, 0, 0);
            w[i] = g < ngroups ? (uint32_t)kR * (uint32_t)(min(16 * g + 16, nbmax) - 16 * g) : 0u;
        }
        uint32_t aI = 0, aQ = 0;
#pragma unroll
        for (int i = 0; i < kPer; ++i) { aI += (uint32_t)t[i].x; aQ += (uint32_t)t[i].z; }
        uint32_t p1I = aI, p1Q = aQ;
        block_scan_incl2(p1I, p1Q, s_wave);
        p1I += c1I - aI;                                      // P1base of this thread's first group
        p1Q += c1Q - aQ;
        uint32_t tI = 0, tQ = 0;
        {
            uint32_t qI = p1I, qQ = p1Q;
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                tI += w[i] * qI + (uint32_t)t[i].y;
                tQ += w[i] * qQ + (uint32_t)t[i].w;
                qI += (uint32_t)t[i].x;
                qQ += (uint32_t)t[i].z;
            }
        }
        uint32_t p2I = tI, p2Q = tQ;
        block_scan_incl2(p2I, p2Q, s_wave);
        p2I += c2I - tI;
        p2Q += c2Q - tQ;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            if (g0 + i < ngroups) out[g0 + i] = make_int4((int)p1I, (int)p2I, (int)p1Q, (int)p2Q);
            p2I += w[i] * p1I + (uint32_t)t[i].y;
            p2Q += w[i] * p1Q + (uint32_t)t[i].w;
            p1I += (uint32_t)t[i].x;
            p1Q += (uint32_t)t[i].z;
        }
        if (tid == 1023) { s_carry[0] = p1I; s_carry[1] = p2I; s_carry[2] = p1Q; s_carry[3] = p2Q; }   // state after the tile
        __syncthreads();
        c1I = s_carry[0]; c2I = s_carry[1]; c1Q = s_carry[2]; c2Q = s_carry[3];
    }
    __threadfence_block();
    __syncthreads();                                          // the groups' entry states written above are read below
    // ---- exit state: X_k for k = E - 60 .. E - 1 gives the comb delays, the last comb outputs and the FIR history
    const int4 *cs = sums + (size_t)stream * nbmax;
    if (tid < 64) {
        const int k = E - 60 + tid;
        uint32_t xI = 0u, xQ = 0u;
        if (tid < 60) {
            if (k >= 0) integ2(out, cs, k, xI, xQ);
            else if (k >= -4) integ2_entry(s_st, k, xI, xQ);
        }
        s_x[0][tid] = xI;
        s_x[1][tid] = xQ;
    }
    __syncthreads();
    if (tid >= 4 && tid < 60) {                               // FIR history: comb outputs E - 56 .. E - 1, older ones shift down
        const int k = E - 60 + tid, j = tid - 4;
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            const uint32_t a = s_x[ch][tid], b = s_x[ch][tid - 2], c = s_x[ch][tid - 4];
            const float f = k >= 0 ? (float)(int32_t)((a - b) - (b - c)) : __uint_as_float(s_st[17 + 56 * ch + 56 + k]);
            stw[17 + 56 * ch + j] = __float_as_uint(f);
        }
    }
    if (tid < 2) {                                            // the integer statics of channel tid
        const int ch = tid;
        const int4 b = out[E >> 4], l = cs[E];                // block E: the trailing partial block, padded to 751 pairs
        const uint32_t bx = ch ? (uint32_t)b.z : (uint32_t)b.x, by = ch ? (uint32_t)b.w : (uint32_t)b.y;
        const uint32_t lx = ch ? (uint32_t)l.z : (uint32_t)l.x, ly = ch ? (uint32_t)l.w : (uint32_t)l.y;
        const uint32_t x1 = bx + lx;
        const uint32_t x2 = by + (uint32_t)kR * (uint32_t)((E & 15) + 1) * bx + ly - (uint32_t)(kR - rem) * x1;
        const uint32_t *x = s_x[ch];
        const uint32_t t2y = x[59] - x[57], t2z = x[58] - x[56];
        stw[0 + 2 * ch] = x1;
        stw[1 + 2 * ch] = x2;
        stw[4 + 3 * ch] = E >= 1 ? t2y : s_st[4 + 3 * ch];                   // y1: the last first-comb output
        stw[5 + 3 * ch] = x[59];                                             // t1y
        stw[6 + 3 * ch] = x[58];                                             // t1z
        stw[10 + 3 * ch] = E >= 1 ? t2y - (x[57] - x[55]) : s_st[10 + 3 * ch];   // y2
        stw[11 + 3 * ch] = t2y;
        stw[12 + 3 * ch] = t2z;
        if (ch == 0) stw[16] = (uint32_t)rem;
    }
}

// index of the partial peak of cell key = frame * kPeakParts + part and channel ch in peak[frame][2][kPeakParts]
__device__ __forceinline__ size_t peak_at(int key, int ch) {
    const int frame = key / kPeakParts;
    return ((size_t)frame * 2 + ch) * kPeakParts + (key - frame * kPeakParts);
}

// combs, FIR, scaling and store of 256 consecutive output events of a stream, both channels (rx.hip's fir kernel with
// the entry state in place of zeros).  The partial peaks go through atomicMax on the bit pattern of |sample| (floats
// that are not negative order like their bit patterns).
__global__ __launch_bounds__(256)
void ft8_rxs_fir_kernel(const int4 *__restrict__ sums, const int4 *__restrict__ base, const uint32_t *__restrict__ entry,
                        long long T, long long npairs, int nslots, int nbmax, int ngroups, float *__restrict__ iq, uint32_t *__restrict__ peak) {
    __shared__ uint32_t s_p[2][256 + kFirTaps + 4];
    __shared__ float s_y[2][256 + kFirTaps];
    const int stream = blockIdx.y;
    const uint32_t *st = entry + (size_t)stream * kEntryStride;
    const int d0 = (int)st[16];
    const int E = (int)((T + d0) / kR);
    const int k0 = blockIdx.x * 256;
    if (k0 >= E) return;
    const int4 *cs = sums + (size_t)stream * nbmax, *cb = base + (size_t)stream * ngroups;
    for (int i = threadIdx.x; i < 256 + kFirTaps + 4; i += 256) {
        const int k = k0 - kFirTaps - 4 + i;
        uint32_t pI = 0u, pQ = 0u;
        if (k >= 0) { if (k < E) integ2(cb, cs, k, pI, pQ); }
        else if (k >= -4) integ2_entry(st, k, pI, pQ);
        s_p[0][i] = pI;
        s_p[1][i] = pQ;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256 + kFirTaps; i += 256) {
        const int k = k0 - kFirTaps + i;                     // comb output index
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            const uint32_t a = s_p[ch][i + 4], b = s_p[ch][i + 2], c = s_p[ch][i];
            float y = 0.0f;
            if (k >= 0) { if (k < E) y = (float)(int32_t)((a - b) - (b - c)); }
            else y = __uint_as_float(st[17 + 56 * ch + 56 + k]);              // the entry FIR history
            s_y[ch][i] = y;
        }
    }
    __syncthreads();
    float acc[2] = { 0.0f, 0.0f };
#pragma unroll
    for (int j = 0; j <= kFirTaps; ++j) {                    // :181-192, oldest first
        const float cj = c_zCoef[j];
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) acc[ch] += s_y[ch][threadIdx.x + j] * cj;
    }
    const int e = k0 + threadIdx.x;
    int key = -1;                                            // partial-peak cell (frame, part) of the stored output, or -1
    int frame = 0;
    int idx = 0;
    if (e < E) {
        const unsigned long long pos = (unsigned long long)((long long)kR * (e + 1) - d0 - 1);   // the pair the event fires on
        const unsigned long long slot = pos / (unsigned long long)npairs;
        idx = e - (int)((slot * (unsigned long long)npairs + (unsigned long long)d0) / kR);      // events of earlier slots
        frame = stream * nslots + (int)slot;
        if (idx < kNSamples) key = frame * kPeakParts + 2 * (idx >> 8) + (int)(blockIdx.x & 1);
    }
    float m[2];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const float v = (float)((double)acc[ch] / (32768.0 * 750));
        if (key >= 0) iq[((size_t)frame * 2 + ch) * kNSamples + idx] = v;
        m[ch] = key >= 0 ? fabsf(v) : 0.0f;
    }
    const int first = __builtin_amdgcn_readfirstlane(key);
    if (__all(key == first)) {                               // the whole wave stores into one cell
        if (first >= 0) {
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                for (int o = 32; o > 0; o >>= 1) m[ch] = fmaxf(m[ch], __shfl_xor(m[ch], o, 64));
                if ((threadIdx.x & 63) == 0) atomicMax(&peak[peak_at(first, ch)], __float_as_uint(m[ch]));
            }
        }
    } else if (key >= 0) {
        atomicMax(&peak[peak_at(key, 0)], __float_as_uint(m[0]));
        atomicMax(&peak[peak_at(key, 1)], __float_as_uint(m[1]));
    }
}

// per slot: the stored count, the decoder thread's tail zeroing (:243-246) and, with normalise, its peak normalisation
// to 0.5 (:248-263)
__global__ __launch_bounds__(256)
void ft8_rxs_finish_kernel(float *__restrict__ iq, const uint32_t *__restrict__ peak, const uint32_t *__restrict__ entry,
                           long long npairs, int nslots, int normalise, uint32_t *__restrict__ n_out) {
    const int frame = blockIdx.y, stream = frame / nslots, slot = frame - stream * nslots;
    const uint32_t d0 = entry[(size_t)stream * kEntryStride + 16];
    const unsigned long long ds = ((unsigned long long)slot * (unsigned long long)npairs + d0) % kR;   // decimationIndex at the slot's entry
    const unsigned long long ev = (ds + (unsigned long long)npairs) / kR;
    const int n = ev > (unsigned long long)kNSamples ? kNSamples : (int)ev;
    if (n_out && blockIdx.x == 0 && threadIdx.x == 0) n_out[frame] = (uint32_t)n;
    __shared__ float s_max[4];
    float pk = 0.0f;
    if (normalise) {                                         // uniform: the whole workgroup takes the barrier
        for (int j = threadIdx.x; j < 2 * kPeakParts; j += 256) pk = fmaxf(pk, __uint_as_float(peak[(size_t)frame * 2 * kPeakParts + j]));
        for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
        if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = pk;
        __syncthreads();
        pk = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * kNSamples / 4) return;
    const int k = (i % (kNSamples / 4)) * 4;                 // first sample index of this float4 within its channel
    float4 *f = reinterpret_cast<float4 *>(iq + (size_t)frame * 2 * kNSamples) + i;
    if (!normalise && k + 4 <= n) return;                    // stored samples stay as they are
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (k < n) v = *f;
    float sc = 1.0f;
    if (normalise) {
        float maxSig = 1e-24f;                               // :249
        if (pk > maxSig) maxSig = pk;
        sc = (float)(0.5 / (double)maxSig);                  // :259
        v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
    }
    if (k + 0 >= n) v.x = 0.0f;
    if (k + 1 >= n) v.y = 0.0f;
    if (k + 2 >= n) v.z = 0.0f;
    if (k + 3 >= n) v.w = 0.0f;
    *f = v;
}

}  // namespace

void rx_stream_scratch(int nstreams, int nslots, size_t npairs, size_t *sums_bytes, size_t *p2_bytes) {
    const unsigned long long T = (unsigned long long)nslots * npairs;
    const size_t nbmax = (size_t)((T + 750) / 751) + 1, ngroups = (nbmax + 15) / 16;
    *sums_bytes = (size_t)nstreams * nbmax * 16;
    *p2_bytes = (size_t)nstreams * ngroups * 32 + (size_t)nstreams * kEntryStride * 4 + (size_t)nstreams * nslots * 2 * kPeakParts * 4;
}

// raw: [nstreams][nslots][2*npairs] bytes, state: [nstreams], iq: [nstreams][nslots][2][48000], n_out: [nstreams][nslots] or
// nullptr, all on the device; scratch sized by rx_stream_scratch
hipError_t launch_rx_stream(const uint8_t *raw, int nstreams, int nslots, size_t npairs, ft8gpu_rx_state *state,
                            void *scratch_sums, void *scratch_p2, float *iq, uint32_t *n_out, int normalise, hipStream_t s) {
    if (nstreams < 1 || nslots < 1 || npairs < 8) return hipSuccess;
    const unsigned long long T = (unsigned long long)nslots * npairs;
    const unsigned long long nb = (T + 750) / 751 + 1;       // blocks of a stream with d0 = 750, trailing one included
    if (nb + 16 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const int nbmax = (int)nb, ngroups = (nbmax + 15) / 16, emax = nbmax - 1;
    int4 *base = (int4 *)scratch_p2;
    int4 *gtot = base + (size_t)nstreams * ngroups;
    uint32_t *entry = (uint32_t *)(gtot + (size_t)nstreams * ngroups);
    uint32_t *peak = entry + (size_t)nstreams * kEntryStride;
    hipLaunchKernelGGL(ft8_rxs_block_kernel, dim3(ngroups, nstreams), dim3(256), 0, s,
                       raw, (const ft8gpu_rx_state *)state, (long long)T, nbmax, (int4 *)scratch_sums, gtot);
    hipLaunchKernelGGL(ft8_rxs_scan_kernel, dim3(nstreams), dim3(1024), 0, s,
                       (const int4 *)gtot, (const int4 *)scratch_sums, (long long)T, nslots, nbmax, ngroups, base, state, entry, peak);
    if (emax > 0)
        hipLaunchKernelGGL(ft8_rxs_fir_kernel, dim3((emax + 255) / 256, nstreams), dim3(256), 0, s,
                           (const int4 *)scratch_sums, (const int4 *)base, (const uint32_t *)entry, (long long)T, (long long)npairs,
                           nslots, nbmax, ngroups, iq, peak);
    hipLaunchKernelGGL(ft8_rxs_finish_kernel, dim3((2 * kNSamples / 4 + 255) / 256, nstreams * nslots), dim3(256), 0, s,
                       iq, (const uint32_t *)peak, (const uint32_t *)entry, (long long)npairs, nslots, normalise, n_out);
    return hipGetLastError();
}
