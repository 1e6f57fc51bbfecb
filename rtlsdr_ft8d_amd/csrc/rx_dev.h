// rx_dev.h -- device helpers shared by the two forms of the RX front end: rx.hip (every capture from reset, one frame
// per capture) and rx_stream.hip (filter state carried from slot to slot).  The arithmetic of rtlsdr_callback()
// (rtlsdr_ft8d.c:76-202) is stated once here: mixer, block sums, row scans, FIR coefficients.
#pragma once
#include "ft8gpu_internal.h"

namespace {

constexpr int kR = 751;                       // input pairs per output sample (DOWNSAMPLING + 1, rtlsdr_ft8d.c:157)
constexpr int kFirTaps = 56;                  // FIR_TAPS, rtlsdr_ft8d.h:40 (57 coefficients)

__constant__ float c_zCoef[kFirTaps + 1] = {  // rtlsdr_ft8d.c:94-110
    -0.0025719973f,  0.0010118403f,  0.0009110571f, -0.0034940765f,
     0.0069713409f, -0.0114242790f,  0.0167023466f, -0.0223683056f,
     0.0276808966f, -0.0316243672f,  0.0329894230f, -0.0305042011f,
     0.0230074504f, -0.0096499429f, -0.0098950502f,  0.0352349632f,
    -0.0650990428f,  0.0972406918f, -0.1284211497f,  0.1544893973f,
    -0.1705667465f,  0.1713383321f, -0.1514501610f,  0.1060148823f,
    -0.0312560926f, -0.0745846391f,  0.2096088743f, -0.3638689868f,
     0.5000000000f,
    -0.3638689868f,  0.2096088743f, -0.0745846391f, -0.0312560926f,
     0.1060148823f, -0.1514501610f,  0.1713383321f, -0.1705667465f,
     0.1544893973f, -0.1284211497f,  0.0972406918f, -0.0650990428f,
     0.0352349632f, -0.0098950502f, -0.0096499429f,  0.0230074504f,
    -0.0305042011f,  0.0329894230f, -0.0316243672f,  0.0276808966f,
    -0.0223683056f,  0.0167023466f, -0.0114242790f,  0.0069713409f,
    -0.0034940765f,  0.0009110571f,  0.0010118403f, -0.0025719973f
};

// Four raw bytes -> four signed samples (x = raw ^ 0x80), with the bytes selected by `neg` (0xFF per
// byte) negated the way an int8 store does it: -(-128) wraps back to -128 (rtlsdr_ft8d.c:134-139).
__device__ __forceinline__ uint32_t mix4(uint32_t raw, uint32_t neg) {
    const uint32_t t = raw ^ (0x80808080u ^ neg);                     // x, or ~x where negated
    return ((t & 0x7F7F7F7Fu) + (neg & 0x01010101u)) ^ (t & 0x80808080u);   // ~x + 1 per selected byte
}

// One group of four I/Q pairs (8 bytes x0..x7, pair index of the first = multiple of 4) with the fs/4 rotation of :129-140:
// I stream = (x0, -x3, -x4, x7), Q stream = (x1, x2, -x5, -x6).  The four bytes of each stream are gathered into one
// dword (v_perm_b32), negated where the rotation says so, and summed with v_dot4_i32_i8 straight into the lane's running
// sums: a = sum of the stream, u = sum of (pair index within the 16-byte unit) * sample.  keep = byte mask of the pairs
// inside the block (byte p = pair p); uw = the group's pair indices as dot weights.
__device__ __forceinline__ void group_sums(uint32_t lo, uint32_t hi, uint32_t keep, int uw, int &aI, int &uI, int &aQ, int &uQ) {
    const int yi = (int)(mix4(__builtin_amdgcn_perm(hi, lo, 0x07040300u), 0x00FFFF00u) & keep);   // (x0, x3, x4, x7), middle two negated
    const int yq = (int)(mix4(__builtin_amdgcn_perm(hi, lo, 0x06050201u), 0xFFFF0000u) & keep);   // (x1, x2, x5, x6), upper two negated
    aI = __builtin_amdgcn_sdot4(yi, 0x01010101, aI, false);
    uI = __builtin_amdgcn_sdot4(yi, uw, uI, false);
    aQ = __builtin_amdgcn_sdot4(yq, 0x01010101, aQ, false);
    uQ = __builtin_amdgcn_sdot4(yq, uw, uQ, false);
}

// byte mask keeping pairs [plo, phi) of a 4-pair group (byte p = pair p)
__device__ __forceinline__ uint32_t pair_mask(int plo, int phi) {
    plo = plo < 0 ? 0 : (plo > 4 ? 4 : plo);
    phi = phi < 0 ? 0 : (phi > 4 ? 4 : phi);
    const uint32_t lo = plo >= 4 ? 0u : (~0u << (8 * plo));
    const uint32_t hi = phi >= 4 ? ~0u : ~(~0u << (8 * phi));
    return lo & hi;
}

// sum over the 16 lanes of a DPP row, result in every lane of the row (wrapping int32)
__device__ __forceinline__ int row_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);   // row_mirror
    return v;
}
// inclusive prefix sum over the 16 lanes of a DPP row (row_shr:n shifts in zeros: bound_ctrl)
__device__ __forceinline__ uint32_t row_scan(uint32_t x) {
    int v = (int)x;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);   // row_shr:8
    return (uint32_t)v;
}

// inclusive scan of a pair of uint32 per thread over a 1024-thread workgroup (wrapping sums; I and Q share the barriers)
__device__ __forceinline__ void block_scan_incl2(uint32_t &a, uint32_t &b, uint32_t (*s_wave)[2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t na = __shfl_up(a, o, 64), nb = __shfl_up(b, o, 64);
        if (lane >= o) { a += na; b += nb; }
    }
    __syncthreads();                                          // the previous scan's readers are done with s_wave
    if (lane == 63) { s_wave[wave][0] = a; s_wave[wave][1] = b; }
    __syncthreads();
    uint32_t oa = 0, ob = 0;
    for (int w = 0; w < wave; ++w) { oa += s_wave[w][0]; ob += s_wave[w][1]; }
    a += oa;
    b += ob;
}

}  // namespace
