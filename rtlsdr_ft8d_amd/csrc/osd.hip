// osd.hip -- ordered-statistics decoding of the candidates belief propagation gives up on (DESIGN.md "Ordered-statistics
// decoding").  Not part of the reference's path: a second chance for a candidate whose status record says ok == 0 and
// ldpc_errors != 0.  The rule is exact (integers and float comparisons), restated in tests/ft8_spec_osd.py:
//   soft bits as the LDPC kernel forms them (ft8_extract_likelihood, ftx_normalize_logl of ft8_lib decode.c, reached
//   through ft8_decode, rtlsdr_ft8d.c:1476); hard decision h, 8-bit weights; positions sorted by |llr| bits descending;
//   the 91 first independent columns of the generator in that order are the basis; reduced echelon form; the patterns
//   c0, c0 ^ R_k, c0 ^ R_i ^ R_j; the one with the smallest (metric, index) is judged: all-zero, hard errors, CRC, unpack77.
//
// One wave64 per candidate, four per workgroup, the launch geometry of the LDPC kernel; the head of the kernel, which leaves a
// candidate that does not qualify as it is, is cand_dev.h's.  Everything else is wave-local:
//   * sort: 174 keys in LDS, every lane counts the keys that precede its three (a rank, no exchange network);
//   * the generator with its COLUMNS in sorted order: lane k fetches the column mask (91 row bits) of the position ranked k,
//     and 91 x 3 ballots turn the column masks into rows -- lane l then holds rows l and 64 + l as three 64-bit words each,
//     in registers, indexed by compile-time constants only (no scratch segment);
//   * elimination walks the sorted columns in order: a ballot finds a row without a pivot that has the bit, six v_readlane
//     broadcast it, every other row with the bit takes the XOR.  It stops at the 91st pivot;
//   * metric of a pattern = sum of weights over its difference from h.  The weights are kept as eight bit planes (ballots),
//     so a metric is 24 and / popcount pairs on 64-bit words instead of 174 table steps;
//   * search: the reduced rows go to LDS by pivot ordinal; order 1 is two rows per lane, order 2 walks i on the scalar side
//     and spreads j over the lanes.  (metric << 13 | index) through one butterfly minimum is the best pattern with the
//     rule's tie break;
//   * the best pattern returns to codeword order through the ranks, and the epilogue is the LDPC kernel's: CRC-14 by
//     linearity, unpack77 on two 64-bit words, the 48-byte record composed in LDS (cand_dev.h, as the soft bits, the
//     judgement, the launch geometry and the kernel that tags the message records OSD gained).
#include "cand_dev.h"

namespace {

struct OsdTables {
    uint32_t col[kLdpcN][4];      // column c of the generator as a row mask: rows 0..31, 32..63, 64..90, 0
    uint16_t crc_bit[77];         // CRC-14 (over 82 bits) of the message whose only set bit is payload bit i
};

__device__ OsdTables d_osd;

constexpr int kRowStride = 7;                          // dwords between reduced rows in LDS (odd: conflict-free per lane)
constexpr int kOffPerm = 192, kOffRows = 384, kOffCw = kOffRows + kLdpcK * kRowStride + 3, kOffRec = kOffCw + 8;
constexpr int kOsdLds = kOffRec + 12;
static_assert(kOffCw % 2 == 0 && kOffRec % 4 == 0, "LDS areas keep their alignment");

__device__ __forceinline__ uint64_t wave_xor64(uint64_t v) {
    return (uint64_t)wave_xor((uint32_t)v) | ((uint64_t)wave_xor((uint32_t)(v >> 32)) << 32);
}
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// a reduced row from LDS (six dwords at an odd stride)
__device__ __forceinline__ void load_row(const uint32_t *rows, int k, uint64_t x[3]) {
    const uint32_t *p = rows + k * kRowStride;
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = (uint64_t)p[2 * j] | ((uint64_t)p[2 * j + 1] << 32);
}

constexpr uint32_t kKeyNone = 0xFFFFFFFFu;
constexpr int kPatShift = 13;                          // 4187 patterns < 2^13; metric <= 174 * 255 < 2^16

__global__ __launch_bounds__(256)
void ft8_osd_kernel(const uint8_t *__restrict__ mag, const ft8gpu_candidate *__restrict__ cands,
                    const int32_t *__restrict__ counts, const ft8gpu_decode_status *status_in,
                    ft8gpu_decode_status *status_out, ft8gpu_osd_info *info, int nframes, int max_candidates,
                    int order, int max_hard_errors, unsigned blocks_per_frame) {
    __shared__ __attribute__((aligned(16))) uint32_t s_mem[4][kOsdLds];

    static_assert(sizeof(ft8gpu_osd_info) == 8, "record sizes");
    const CandWave w = cand_prologue(blockIdx.x, blocks_per_frame, 0u, counts, status_in, status_out, info, nframes, max_candidates);
    if (w.verdict != kCandRun) return;
    const int lane = w.lane, frame = w.frame;
    const size_t rec_index = w.rec_index;
    const uint32_t *in32 = w.in32, mine = w.mine, dw0 = w.dw0;
    uint32_t *out32 = w.out32, *info32 = w.info32;

    uint32_t *s = s_mem[w.wave];
    uint32_t *perm = s + kOffPerm;
    uint32_t *rows = s + kOffRows;

    float cw[3];
    bool has[3];
    if (!soft_bits(mag, frame, cands[rec_index], reinterpret_cast<float *>(s), lane, cw, has)) {      // wave-uniform: nothing is searched
        leave_record(out32, in32, info32, mine, 6u, lane);
        return;
    }

    // ---- order: rank of each position among the keys (|llr| bits descending, ties by ascending position) -----------
    wave_lds_sync();                                                  // every lane has read the raw values
    uint32_t key[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        key[r] = __float_as_uint(cw[r]) & 0x7FFFFFFFu;
        if (has[r]) s[lane + 64 * r] = __float_as_uint(cw[r]);
    }
    wave_lds_sync();
    int rank[3] = { 0, 0, 0 };
    for (int j = 0; j < kLdpcN; ++j) {
        const uint32_t kj = s[j] & 0x7FFFFFFFu;                       // same address in every lane: a broadcast read
#pragma unroll
        for (int r = 0; r < 3; ++r) rank[r] += (kj > key[r] || (kj == key[r] && j < lane + 64 * r)) ? 1 : 0;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
        if (has[r]) perm[rank[r]] = (uint32_t)(lane + 64 * r);
    wave_lds_sync();

    // ---- the sorted view: lane k & 63, slot k >> 6 holds sorted position k -----------------------------------------
    uint64_t Hs[3], P[8][3];                                          // hard decisions and weight planes, wave-uniform
    uint64_t CL[3];                                                   // column masks of the generator: rows 0..63
    uint32_t CH[3];                                                   //                                 rows 64..90
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int k = lane + 64 * q;
        const bool valid = k < kLdpcN;
        const int n = valid ? (int)perm[k] : 0;
        bool hbit;
        int wt;
        hard_and_weight(s[n], valid, hbit, wt);
        Hs[q] = __ballot(hbit);
#pragma unroll
        for (int b = 0; b < 8; ++b) P[b][q] = __ballot((wt >> b) & 1);
        const uint32_t *col = d_osd.col[n];
        CL[q] = valid ? ((uint64_t)col[0] | ((uint64_t)col[1] << 32)) : 0ull;
        CH[q] = valid ? col[2] : 0u;
    }

    // ---- rows from column masks: row r of slot q is the ballot of bit r ----------------------------------------------
    uint64_t R0[3] = { 0ull, 0ull, 0ull }, R1[3] = { 0ull, 0ull, 0ull };   // rows lane and 64 + lane (lanes 0..26)
    for (int r = 0; r < 64; ++r) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const uint64_t bal = __ballot((int)((CL[q] >> r) & 1ull));
            if (lane == r) R0[q] = bal;
        }
    }
    for (int r = 0; r < kLdpcK - 64; ++r) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const uint64_t bal = __ballot((int)((CH[q] >> r) & 1u));
            if (lane == r) R1[q] = bal;
        }
    }

    // ---- elimination over the sorted columns, full reduction; pivot ordinals and pivot columns per row ----------------
    bool used0 = false, used1 = false;
    int ord0 = 0, ord1 = 0, pk0 = 0, pk1 = 0;
    int npiv = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        for (int b = 0; b < 64 && npiv < kLdpcK; ++b) {
            const bool bit0 = ((R0[q] >> b) & 1ull) != 0ull, bit1 = ((R1[q] >> b) & 1ull) != 0ull;
            const uint64_t m0 = __ballot(bit0 && !used0), m1 = __ballot(bit1 && !used1);
            if ((m0 | m1) == 0ull) continue;                          // depends on the pivots so far (or k >= 174: all zero)
            uint64_t piv[3];
            bool me0 = false, me1 = false;
            if (m0 != 0ull) {
                const int p = __builtin_ctzll(m0);
#pragma unroll
                for (int j = 0; j < 3; ++j) piv[j] = readlane64(R0[j], p);
                me0 = lane == p;
            } else {
                const int p = __builtin_ctzll(m1);
#pragma unroll
                for (int j = 0; j < 3; ++j) piv[j] = readlane64(R1[j], p);
                me1 = lane == p;
            }
            if (me0) { used0 = true; ord0 = npiv; pk0 = 64 * q + b; }
            if (me1) { used1 = true; ord1 = npiv; pk1 = 64 * q + b; }
            const bool x0 = bit0 && !me0, x1 = bit1 && !me1;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                R0[j] ^= x0 ? piv[j] : 0ull;
                R1[j] ^= x1 ? piv[j] : 0ull;
            }
            ++npiv;
        }
    }
    // (the generator has rank 91: every row is a pivot row now)

    // ---- reduced rows to LDS by pivot ordinal; c0 = XOR of the rows whose pivot position has h = 1 ---------------------
    const bool has1 = lane < kLdpcK - 64;
    {
        uint32_t *p0 = rows + ord0 * kRowStride;
#pragma unroll
        for (int j = 0; j < 3; ++j) { p0[2 * j] = (uint32_t)R0[j]; p0[2 * j + 1] = (uint32_t)(R0[j] >> 32); }
        if (has1) {
            uint32_t *p1 = rows + ord1 * kRowStride;
#pragma unroll
            for (int j = 0; j < 3; ++j) { p1[2 * j] = (uint32_t)R1[j]; p1[2 * j + 1] = (uint32_t)(R1[j] >> 32); }
        }
    }
    const uint64_t hw0 = pk0 < 64 ? Hs[0] : (pk0 < 128 ? Hs[1] : Hs[2]);
    const uint64_t hw1 = pk1 < 64 ? Hs[0] : (pk1 < 128 ? Hs[1] : Hs[2]);
    const bool inc0 = ((hw0 >> (pk0 & 63)) & 1ull) != 0ull;
    const bool inc1 = has1 && ((hw1 >> (pk1 & 63)) & 1ull) != 0ull;
    uint64_t D[3];                                                    // c0 ^ h: where pattern 0 differs from the hard decision
#pragma unroll
    for (int j = 0; j < 3; ++j) D[j] = wave_xor64((inc0 ? R0[j] : 0ull) ^ (inc1 ? R1[j] : 0ull)) ^ Hs[j];
    wave_lds_sync();

    // ---- search --------------------------------------------------------------------------------------------------------
    uint32_t best = lane == 0 ? (metric_of(D, P) << kPatShift) : kKeyNone;
    if (order >= 1) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int k = lane + 64 * r;
            if (k < kLdpcK) {
                uint64_t x[3];
                load_row(rows, k, x);
#pragma unroll
                for (int j = 0; j < 3; ++j) x[j] ^= D[j];
                best = min(best, (metric_of(x, P) << kPatShift) | (uint32_t)(1 + k));
            }
        }
    }
    if (order >= 2) {
        int base = 1 + kLdpcK;                                        // index of the pair (i, i + 1)
        for (int i = 0; i < kLdpcK - 1; ++i) {
            uint64_t di[3];
            load_row(rows, i, di);                                    // broadcast
#pragma unroll
            for (int j = 0; j < 3; ++j) di[j] ^= D[j];
            for (int jj = i + 1 + lane; jj < kLdpcK; jj += 64) {
                uint64_t x[3];
                load_row(rows, jj, x);
#pragma unroll
                for (int j = 0; j < 3; ++j) x[j] ^= di[j];
                best = min(best, (metric_of(x, P) << kPatShift) | (uint32_t)(base + (jj - i - 1)));
            }
            base += kLdpcK - 1 - i;
        }
    }
    best = wave_min(best);
    const int pattern = (int)(best & ((1u << kPatShift) - 1u));
    const uint32_t metric = best >> kPatShift;

    // ---- the best pattern again, in sorted order, then back to codeword order through the ranks ----------------------
    uint64_t X[3] = { D[0], D[1], D[2] };
    if (pattern >= 1) {                                               // wave-uniform
        int i = pattern - 1, j2 = -1;
        if (pattern > kLdpcK) {
            int q = pattern - 1 - kLdpcK;
            i = 0;
            while (q >= kLdpcK - 1 - i) { q -= kLdpcK - 1 - i; ++i; }
            j2 = i + 1 + q;
        }
        uint64_t x[3];
        load_row(rows, i, x);
#pragma unroll
        for (int j = 0; j < 3; ++j) X[j] ^= x[j];
        if (j2 >= 0) {
            load_row(rows, j2, x);
#pragma unroll
            for (int j = 0; j < 3; ++j) X[j] ^= x[j];
        }
    }
    const int nhard = __popcll(X[0]) + __popcll(X[1]) + __popcll(X[2]);
    uint32_t *cwl = s + kOffCw;
    if (lane < 3) {
        const uint64_t c = lane == 0 ? (X[0] ^ Hs[0]) : (lane == 1 ? (X[1] ^ Hs[1]) : (X[2] ^ Hs[2]));
        cwl[2 * lane] = (uint32_t)c;
        cwl[2 * lane + 1] = (uint32_t)(c >> 32);
    }
    wave_lds_sync();
    bool cbit[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cbit[r] = has[r] && ((cwl[rank[r] >> 5] >> (rank[r] & 31)) & 1u) != 0u;
    const uint64_t B0 = __ballot(cbit[0]), B1 = __ballot(cbit[1]), B2 = __ballot(cbit[2]);

    // ---- judge the best pattern: all-zero, hard errors, CRC, unpack77 -------------------------------------------------
    uint32_t *rec32 = s + kOffRec;
    const int result = judge_word(B0, B1, B2, nhard, max_hard_errors, dw0, d_osd.crc_bit, rec32, lane);
    store_record(out32, in32, rec32, mine, result == 1, lane);
    if (lane == 0) {
        info32[0] = (uint32_t)result | ((uint32_t)nhard << 8) | ((uint32_t)pattern << 16);
        info32[1] = metric;
    }
}

}  // namespace

hipError_t osd_tables_init(hipStream_t s) {
    static OsdTables h;
    for (int c = 0; c < kLdpcN; ++c) {
        uint32_t m[4] = { 0, 0, 0, 0 };
        for (int k = 0; k < kLdpcK; ++k) {
            // row k of the generator: the identity, then parity m covers message bit k when that bit of generator row m is set
            const int bit = c < kLdpcK ? (c == k) : ((kFT8_generator[c - kLdpcK][k >> 3] >> (7 - (k & 7))) & 1);
            if (bit) m[k >> 5] |= 1u << (k & 31);
        }
        for (int j = 0; j < 4; ++j) h.col[c][j] = m[j];
    }
    fill_crc_bits(h.crc_bit);
    return hipMemcpyToSymbolAsync(HIP_SYMBOL(d_osd), &h, sizeof(h), 0, hipMemcpyHostToDevice, s);
}

hipError_t launch_osd(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                      const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, ft8gpu_osd_info *info,
                      int nframes, int max_candidates, int order, int max_hard_errors, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    CandGrid g;
    if (cand_grid(nframes, max_candidates, g) != hipSuccess) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ft8_osd_kernel, dim3(g.nblocks), dim3(256), 0, s, mag, cands, counts, status_in, status_out, info,
                       nframes, max_candidates, order, max_hard_errors, g.bpf);
    return hipGetLastError();
}

hipError_t launch_osd_tag(const ft8gpu_osd_info *info, const int32_t *map, const int32_t *n_before, const int32_t *n_msgs,
                          int nslots, int max_candidates, ft8gpu_message *msgs, hipStream_t s) {
    // pad[0] of the message records OSD gained: the hard errors of the pattern behind them
    return launch_tag(map, n_before, 1, n_msgs, nslots, msgs, TagInfo<0, ft8gpu_osd_info, &ft8gpu_osd_info::nhard>{ info, max_candidates }, s);
}
