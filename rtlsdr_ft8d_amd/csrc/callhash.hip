// callhash.hip -- resolves hashed call signs from a call hash table per receiver (include/ft8gpu.h "hashed call signs",
// DESIGN.md "Call hash table").  The table lives from one 15 s slot to the next, so a receiver is a strictly sequential walk
// over its slots; receivers are independent.  One wave per receiver, lanes = the records of a slot (at most 50 of 64).
//
// A slot, in the order of the rule:
//   parse    every lane takes its record's a91 apart as unpack77 does (unpack_dev.h) into at most two inserts and at most two
//            lookups.  A call that is inserted is printed into the lane's row of LDS (16 bytes = one table entry:
//            unpack_callsign / put_range write at a running position, nothing is indexed in private memory), hashed from
//            there with eleven multiply-adds and one 64-bit multiply, and completed with len and h22.
//   elect    last writer wins, by the rule and not by the order in which stores retire: every insert does an LDS atomicMax
//            of (slot number of this launch + 1) << 7 | (2 * lane + ordinal) on owner[index]; after the barrier exactly
//            the insert whose key is there stores its entry and stamp to the table in HBM.  The tags grow with the slot, so
//            the 16 KB owner array is cleared once per launch, not per slot.
//   hand-off lanes now read entries that OTHER lanes of this wave have just stored to global memory.  That is ordered
//            explicitly: s_waitcnt vmcnt(0) (the stores have left the wave and are acknowledged), then a workgroup-scope
//            acq_rel fence.  Workgroup scope is what one wave on one CU needs: its loads go through the same vector L1 its
//            stores went through (write-through, one per CU), and nothing outside this CU touches the receiver's table
//            during the launch.  The same pair closes the slot, so that the next slot's stores cannot pass this slot's
//            loads.  (DESIGN.md has the argument in full.)
//   resolve  each lookup loads its 16-byte entry and stamp and applies the rule; resolved entries go to the lane's LDS rows.
//   text     the record's text (two 16-byte loads, staged in LDS) is copied into the lane's output row with the k-th
//            "<...>" replaced; the 48-byte record leaves as three 16-byte stores.  All byte indexing is in LDS.
#include "callhash.h"
#include "unpack_dev.h"

namespace {

using namespace ft8dev;

constexpr int kWave = 64;
constexpr int kEntries = FT8GPU_CALLHASH_ENTRIES;
constexpr int kTextIn = 25, kTextOut = 39;             // characters read from ft8gpu_message.text / written at most

struct CallhashLds {
    uint32_t owner[kEntries];      // the winning insert of an index: (slot of the launch + 1) << 7 | key
    uint4    ins[kWave][2];        // the entries a lane inserts
    uint4    hit[kWave][2];        // the entries its hashed fields resolved to, in text order
    uint4    src[kWave][2];        // ft8gpu_message.text and the 7 bytes behind it
    uint4    out[kWave][3];        // the ft8gpu_resolved record
};

// " 0-9A-Z/" -> 0 .. 37
__device__ __forceinline__ uint32_t code38(uint32_t ch) {
    if (ch >= 'A') return ch - 'A' + 11;
    if (ch >= '0') return ch - '0' + 1;
    return ch == '/' ? 37u : 0u;
}

// row: a call of `len` characters, left-justified in blanks.  Completes the entry (len, h22) and returns h22.
__device__ __forceinline__ uint32_t finish_entry(uint4 *row, int len) {
    uint32_t *w = reinterpret_cast<uint32_t *>(row);
    const uint32_t d[3] = { w[0], w[1], w[2] };
    uint64_t n = 0;
#pragma unroll
    for (int i = 0; i < 11; ++i) n = n * 38u + code38((d[i >> 2] >> (8 * (i & 3))) & 0xFFu);
    const uint32_t h22 = (uint32_t)((47055833459ull * n) >> 42);
    w[2] = (d[2] & 0x00FFFFFFu) | ((uint32_t)len << 24);
    w[3] = h22;
    return h22;
}

__device__ __forceinline__ void blank_row(uint4 *row) { *row = make_uint4(0x20202020u, 0x20202020u, 0x20202020u, 0u); }

__global__ __launch_bounds__(kWave)
void ft8_callhash_kernel(const ft8gpu_message *msgs, const int32_t *n_msgs, int ns, ft8gpu_callhash_state *state,
                         uint32_t max_age, ft8gpu_resolved *resolved) {
    __shared__ CallhashLds L;
    const int lane = threadIdx.x;
    ft8gpu_callhash_state *st = state + blockIdx.x;
    uint4 *entries = reinterpret_cast<uint4 *>(st->entry);
    uint32_t *stamps = st->stamp;
    for (int i = lane; i < kEntries / 4; i += kWave) reinterpret_cast<uint4 *>(L.owner)[i] = make_uint4(0, 0, 0, 0);
    uint32_t slot = st->slot;
    __syncthreads();

    for (int s = 0; s < ns; ++s, ++slot) {
        const size_t f = (size_t)blockIdx.x * ns + s;
        int n = n_msgs[f];
        n = n < 0 ? 0 : (n > kMaxMessages ? kMaxMessages : n);
        const bool active = lane < n;
        const uint32_t tag = ((uint32_t)(s + 1) << 7) | (uint32_t)(2 * lane);

        // ---- parse ----
        int nins = 0, nlook = 0;
        uint32_t ins_idx0 = 0, ins_idx1 = 0;           // table index of the inserts
        uint32_t look0 = 0, look1 = 0;                 // lookups: the hash, bit 31 set for a 12-bit one
        if (active) {
            const uint4 *rec = reinterpret_cast<const uint4 *>(msgs + f * kMaxMessages + lane);
            L.src[lane][0] = rec[0];
            L.src[lane][1] = rec[1];
            const uint4 a = rec[3];                    // a91[12], pad[4]
            const uint64_t w0 = (uint64_t)__builtin_bswap32(a.x) << 32 | __builtin_bswap32(a.y);
            const uint64_t w1 = (uint64_t)__builtin_bswap32(a.z) << 32;
            const int i3 = (int)(w1 >> 51) & 7;
            if (i3 == 1 || i3 == 2) {
                const uint32_t n29a = (uint32_t)(w0 >> 35), n29b = (uint32_t)(w0 >> 6) & 0x1FFFFFFFu;
#pragma unroll
                for (int fld = 0; fld < 2; ++fld) {
                    const uint32_t n28 = (fld ? n29b : n29a) >> 1;
                    if (n28 >= NTOKENS + MAX22) {
                        uint4 *row = &L.ins[lane][nins];
                        blank_row(row);
                        char *p = reinterpret_cast<char *>(row);
                        const char *end = unpack_callsign(n28, 0, i3, p);
                        const uint32_t idx = finish_entry(row, end ? (int)(end - p) : 0) >> 10;
                        if (nins == 0) ins_idx0 = idx; else ins_idx1 = idx;
                        ++nins;
                    } else if (n28 >= NTOKENS) {
                        if (nlook == 0) look0 = n28 - NTOKENS; else look1 = n28 - NTOKENS;
                        ++nlook;
                    }
                }
            } else if (i3 == 4) {
                uint64_t n58 = ((w0 & 0x000FFFFFFFFFFFFFull) << 6) | (w1 >> 58);
                const int icq = (int)(w1 >> 54) & 1;
                char c[11];
#pragma unroll
                for (int i = 10; i >= 0; --i) { c[i] = charn((int)(n58 % 38), 5); if (i) n58 /= 38; }
                int lo, hi;
                trim_bounds(c, lo, hi);
                if (hi > lo) {
                    uint4 *row = &L.ins[lane][0];
                    blank_row(row);
                    put_range(reinterpret_cast<char *>(row), c, lo, hi);
                    ins_idx0 = finish_entry(row, hi - lo) >> 10;
                    nins = 1;
                }
                if (!icq) { look0 = 0x80000000u | (uint32_t)(w0 >> 52); nlook = 1; }
            }
        }

        // ---- elect the last writer of every index, then store the winners ----
        if (nins > 0) atomicMax(&L.owner[ins_idx0], tag);
        if (nins > 1) atomicMax(&L.owner[ins_idx1], tag | 1u);
        __syncthreads();
        if (nins > 0 && L.owner[ins_idx0] == tag) { entries[ins_idx0] = L.ins[lane][0]; stamps[ins_idx0] = slot; }
        if (nins > 1 && L.owner[ins_idx1] == (tag | 1u)) { entries[ins_idx1] = L.ins[lane][1]; stamps[ins_idx1] = slot; }

        // ---- hand-off: the stores above are read below by other lanes of this wave ----
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");

        // ---- resolve ----
        // both entries and both stamps are loaded in one round trip (a lane without a lookup reads index 0 and drops it)
        uint32_t mask = 0;
        if (active) {
            const bool h12[2] = { (look0 >> 31) != 0, (look1 >> 31) != 0 };
            const uint32_t h[2] = { look0 & 0x7FFFFFFFu, look1 & 0x7FFFFFFFu };
            const uint32_t idx[2] = { h12[0] ? h[0] : h[0] >> 10, h12[1] ? h[1] : h[1] >> 10 };
            const uint4 e[2] = { entries[idx[0]], entries[idx[1]] };
            const uint32_t age[2] = { slot - stamps[idx[0]], slot - stamps[idx[1]] };
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const bool ok = k < nlook && (e[k].z >> 24) != 0 && !(max_age != 0 && age[k] > max_age) && (h12[k] || e[k].w == h[k]);
                if (ok) { L.hit[lane][k] = e[k]; mask |= 1u << k; }
            }
        }

        // ---- text ----
        if (active) {
            uint4 *orow = L.out[lane];
            orow[0] = orow[1] = orow[2] = make_uint4(0, 0, 0, 0);
            const char *src = reinterpret_cast<const char *>(L.src[lane]);
            char *out = reinterpret_cast<char *>(orow);
            int o = 0, k = 0;
            for (int i = 0; i < kTextIn && o < kTextOut;) {
                const char ch = src[i];
                if (ch == 0) break;
                // a whole "<...>" inside the 25 bytes (the 7 bytes behind the text are staged too, so src[i + 4] is in the row)
                const bool occ = ch == '<' && i + 4 < kTextIn && src[i + 1] == '.' && src[i + 2] == '.' && src[i + 3] == '.' && src[i + 4] == '>';
                if (occ && k < 2 && (mask >> k & 1u)) {
                    const char *call = reinterpret_cast<const char *>(&L.hit[lane][k]);
                    const int len = (uint8_t)call[11] > 11 ? 11 : (uint8_t)call[11];
                    out[o++] = '<';
                    for (int j = 0; j < len && o < kTextOut; ++j) out[o++] = call[j];
                    if (o < kTextOut) out[o++] = '>';
                } else if (occ) {
                    for (int j = 0; j < 5 && o < kTextOut; ++j) out[o++] = src[i + j];
                } else {
                    out[o++] = ch;
                }
                k += occ ? 1 : 0;
                i += occ ? 5 : 1;
            }
            reinterpret_cast<uint32_t *>(orow)[10] = (uint32_t)nlook | (uint32_t)__popc(mask) << 8 | (uint32_t)nins << 16 | mask << 24;
            uint4 *dst = reinterpret_cast<uint4 *>(resolved + f * kMaxMessages + lane);
            dst[0] = orow[0];
            dst[1] = orow[1];
            dst[2] = orow[2];
        }

        // ---- the next slot's stores must not pass this slot's loads ----
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __syncthreads();
    }
    if (lane == 0) st->slot = slot;
}

}  // namespace

hipError_t launch_callhash(const ft8gpu_message *msgs, const int32_t *n_msgs, int nrecv, int ns, ft8gpu_callhash_state *state,
                           uint32_t max_age, ft8gpu_resolved *resolved, hipStream_t s) {
    if (nrecv <= 0 || ns <= 0) return hipSuccess;
    ft8_callhash_kernel<<<dim3((unsigned)nrecv), dim3(kWave), 0, s>>>(msgs, n_msgs, ns, state, max_age, resolved);
    return hipGetLastError();
}
