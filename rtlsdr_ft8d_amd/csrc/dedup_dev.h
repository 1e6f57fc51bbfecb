// dedup_dev.h -- the dedup of rtlsdr_ft8d.c:1487-1507 as the wave-per-frame kernels run it (spots.hip, and record_dev.h for
// messages.hip and multipass.hip): staged texts in canonical form, strcmp == 0 as dword equality, and the leader loop that
// numbers the new messages of a chunk of 64 candidates in list order.  Shared so that both output paths keep exactly the
// same messages in the same order.  (wave_lds_sync comes from wave_dev.h.)
#pragma once
#include "ft8gpu_internal.h"
#include "wave_dev.h"

namespace {

constexpr int kTextDw = 7;                    // message_t.text[25] in 7 aligned dwords (bytes 25..27 are 0)

// Staged texts are kept in CANONICAL form: every byte behind the first NUL is zero (what strcmp never looks at), so
// strcmp(a, b) == 0 is equality of the seven dwords -- a dozen instructions instead of a 25-step byte loop, and that
// comparison runs once per (lane, kept message) and once per (lane, unique message of the chunk).  The LDPC kernel
// writes its texts into zero-filled records, but the stage entries also take caller-made records: canonicalising here
// keeps the reference's semantics for any input.
__device__ __forceinline__ void canonical_text(uint32_t (&w)[kTextDw]) {
    bool open = true;                               // no terminator seen yet
#pragma unroll
    for (int k = 0; k < kTextDw; ++k) {
        const uint32_t v = open ? w[k] : 0u;
        const uint32_t z = ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u;   // 0x80 in every zero byte (exact, no carries between bytes)
        const uint32_t low = z & (0u - z);          // the first one: 0x80 << 8 i  (0 if none)
        w[k] = v & ((low >> 7) - 1u);               // bytes below it (all four if none)
        open = open && z == 0u;
    }
}
// strcmp == 0 between the lane's own text (registers) and a staged one
__device__ __forceinline__ bool text_equal(const uint32_t (&mine)[kTextDw], const uint32_t *other) {
    uint32_t d = 0;
#pragma unroll
    for (int k = 0; k < kTextDw; ++k) d |= mine[k] ^ other[k];
    return d == 0u;
}

// :1487-1503 for one chunk -- is the lane's message already known?  First against the `num_decoded` messages kept from
// earlier chunks (thash / ttext).  Then inside the chunk (chash / ctext, staged by every `ok` lane), leader by leader: the
// first lane that is still undecided cannot have an equal message before it (that one would be a leader, and would have
// struck it), so it is NEW; it strikes every later lane carrying its message.  One round per UNIQUE message of the chunk
// (about a dozen) instead of one per decoded candidate (about forty), and a text comparison only where the 16-bit
// hashes agree.  Returns the ballot of the lanes whose message is new, in list order.
__device__ __forceinline__ unsigned long long dedup_chunk(bool ok, uint32_t my_hash, const uint32_t (&mine)[kTextDw], int lane,
                                                          int num_decoded, const uint16_t *thash, const uint32_t (*ttext)[kTextDw],
                                                          const uint16_t *chash, const uint32_t (*ctext)[kTextDw]) {
    bool dup = false;
    for (int t = 0; t < num_decoded; ++t)
        if (ok && thash[t] == my_hash && text_equal(mine, ttext[t])) dup = true;
    unsigned long long pending = __ballot(ok && !dup), fresh = 0ull;
    while (pending != 0ull) {                                             // wave-uniform
        const int j = __builtin_ctzll(pending);
        fresh |= 1ull << j;
        const bool same = ok && !dup && lane > j && chash[j] == my_hash && text_equal(mine, ctext[j]);
        dup = dup || same;
        pending &= ~((1ull << j) | __ballot(same));
    }
    return fresh;
}

}  // namespace
