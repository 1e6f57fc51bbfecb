/*
 * ft8_hint.c -- the call hints of a receiver, host side (plain C, no GPU; ft8gpu.h "call hints"; csrc/hint.hip has the
 * kernels): reset, insert as the update rule inserts, insert from an a-priori pattern, and the hypothesis of an entry.
 */
#include "../../include/ft8gpu.h"

#include <string.h>

#define FIELD29 0x1FFFFFFFu

void ft8gpu_hint_reset(ft8gpu_hint_state *state) {
    if (state) memset(state, 0, sizeof *state);
}

int ft8gpu_hint_insert(ft8gpu_hint_state *state, int kind, uint32_t a, uint32_t b, int phase) {
    if (!state || kind < 1 || kind > 3) return -1;
    a &= FIELD29;
    b &= FIELD29;
    const uint8_t p = (uint8_t)(phase & 1);
    for (int i = 0; i < FT8GPU_HINT_ENTRIES; ++i) {
        ft8gpu_hint_entry *e = &state->entry[i];
        if (e->used && e->kind == kind && (e->a & FIELD29) == a && (e->b & FIELD29) == b && (e->phase & 1u) == p) {
            e->stamp = state->slot;
            return 0;
        }
    }
    const uint32_t at = state->cursor % FT8GPU_HINT_ENTRIES;
    ft8gpu_hint_entry *e = &state->entry[at];
    e->a = a;
    e->b = b;
    e->stamp = state->slot;
    e->kind = (uint8_t)kind;
    e->used = 1;
    e->phase = p;
    e->pad = 0;
    state->cursor = at + 1;
    return 0;
}

/* payload bits [first, first + 29) of a hypothesis array as a number, MSB first */
static uint32_t field29(const uint8_t bits[10], int first) {
    uint32_t v = 0;
    for (int i = first; i < first + 29; ++i) v = v << 1 | ((bits[i >> 3] >> (7 - (i & 7))) & 1u);
    return v;
}

int ft8gpu_hint_insert_text(ft8gpu_hint_state *state, const char *pattern, int phase) {
    ft8gpu_ap_hypothesis h;
    if (!state || !pattern || ft8gpu_ap_from_text(pattern, &h) != 0) return -1;
    /* a field is known when the pattern masks its first bit: ft8gpu_ap_from_text masks whole fields */
    const int known1 = (h.mask[0] & 0x80u) != 0, known2 = (h.mask[29 >> 3] >> (7 - (29 & 7))) & 1u, known3 = (h.mask[58 >> 3] >> (7 - (58 & 7))) & 1u;
    if (known3 || (!known1 && !known2)) return -1;
    return ft8gpu_hint_insert(state, known1 + 2 * known2, known1 ? field29(h.bits, 0) : 0u, known2 ? field29(h.bits, 29) : 0u, phase);
}

static void put_field(ft8gpu_ap_hypothesis *out, int first, int width, uint32_t value) {
    for (int k = 0; k < width; ++k) {
        const int i = first + k;
        const uint8_t bit = (uint8_t)(0x80u >> (i & 7));
        out->mask[i >> 3] |= bit;
        if ((value >> (width - 1 - k)) & 1u) out->bits[i >> 3] |= bit;
    }
}

int ft8gpu_hint_hypothesis(const ft8gpu_hint_entry *entry, ft8gpu_ap_hypothesis *out) {
    if (!out) return -1;
    memset(out, 0, sizeof *out);
    if (!entry || entry->kind < 1 || entry->kind > 3) return -1;
    if (entry->kind & 1) put_field(out, 0, 29, entry->a & FIELD29);
    if (entry->kind & 2) put_field(out, 29, 29, entry->b & FIELD29);
    put_field(out, 74, 3, 1u);                                     /* i3 = 1 */
    return 0;
}
