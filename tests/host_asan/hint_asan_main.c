/* The host helpers of the call hints (csrc/ft8_hint.c: ft8gpu_hint_reset / _insert / _insert_text / _hypothesis) at the
 * table's edges, as a program of its own for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_hint_cpu.py builds
 * and runs it; nothing is loaded into python).  The states live on the heap with nothing behind them, so a write past entry
 * 511 is a report. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ft8gpu.h"

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("hint_asan: line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

static int popcount_bytes(const uint8_t *p, int n) {
    int c = 0;
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < 8; ++b) c += (p[i] >> b) & 1;
    return c;
}

int main(void) {
    ft8gpu_hint_state *st = malloc(sizeof *st);
    CHECK(st);
    memset(st, 0xA5, sizeof *st);
    ft8gpu_hint_reset(st);
    for (size_t i = 0; i < sizeof *st; ++i) CHECK(((const uint8_t *)st)[i] == 0);
    ft8gpu_hint_reset(NULL);

    /* refusals */
    CHECK(ft8gpu_hint_insert(NULL, 1, 1, 1, 0) == -1 && ft8gpu_hint_insert(st, 0, 1, 1, 0) == -1 && ft8gpu_hint_insert(st, 4, 1, 1, 0) == -1);
    CHECK(ft8gpu_hint_insert(st, -1, 1, 1, 0) == -1 && st->cursor == 0);
    CHECK(ft8gpu_hint_insert_text(st, "? ? ?", 0) == -1 && ft8gpu_hint_insert_text(st, "K1ABC W9XYZ RR73", 0) == -1);
    CHECK(ft8gpu_hint_insert_text(st, "? ? RR73", 0) == -1 && ft8gpu_hint_insert_text(st, "NO SUCH PATTERN AT ALL", 0) == -1);
    CHECK(ft8gpu_hint_insert_text(st, NULL, 0) == -1 && ft8gpu_hint_insert_text(NULL, "K1ABC ? ?", 0) == -1 && st->cursor == 0);

    /* the ring: 512 distinct entries fill it, the 513th overwrites entry 0, the cursor stays in 1..512 */
    for (uint32_t k = 0; k < 513; ++k) {
        st->slot = k;
        CHECK(ft8gpu_hint_insert(st, 1 + (int)(k % 3), 0xE0000000u | (k * 7919u), k, (int)k) == 0);
        CHECK(st->cursor == k % 512 + 1);
    }
    CHECK(st->entry[0].stamp == 512 && st->entry[0].kind == 3 && st->entry[511].stamp == 511 && st->entry[511].kind == 2);
    for (int i = 0; i < FT8GPU_HINT_ENTRIES; ++i)
        CHECK(st->entry[i].used == 1 && st->entry[i].a <= 0x1FFFFFFFu && st->entry[i].phase <= 1 && st->entry[i].pad == 0);

    /* refresh: the same (kind, a, b, phase), whatever lies above bit 28 or bit 0, touches the stamp only */
    st->slot = 0xFFFFFFFFu;
    CHECK(ft8gpu_hint_insert(st, 2, 511u * 7919u, 0x20000000u | 511u, 3) == 0 && st->cursor == 1 && st->entry[511].stamp == 0xFFFFFFFFu);
    CHECK(ft8gpu_hint_insert(st, 2, 511u * 7919u, 511u, 0) == 0 && st->cursor == 2 && st->entry[1].stamp == 0xFFFFFFFFu);   /* another phase: new */
    CHECK(ft8gpu_hint_insert(st, 1, 511u * 7919u, 511u, 1) == 0 && st->cursor == 3);                                        /* another kind: new */

    /* a caller-built state: cursor far past 512, used above 1, garbage above bit 28 and in phase, two equal entries */
    st->cursor = 0xFFFFFFFFu;                      /* % 512 = 511 */
    CHECK(ft8gpu_hint_insert(st, 3, 123456u, 654321u, 0) == 0 && st->cursor == 512 && st->entry[511].kind == 3);
    CHECK(ft8gpu_hint_insert(st, 3, 123457u, 654321u, 0) == 0 && st->cursor == 1 && st->entry[0].stamp == 0xFFFFFFFFu);
    st->entry[7] = st->entry[300];
    st->entry[7].used = 200;
    st->entry[7].a |= 0xE0000000u;
    st->entry[7].phase |= 0xFE;
    st->slot = 77;
    CHECK(ft8gpu_hint_insert(st, st->entry[300].kind, st->entry[300].a, st->entry[300].b, st->entry[300].phase) == 0);
    CHECK(st->entry[7].stamp == 77 && st->entry[7].used == 200 && st->entry[300].stamp != 77 && st->cursor == 1);

    /* text: goes through ft8gpu_ap_from_text; the same pattern refreshes */
    ft8gpu_hint_reset(st);
    CHECK(ft8gpu_hint_insert_text(st, "K1ABC ? ?", 1) == 0 && st->cursor == 1 && st->entry[0].kind == 1 && st->entry[0].b == 0 && st->entry[0].phase == 1);
    st->slot = 3;
    CHECK(ft8gpu_hint_insert_text(st, "K1ABC ? ?", 1) == 0 && st->cursor == 1 && st->entry[0].stamp == 3);
    CHECK(ft8gpu_hint_insert_text(st, "? W9XYZ ?", 0) == 0 && st->cursor == 2 && st->entry[1].kind == 2 && st->entry[1].a == 0);
    CHECK(ft8gpu_hint_insert_text(st, "K1ABC W9XYZ ?", 0) == 0 && st->cursor == 3 && st->entry[2].kind == 3);
    CHECK(st->entry[2].a == st->entry[0].a && st->entry[2].b == st->entry[1].b);

    /* the hypothesis of an entry equals the pattern's */
    ft8gpu_ap_hypothesis *h = malloc(sizeof *h), want;
    CHECK(h);
    static const char *const pattern[3] = { "K1ABC ? ?", "? W9XYZ ?", "K1ABC W9XYZ ?" };
    for (int i = 0; i < 3; ++i) {
        memset(h, 0xA5, sizeof *h);
        CHECK(ft8gpu_hint_hypothesis(&st->entry[i], h) == 0 && ft8gpu_ap_from_text(pattern[i], &want) == 0);
        CHECK(memcmp(h, &want, sizeof want) == 0 && popcount_bytes(h->mask, 10) == (i == 2 ? 61 : 32));
    }
    st->entry[0].kind = 0;
    CHECK(ft8gpu_hint_hypothesis(&st->entry[0], h) == -1 && popcount_bytes(h->mask, 10) == 0);
    st->entry[0].kind = 4;
    CHECK(ft8gpu_hint_hypothesis(&st->entry[0], h) == -1 && ft8gpu_hint_hypothesis(NULL, h) == -1 && ft8gpu_hint_hypothesis(&st->entry[1], NULL) == -1);

    free(h);
    free(st);
    printf("hint_asan ok\n");
    return 0;
}
