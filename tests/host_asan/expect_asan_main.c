/* The host helpers of the expected-messages table (csrc/ft8_pack.c: ft8gpu_expect_reset / _insert / _insert_text) at the
 * table's edges, as a program of its own for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_match_cpu.py builds
 * and runs it; nothing is loaded into python).  The states live on the heap with nothing behind them, so a write past entry
 * 511 or a read past payload[9] is a report. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ft8gpu.h"

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("expect_asan: line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

static void payload_of(uint32_t k, uint8_t p[10]) {
    for (int i = 0; i < 10; ++i) p[i] = (uint8_t)((k * 2654435761u) >> (3 * i)) ^ (uint8_t)(17 * i);
    p[0] = (uint8_t)k;
    p[1] = (uint8_t)(k >> 8);
}

int main(void) {
    ft8gpu_expect_state *st = malloc(sizeof *st);
    CHECK(st);
    memset(st, 0xA5, sizeof *st);
    ft8gpu_expect_reset(st);
    for (size_t i = 0; i < sizeof *st; ++i) CHECK(((const uint8_t *)st)[i] == 0);
    ft8gpu_expect_reset(NULL);

    /* refusals */
    uint8_t *p = malloc(10);                       /* exactly ten bytes: nothing behind payload[9] may be read */
    CHECK(p);
    payload_of(1, p);
    CHECK(ft8gpu_expect_insert(NULL, p, 0) == -1 && ft8gpu_expect_insert(st, NULL, 0) == -1);
    CHECK(ft8gpu_expect_insert(st, p, 2) == -1 && ft8gpu_expect_insert(st, p, -1) == -1);
    CHECK(ft8gpu_expect_insert_text(st, "THIS IS NO FT8 MESSAGE AT ALL") == -1 && ft8gpu_expect_insert_text(st, NULL) == -1);
    CHECK(ft8gpu_expect_insert_text(NULL, "CQ K1ABC FN42") == -1 && st->cursor == 0);

    /* the ring: 512 distinct payloads fill it, the 513th overwrites entry 0, the cursor stays in 1..512 */
    for (uint32_t k = 0; k < 513; ++k) {
        payload_of(k, p);
        st->slot = k;
        CHECK(ft8gpu_expect_insert(st, p, (int)(k & 1)) == 0);
        CHECK(st->cursor == k % 512 + 1);
    }
    CHECK(st->entry[0].stamp == 512 && st->entry[0].kind == 0 && st->entry[511].stamp == 511 && st->entry[511].kind == 1);
    for (int i = 0; i < FT8GPU_EXPECT_ENTRIES; ++i) CHECK(st->entry[i].used == 1 && (st->entry[i].payload[9] & 7) == 0);

    /* refresh: the same 77 bits, whatever bits 77..79 say, touch stamp and kind only; derived over heard stays heard */
    payload_of(511, p);
    p[9] |= 7;
    st->slot = 0xFFFFFFFFu;
    CHECK(ft8gpu_expect_insert(st, p, 0) == 0 && st->cursor == 1 && st->entry[511].stamp == 0xFFFFFFFFu && st->entry[511].kind == 0);
    CHECK(ft8gpu_expect_insert(st, p, 1) == 0 && st->entry[511].kind == 0);

    /* a caller-built state: cursor far past 512, used above 1, garbage behind bit 76 of a stored payload, two equal entries */
    st->cursor = 0xFFFFFFFFu;                      /* % 512 = 511 */
    payload_of(9000, p);
    CHECK(ft8gpu_expect_insert(st, p, 1) == 0 && st->cursor == 512 && st->entry[511].kind == 1);
    payload_of(9001, p);
    CHECK(ft8gpu_expect_insert(st, p, 0) == 0 && st->cursor == 1 && st->entry[0].stamp == 0xFFFFFFFFu);
    st->entry[7] = st->entry[300];
    st->entry[7].used = 200;
    st->entry[7].payload[9] |= 5;
    st->slot = 77;
    memcpy(p, st->entry[300].payload, 10);
    CHECK(ft8gpu_expect_insert(st, p, 0) == 0 && st->entry[7].stamp == 77 && st->entry[7].used == 200 && st->entry[300].stamp != 77);

    /* text: goes through the packer, equal text refreshes */
    ft8gpu_expect_reset(st);
    CHECK(ft8gpu_expect_insert_text(st, "K1ABC W9XYZ RR73") == 0 && st->cursor == 1);
    st->slot = 3;
    CHECK(ft8gpu_expect_insert_text(st, "K1ABC W9XYZ RR73") == 0 && st->cursor == 1 && st->entry[0].stamp == 3);
    CHECK(ft8gpu_expect_insert_text(st, "CQ K1ABC FN42") == 0 && st->cursor == 2);
    uint8_t q[10];
    CHECK(ft8gpu_pack77("CQ K1ABC FN42", q) == 0 && memcmp(q, st->entry[1].payload, 10) == 0);

    free(p);
    free(st);
    printf("expect_asan ok\n");
    return 0;
}
