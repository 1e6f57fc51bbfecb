/* callhash_asan_main.c -- the host helpers of the call hash table (csrc/ft8_pack.c) under AddressSanitizer and
 * UndefinedBehaviorSanitizer, as a program of its own: reset, hash, insert, lookup at the edges of their arguments (calls of
 * 1 and 11 characters, refused calls, every entry of the table, a slot counter about to wrap, output buffers of exactly the
 * documented size on the heap) and the line formatter with truncating capacities.
 *   gcc -fsanitize=address,undefined -I include tests/host_asan/callhash_asan_main.c rtlsdr_ft8d_amd/csrc/ft8_pack.c */
#include "ft8gpu.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main(void) {
    ft8gpu_callhash_state *st = malloc(sizeof *st);
    CHECK(st);
    memset(st, 0x5A, sizeof *st);
    ft8gpu_callhash_reset(st);
    ft8gpu_callhash_reset(NULL);
    for (size_t i = 0; i < sizeof *st; ++i) CHECK(((const unsigned char *)st)[i] == 0);

    uint32_t h = 0;
    CHECK(ft8gpu_call_hash("K1ABC", 22, &h) == 0 && h == 2920267u);
    CHECK(ft8gpu_call_hash("K1ABC", 12, &h) == 0 && h == 2851u);
    CHECK(ft8gpu_call_hash("PJ4/K1ABC", 22, &h) == 0 && h == 1420834u);
    CHECK(ft8gpu_call_hash("K1ABC", 32, &h) == 0 && ft8gpu_call_hash("K1ABC", 1, &h) == 0 && h <= 1u);
    CHECK(ft8gpu_call_hash("K1ABC", 0, &h) == -1 && ft8gpu_call_hash("K1ABC", 33, &h) == -1 && ft8gpu_call_hash("K1ABC", 22, NULL) == -1);
    static const char *const refused[] = { "", " K1ABC", "K1ABC ", "k1abc", "K1ABC+", "ABCDEFGHIJKL", "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789", NULL };
    for (int i = 0; refused[i]; ++i) CHECK(ft8gpu_call_hash(refused[i], 22, &h) == -1 && ft8gpu_callhash_insert(st, refused[i]) == -1);
    CHECK(ft8gpu_call_hash(NULL, 22, &h) == -1 && ft8gpu_callhash_insert(st, NULL) == -1 && ft8gpu_callhash_insert(NULL, "K1ABC") == -1);

    /* calls of every length, the call in a heap buffer of exactly its size; the answer in a heap buffer of exactly 12 bytes */
    static const char full[] = "VP2E/W1ABCD";
    char *out = malloc(12);
    CHECK(out);
    for (size_t len = 1; len <= 11; ++len) {
        char *call = malloc(len + 1);
        CHECK(call);
        memcpy(call, full, len);
        call[len] = 0;
        if (call[len - 1] == ' ') { free(call); continue; }
        uint32_t h22 = 0, h12 = 0;
        CHECK(ft8gpu_call_hash(call, 22, &h22) == 0 && ft8gpu_call_hash(call, 12, &h12) == 0 && h12 == h22 >> 10);
        st->slot = 0xFFFFFFFFu;                                  /* the counter is about to wrap */
        CHECK(ft8gpu_callhash_insert(st, call) == 0);
        CHECK(st->entry[h12].len == len && st->entry[h12].h22 == h22 && st->stamp[h12] == 0xFFFFFFFFu);
        st->slot = 1u;                                           /* two slots later */
        CHECK(ft8gpu_callhash_lookup(st, 22, h22, 0, out) == 1 && strcmp(out, call) == 0);
        CHECK(ft8gpu_callhash_lookup(st, 12, h12, 2, out) == 1 && strcmp(out, call) == 0);
        CHECK(ft8gpu_callhash_lookup(st, 12, h12, 1, out) == 0 && out[0] == 0);
        CHECK(ft8gpu_callhash_lookup(st, 22, h22 ^ 1u, 0, out) == 0 && out[0] == 0);
        free(call);
    }
    /* every index of the table, both widths; arguments out of range */
    for (uint32_t i = 0; i < FT8GPU_CALLHASH_ENTRIES; ++i) {
        CHECK(ft8gpu_callhash_lookup(st, 12, i, 0, out) >= 0);
        CHECK(ft8gpu_callhash_lookup(st, 22, i << 10 | 1023u, 5, out) >= 0);
    }
    CHECK(ft8gpu_callhash_lookup(st, 12, 4096u, 0, out) == -1 && ft8gpu_callhash_lookup(st, 22, 1u << 22, 0, out) == -1);
    CHECK(ft8gpu_callhash_lookup(st, 10, 1u, 0, out) == -1 && ft8gpu_callhash_lookup(NULL, 12, 1u, 0, out) == -1);
    CHECK(ft8gpu_callhash_lookup(st, 12, 1u, 0, NULL) == -1);
    /* an entry whose len byte is beyond 11 (a state is caller-owned memory) reads as 11 */
    st->entry[7].len = 200;
    memcpy(st->entry[7].call, "ABCDEFGHIJK", 11);
    CHECK(ft8gpu_callhash_lookup(st, 12, 7u, 0, out) == 1 && strcmp(out, "ABCDEFGHIJK") == 0);
    free(out);

    /* the formatter: texts that fill all 40 bytes without a NUL, every capacity from 0 to past the end */
    enum { N = 3 };
    ft8gpu_message *msgs = calloc(N, sizeof *msgs);
    ft8gpu_resolved *res = malloc(N * sizeof *res);
    CHECK(msgs && res);
    memset(res, 'X', N * sizeof *res);
    strcpy(res[1].text, "<VP2E/W1ABCD> <PJ4/K1ABC/P> R FN20");
    msgs[1].snr_db = -30; msgs[1].dt_s = -1.5f; msgs[1].freq_hz = 2999.9f;
    const int need = ft8gpu_format_resolved(msgs, res, N, NULL, 0);
    CHECK(need > 0 && ft8gpu_format_resolved(msgs, res, 0, NULL, 0) == 0 && ft8gpu_format_resolved(NULL, res, 1, NULL, 0) == -1);
    for (int cap = 0; cap <= need + 2; ++cap) {
        char *buf = malloc((size_t)cap + 1);                     /* + 1 so that cap = 0 is a valid allocation; only cap bytes are offered */
        CHECK(buf);
        memset(buf, 0x7F, (size_t)cap + 1);
        CHECK(ft8gpu_format_resolved(msgs, res, N, buf, (size_t)cap) == need);
        CHECK(buf[cap] == 0x7F);
        if (cap > 0) CHECK(strlen(buf) == (size_t)(cap - 1 < need ? cap - 1 : need));
        free(buf);
    }
    char whole[512];
    CHECK(ft8gpu_format_resolved(msgs, res, N, whole, sizeof whole) == need);
    CHECK(strstr(whole, "-30 -1.5 2999 ~  <VP2E/W1ABCD> <PJ4/K1ABC/P> R FN20\n"));
    free(msgs);
    free(res);
    free(st);
    printf("callhash_asan ok\n");
    return 0;
}
