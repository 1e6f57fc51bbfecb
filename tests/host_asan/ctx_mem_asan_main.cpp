// AddressSanitizer + UBSan run of csrc/ctx_mem.h -- the owner of a context's device and pinned host memory.  The header has no
// HIP in it, so this file is the real class under g++ -fsanitize=address,undefined, on a counting fake backend (malloc / free
// underneath, so a double free or a block freed by the wrong function is the sanitizer's or this file's to catch) that can refuse
// the k-th allocation or the upload.
//
// One script stands for a context's life: several once(), a table(), a grow() up and up again, a pair() and a pair_kept() grown
// twice each, a pinned block.  For every k up to the script's number of allocations the k-th is refused: the step must fail by
// the owner's rule (fields null, cap 0 -- pair_kept: everything as before --, the runtime's error cleared once, nothing recorded),
// the same step repeated without the fault must succeed, and at the end release_all() frees every live block exactly once.
#include "ctx_mem.h"

#include <functional>
#include <set>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>

static char g_err[512];
int ft8_fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return -1;
}

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) { printf("ctx_mem_asan: line %d: %s (k = %d, error \"%s\")\n", __LINE__, #cond, g_k, g_err); exit(1); } \
    } while (0)

static int g_k = 0;                       // the allocation being refused (0: none), for the messages
static std::set<void *> g_dev, g_host;    // live blocks
static int g_allocs = 0, g_fail_at = 0, g_frees = 0, g_cleared = 0, g_uploads = 0;
static bool g_fail_upload = false;

static void *fake_alloc(std::set<void *> &live, size_t bytes) {
    if (++g_allocs == g_fail_at) return nullptr;
    void *p = malloc(bytes ? bytes : 1);
    memset(p, 0xA5, bytes);
    live.insert(p);
    return p;
}
static void fake_free(std::set<void *> &live, void *p) {
    if (live.erase(p) != 1) { printf("ctx_mem_asan: a block that is not live (or of the other kind) was freed\n"); exit(1); }
    ++g_frees;
    free(p);
}
static const MemBackend kFake = {
    [](size_t n) { return fake_alloc(g_dev, n); },  [](void *p) { fake_free(g_dev, p); },
    [](size_t n) { return fake_alloc(g_host, n); }, [](void *p) { fake_free(g_host, p); },
    [](void *dst, const void *src, size_t n) {
        ++g_uploads;
        if (g_fail_upload) return -1;
        if (!g_dev.count(dst)) { printf("ctx_mem_asan: upload to a block that is not live\n"); exit(1); }
        memcpy(dst, src, n);
        return 0;
    },
    []() -> const char * { ++g_cleared; return "fake refusal"; },
};

struct Table { int v[64]; };
struct RecA { char b[24]; };
struct RecB { char b[5]; };

// what a context keeps: named fields and their caps
struct Fields {
    float *a = nullptr;
    unsigned char *b = nullptr;
    Table *tab = nullptr;
    void *g = nullptr;
    size_t g_cap = 0;
    RecA *pa = nullptr;
    RecB *pb = nullptr;
    int p_cap = 0;
    RecA *ka = nullptr;
    RecB *kb = nullptr;
    int k_cap = 0;
    int *pinned = nullptr;
};

struct Step {
    const char *what;
    std::function<int()> run;
    std::function<bool()> cleared;        // after a failure: the step's fields are null and its cap 0
    bool kept;                            // pair_kept: a failure changes nothing
};

static int fill_table(Table *t) {
    for (int i = 0; i < 64; ++i) { if (t->v[i] != 0) return ft8_fail("the host table was not zeroed"); t->v[i] = 3 * i + 1; }
    return 0;
}

// the script on one context; k: the allocation to refuse (0: none).  Returns the number of allocations a clean run makes.
static int run_script(int k) {
    g_k = k;
    g_allocs = g_frees = g_cleared = g_uploads = 0;
    g_fail_at = k;
    g_err[0] = 0;
    Fields f;
    CtxMem m(&kFake);
    const size_t frames = 4;
    const Step steps[] = {
        { "once a", [&] { return m.once(&f.a, 100, "buffer a"); }, [&] { return !f.a; }, false },
        { "once b", [&] { return m.once(&f.b, 200, "buffer b"); }, [&] { return !f.b; }, false },
        { "once a again", [&] { return m.once(&f.a, 100, "buffer a"); }, [&] { return false; }, false },     // allocates nothing
        { "table", [&] { return m.table(&f.tab, "the table", fill_table); }, [&] { return !f.tab; }, false },
        { "grow to 64", [&] { return m.grow(&f.g, &f.g_cap, 64, "scratch"); }, [&] { return !f.g && f.g_cap == 0; }, false },
        { "grow to 128", [&] { return m.grow(&f.g, &f.g_cap, 128, "scratch"); }, [&] { return !f.g && f.g_cap == 0; }, false },
        { "grow to 32", [&] { return m.grow(&f.g, &f.g_cap, 32, "scratch"); }, [&] { return false; }, false },
        { "pair at 120", [&] { return m.pair(&f.pa, &f.pb, &f.p_cap, 120, frames, "the pair"); }, [&] { return !f.pa && !f.pb && f.p_cap == 0; }, false },
        { "pair at 200", [&] { return m.pair(&f.pa, &f.pb, &f.p_cap, 200, frames, "the pair"); }, [&] { return !f.pa && !f.pb && f.p_cap == 0; }, false },
        { "pair at 150", [&] { return m.pair(&f.pa, &f.pb, &f.p_cap, 150, frames, "the pair"); }, [&] { return false; }, false },
        { "kept pair at 120", [&] { return m.pair_kept(&f.ka, &f.kb, &f.k_cap, 120, frames, "the kept pair"); }, [&] { return false; }, true },
        { "kept pair at 300", [&] { return m.pair_kept(&f.ka, &f.kb, &f.k_cap, 300, frames, "the kept pair"); }, [&] { return false; }, true },
        { "pinned", [&] { return m.once_pinned(&f.pinned, sizeof(int), "the pinned count"); }, [&] { return !f.pinned; }, false },
    };
    bool failed = false;
    for (const Step &s : steps) {
        const Fields before = f;
        const size_t live_before = m.live(), blocks_before = g_dev.size() + g_host.size();
        const int allocs_before = g_allocs, cleared_before = g_cleared;
        int rc = s.run();
        if (k && allocs_before < k && g_allocs >= k) {              // this step met the refusal
            CHECK(rc == -1);
            CHECK(!failed);
            failed = true;
            CHECK(g_cleared == cleared_before + 1);                  // the runtime's last error was cleared
            CHECK(strstr(g_err, "fake refusal") && strstr(g_err, "out of ") && strstr(g_err, " bytes)"));
            if (s.kept) {
                CHECK(memcmp(&before, &f, sizeof f) == 0);           // old blocks, old cap
                CHECK(m.live() == live_before && g_dev.size() + g_host.size() == blocks_before);
            } else {
                CHECK(s.cleared());
                CHECK(m.live() <= live_before);                      // nothing was recorded (grow and pair let the old block go)
            }
            CHECK(m.live() == g_dev.size() + g_host.size());         // and nothing is live that is not recorded
            g_fail_at = 0;
            rc = s.run();                                            // the same call, the fault removed
        }
        CHECK(rc == 0);
        CHECK(g_cleared == (failed ? 1 : 0));                        // cleared for the refusal, and only for it
        CHECK(m.live() == g_dev.size() + g_host.size());
    }
    CHECK(!k || failed);
    // the end state is the same whichever allocation was refused on the way
    CHECK(f.a && f.b && f.tab && f.g && f.g_cap == 128 && f.pa && f.pb && f.p_cap == 200 && f.ka && f.kb && f.k_cap == 300 && f.pinned);
    CHECK(g_dev.count(f.a) && g_dev.count(f.g) && g_dev.count(f.ka) && g_dev.count(f.kb) && g_host.count(f.pinned) && g_host.size() == 1);
    for (int i = 0; i < 64; ++i) CHECK(f.tab->v[i] == 3 * i + 1);
    CHECK(g_uploads == 1);
    memset(f.pa, 1, frames * 200 * sizeof(RecA));                    // the blocks have the sizes asked for (ASan watches)
    memset(f.pb, 1, frames * 200 * sizeof(RecB));
    memset(f.ka, 1, frames * 300 * sizeof(RecA));
    memset(f.kb, 1, frames * 300 * sizeof(RecB));
    memset(f.g, 1, 128);
    const int allocs = g_allocs - (k ? 1 : 0);                       // (the refused one counted)
    const size_t live = m.live();
    CHECK(live == 9 && g_dev.size() == 8);
    const int frees_before = g_frees;
    m.release_all();
    CHECK(g_frees == frees_before + (int)live && m.live() == 0 && g_dev.empty() && g_host.empty());
    CHECK(!f.a && !f.b && !f.tab && !f.g && !f.pa && !f.pb && !f.ka && !f.kb && !f.pinned);
    m.release_all();                                                 // a second one frees nothing
    CHECK(g_frees == frees_before + (int)live);
    return allocs;
}

// table(): the device block goes when the upload fails; nothing is allocated when fill fails; either way the field stays null,
// the error is cleared where the runtime raised one, and the same call succeeds afterwards
static void run_table_faults() {
    g_k = -1;
    g_allocs = g_frees = g_cleared = g_uploads = 0;
    g_fail_at = 0;
    Table *tab = nullptr;
    float *other = nullptr;
    CtxMem m(&kFake);
    CHECK(m.once(&other, 64, "another buffer") == 0);
    g_fail_upload = true;
    CHECK(m.table(&tab, "the table", fill_table) == -1);
    CHECK(!tab && m.live() == 1 && g_dev.size() == 1 && g_frees == 1 && g_cleared == 1 && strstr(g_err, "uploading the table failed: fake refusal"));
    g_fail_upload = false;
    CHECK(m.table(&tab, "the table", [](Table *) { return ft8_fail("fill refuses"); }) == -1);
    CHECK(!tab && m.live() == 1 && g_dev.size() == 1 && g_frees == 1 && !strcmp(g_err, "fill refuses"));
    CHECK(m.table(&tab, "the table", fill_table) == 0);
    CHECK(tab && tab->v[63] == 190 && m.live() == 2 && g_dev.size() == 2);
    CHECK(m.table(&tab, "the table", [](Table *) { return ft8_fail("fill must not run again"); }) == 0);
    m.release_all();
    CHECK(!tab && !other && g_dev.empty() && g_frees == 3);
}

int main() {
    const int n = run_script(0);
    CHECK(n == 14);                                                  // 2 once, the table, 2 grow, 2 x 2 pair, 2 x 2 kept pair, the pinned block
    for (int k = 1; k <= n; ++k) run_script(k);
    run_table_faults();
    CHECK(g_dev.empty() && g_host.empty());
    printf("ctx_mem_asan ok: %d allocations, each refused once\n", n);
    return 0;
}
