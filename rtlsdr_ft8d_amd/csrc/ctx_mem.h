// ctx_mem.h -- the one owner of a context's device and pinned host memory (ft8gpu_ctx::mem).  Plain C++17, no HIP: the runtime
// is reached through a MemBackend (the HIP one is api_mem.hip), so tests/host_asan drives this header with a counting fake
// under AddressSanitizer.  The context keeps its named pointer fields; the owner records the address of every field it filled
// and release_all() frees them.  One failure rule for every operation: the field stays (or becomes) null, a cap 0, nothing is
// recorded, the runtime's last error is cleared -- a later launch on the context must not report it -- and ft8_fail() names what
// was wanted, its size and the runtime's reason.
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <vector>

int ft8_fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

struct MemBackend {
    void *(*dev_alloc)(size_t bytes);                          // nullptr: failed
    void (*dev_free)(void *p);
    void *(*host_alloc)(size_t bytes);                         // pinned
    void (*host_free)(void *p);
    int (*upload)(void *dst, const void *src, size_t bytes);   // host to device, complete on return; 0: done
    const char *(*clear_error)();                              // the runtime's last error as text; clears it
};

class CtxMem {
public:
    explicit CtxMem(const MemBackend *b) : b_(b) {}
    CtxMem(const CtxMem &) = delete;
    // *field, if it is still null: `bytes` of device (once) or pinned host (once_pinned) memory
    template <class T> int once(T **field, size_t bytes, const char *what) { return *field ? 0 : alloc((void **)field, bytes, what, false); }
    template <class T> int once_pinned(T **field, size_t bytes, const char *what) { return *field ? 0 : alloc((void **)field, bytes, what, true); }
    // at least `need` bytes; the old block goes first and its content is lost (the caller has synchronised whatever used it)
    template <class T> int grow(T **field, size_t *cap, size_t need, const char *what) {
        if (need <= *cap) return 0;
        drop((void **)field);
        *cap = 0;
        if (alloc((void **)field, need, what, false)) return -1;
        *cap = need;
        return 0;
    }
    // a constant table: fill(T *) writes a zeroed host T and returns 0, the table is uploaded; all or nothing
    template <class T, class Fill> int table(T **field, const char *what, Fill fill) {
        if (*field) return 0;
        T *h = (T *)calloc(1, sizeof(T));
        if (!h) return ft8_fail("out of host memory for %s", what);
        int rc = fill(h);
        if (!rc) rc = alloc((void **)field, sizeof(T), what, false);
        if (!rc && b_->upload(*field, h, sizeof(T))) {
            rc = ft8_fail("uploading %s failed: %s", what, b_->clear_error());
            drop((void **)field);
        }
        free(h);
        return rc;
    }
    // [frames][want] records of A and of B once *cap < want: the old pair goes first, as in grow()
    template <class A, class B> int pair(A **a, B **b, int *cap, int want, size_t frames, const char *what) {
        if (*cap >= want) return 0;
        drop((void **)a);
        drop((void **)b);
        *cap = 0;
        if (alloc((void **)a, frames * want * sizeof(A), what, false)) return -1;
        if (alloc((void **)b, frames * want * sizeof(B), what, false)) { drop((void **)a); return -1; }
        *cap = want;
        return 0;
    }
    // the same, all or nothing: both new blocks exist before the old pair goes, and a failure leaves *a, *b and *cap as they were
    template <class A, class B> int pair_kept(A **a, B **b, int *cap, int want, size_t frames, const char *what) {
        void *na = nullptr, *nb = nullptr;
        if (alloc(&na, frames * want * sizeof(A), what, false)) return -1;
        if (alloc(&nb, frames * want * sizeof(B), what, false)) { drop(&na); return -1; }
        drop((void **)a);
        drop((void **)b);
        for (Rec &r : recs_) if (r.field == &na) r.field = (void **)a; else if (r.field == &nb) r.field = (void **)b;
        *a = (A *)na;
        *b = (B *)nb;
        *cap = want;
        return 0;
    }
    // every recorded field, freed once and nulled
    void release_all() {
        for (Rec &r : recs_) { (r.pinned ? b_->host_free : b_->dev_free)(*r.field); *r.field = nullptr; }
        recs_.clear();
    }
    size_t live() const { return recs_.size(); }

private:
    struct Rec { void **field; bool pinned; };
    int alloc(void **field, size_t bytes, const char *what, bool pinned) {
        void *p = (pinned ? b_->host_alloc : b_->dev_alloc)(bytes);
        if (!p) return ft8_fail("out of %s memory for %s (%zu bytes): %s", pinned ? "pinned host" : "device", what, bytes, b_->clear_error());
        *field = p;
        recs_.push_back(Rec{ field, pinned });
        return 0;
    }
    void drop(void **field) {
        for (size_t i = 0; i < recs_.size(); ++i) {
            if (recs_[i].field != field) continue;
            (recs_[i].pinned ? b_->host_free : b_->dev_free)(*field);
            recs_.erase(recs_.begin() + i);
            break;
        }
        *field = nullptr;
    }
    const MemBackend *b_;
    std::vector<Rec> recs_;
};
