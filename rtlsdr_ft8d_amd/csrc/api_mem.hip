// api_mem.hip -- the HIP binding of the context's memory owner (ctx_mem.h).  Beside the four helpers for the caller's own memory
// (ft8gpu_dev_alloc / _dev_free / _host_alloc / _host_free, api_context.hip) this is the only place of the library's host side
// that allocates or frees device or pinned memory (tests/test_abi.py holds the sources to that).  Every function acts on the
// current device: the entries hold the context's Entry guard, ft8gpu_create / ft8gpu_destroy set the device themselves.
#include "ft8gpu_ctx.h"

namespace {

void *dev_alloc(size_t bytes) { void *p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; }
void dev_free(void *p) { (void)hipFree(p); }                  // waits for work that still uses the block
void *host_alloc(size_t bytes) { void *p = nullptr; return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr; }
void host_free(void *p) { (void)hipHostFree(p); }
int upload(void *dst, const void *src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1; }
const char *clear_error() { return hipGetErrorString(hipGetLastError()); }

}  // namespace

const MemBackend *hip_mem() {
    static const MemBackend b = { dev_alloc, dev_free, host_alloc, host_free, upload, clear_error };
    return &b;
}
