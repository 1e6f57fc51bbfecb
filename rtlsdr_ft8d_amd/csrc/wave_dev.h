// wave_dev.h -- the barrier of the one-wave-per-item kernels, kept once: a wave that exchanges data through its own piece of
// LDS needs no s_barrier, only the order of its own LDS stores and loads.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace
