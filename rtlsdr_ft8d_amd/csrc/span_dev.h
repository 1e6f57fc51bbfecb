// span_dev.h -- the I/Q staging of the kernels that correlate a record against the frame's samples (refine.hip, subtract.hip),
// kept once together with the layout it writes: segments of 32 samples at a pitch of 33 floats, so that the 16 segments of a
// symbol start on 16 different banks.
#pragma once
#include "ft8gpu_internal.h"

namespace {

constexpr int kStageSeg = 32;                                  // samples per staged segment
constexpr int kStagePitch = kStageSeg + 1;                     // floats from one staged segment to the next

// NSEG segments from sample j0 (a multiple of 4) into the wave's planes; samples outside the frame are zero, not read
template <int NSEG>
__device__ __forceinline__ void stage_span(const float *__restrict__ pi, const float *__restrict__ pq, int j0, float *s_i, float *s_q,
                                           int lane) {
    static_assert(NSEG * kStageSeg / 4 % 64 == 0, "whole rounds of 64 float4");
#pragma unroll
    for (int r = 0; r < NSEG * kStageSeg / 4 / 64; ++r) {
        const int v = lane + 64 * r;
        const int j = j0 + 4 * v;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        if (j >= 0 && j < kNSamples) {                                       // 48000 is a multiple of 4: all four or none
            a = *reinterpret_cast<const float4 *>(pi + j);
            b = *reinterpret_cast<const float4 *>(pq + j);
        }
        const int p = 4 * v + (v >> 3);                                      // sample o sits at o + (o >> 5)
        s_i[p] = a.x; s_i[p + 1] = a.y; s_i[p + 2] = a.z; s_i[p + 3] = a.w;
        s_q[p] = b.x; s_q[p + 1] = b.y; s_q[p + 2] = b.z; s_q[p + 3] = b.w;
    }
}

}  // namespace
