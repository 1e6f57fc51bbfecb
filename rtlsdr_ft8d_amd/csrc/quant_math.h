// quant_math.h -- the dB quantiser of the waterfall kernel (rtlsdr_ft8d.c:1415-1427), shared by that kernel (waterfall.hip)
// and by the exhaustive self-test (bp_selftest.hip: quantiser_exhaustive).  Device code only.
//
// qthr[k] = smallest float y with quantised value >= k (qthr[0] = 0, qthr[256..259] = NaN: never compares true), built on
// the host from the reference expression with the host's log10f (api_context.hip: build_tables).
//   * y = 1e-12f + (mag2 * 4.0f) / 1048576.0f in the reference; here one multiplication by 2^-18.
//   * g = 6.0206 log2(y) + 239.99 with v_log_f32 is a guess of the reference's float expression 2 * (10 * log10f(y)) + 240,
//     whose truncation is the result q, biased DOWN by 0.01: kl = trunc(g) satisfies kl <= q <= kl + 1, and q = kl + 1 exactly
//     when y >= qthr[kl + 1] -- one table read and one comparison per bin, branch-free.
// That the byte equals the reference's on EVERY float |X|^2 -- the single scaling against
// the reference's two (subnormal quotients, the overflowing product), the guess window with the device's own v_log_f32, the
// conversion of a NaN / infinite guess (v_cvt_i32_f32: NaN -> 0, +inf saturates and is clamped to 255, where NaN thresholds
// never compare), the table as uploaded -- is proven by exhaustion: ft8gpu_selftest_quantiser() walks every bit pattern
// 0 .. +inf and every NaN through quantise_pair below, in both slots of the pair, and returns the step function, which
// tests/test_gpu_quantiser.py compares step for step with that of the reference expression under the host's libm (the CPU
// oracle's exhaustive scan): 255 steps at identical bit patterns, q(0) = 0, every NaN -> 0.  The device walk takes 6 ms
// on one MI355X.
// Written on pairs so that the scalings and the affine map of the logarithm are packed instructions.
#pragma once
#include <hip/hip_runtime.h>

namespace qm {

typedef float f2 __attribute__((ext_vector_type(2)));

// |a|^2 and |b|^2 of two complex values (x = re, y = im).  A sum of two squares: never negative, never -0.
__device__ __forceinline__ f2 mag2_pair(f2 a, f2 b) {
    const f2 sa = a * a, sb = b * b;
    f2 mag2;                            // horizontal adds, written opaquely: the vectoriser otherwise transposes the two pairs with three moves
    asm("v_add_f32 %0, %1, %2" : "=v"(mag2.x) : "v"(sa.x), "v"(sa.y));
    asm("v_add_f32 %0, %1, %2" : "=v"(mag2.y) : "v"(sb.x), "v"(sb.y));
    return mag2;
}

// y and the guess kl (0..255) for both slots
__device__ __forceinline__ void guess_pair(f2 mag2, f2 &y, int &ka, int &kb) {
    y = mag2 * f2{ 0x1p-18f, 0x1p-18f } + f2{ 1E-12f, 1E-12f };
    const f2 l = { __log2f(y.x), __log2f(y.y) };
    const f2 g = l * f2{ 6.0206f, 6.0206f } + f2{ 239.99f, 239.99f };
    ka = (int)g.x;
    kb = (int)g.y;
    ka = ka > 255 ? 255 : ka;
    kb = kb > 255 ? 255 : kb;
}

// two values of |X|^2 -> two bytes
__device__ __forceinline__ void quantise_pair(f2 mag2, const float *qthr, unsigned &qa, unsigned &qb) {
    f2 y;
    int ka, kb;
    guess_pair(mag2, y, ka, kb);
    qa = (unsigned)ka + (y.x >= qthr[ka + 1] ? 1u : 0u);
    qb = (unsigned)kb + (y.y >= qthr[kb + 1] ? 1u : 0u);
}

}  // namespace qm
