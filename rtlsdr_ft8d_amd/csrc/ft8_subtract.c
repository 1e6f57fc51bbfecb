/* ft8_subtract.c -- host tables of the subtraction in the I/Q samples (include/ft8gpu.h "subtraction in the I/Q samples").
 * Plain C, no GPU. */
#include "../../include/ft8gpu.h"

#include <math.h>

/* w4[i] = (cos, -sin)(2 pi i / 4096), each the float of the double value, as build_tables forms the waterfall's table */
void ft8gpu_subtract_twiddles(float *out) {
    if (!out) return;
    for (int i = 0; i < FT8GPU_SUBTRACT_TABLE; i++) {
        const double a = 2.0 * M_PI * (double)i / (double)FT8GPU_SUBTRACT_TABLE;
        out[2 * i] = (float)cos(a);
        out[2 * i + 1] = (float)(-sin(a));
    }
}

/* inv[n] = (float)(1.0 / (32 n)), n = 1 .. 2 * FT8GPU_SUBTRACT_SMOOTH + 1; inv[0] = 0 (not part of the ABI) */
__attribute__((visibility("hidden"))) void ft8_subtract_inv_table(float *inv) {
    inv[0] = 0.0f;
    for (int n = 1; n <= 2 * FT8GPU_SUBTRACT_SMOOTH + 1; n++) inv[n] = (float)(1.0 / (32.0 * (double)n));
}
