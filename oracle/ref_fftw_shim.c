/*
 * ref_fftw_shim.c -- the FFTW 3 names the reference calls (initFFTW, ft8_subsystem, freeFFTW), implemented over the
 * oracle's 1024-point float32 transform ft8o_fft1024, for oracle/_ref/ref_* (ref_harness.c).  With it the reference's
 * own waterfall code (window, |X|^2, log, quantiser, layout) runs on the transform the oracle and the GPU kernel use,
 * so its mag_power can be compared byte for byte with theirs.
 *
 * Only what the reference asks for is accepted: one size (1024), the forward sign, out of place or in place.  Anything
 * else aborts.  Wisdom is neither read nor written.  ref_fftw_executions counts fftwf_execute calls, so the tests can
 * tell that the reference's waterfall loop ran (184 transforms per frame: 92 blocks x 2 time offsets).
 * Not tests/host_fftw_shim (a float64 DFT for the sanitizer builds).
 */
#include <stdio.h>
#include <stdlib.h>

#include <fftw3.h>

#include "ft8_oracle.h"

unsigned long ref_fftw_executions = 0;

struct fftwf_plan_s {
    fftwf_complex *in, *out;
};

static _Noreturn void refuse(const char *what) {
    fprintf(stderr, "ref_fftw_shim: %s\n", what);
    abort();
}

void *fftwf_malloc(size_t n) { return malloc(n); }

void fftwf_free(void *p) { free(p); }

fftwf_plan fftwf_plan_dft_1d(int n, fftwf_complex *in, fftwf_complex *out, int sign, unsigned flags) {
    (void)flags;
    if (n != FT8O_NFFT) refuse("only 1024-point transforms are provided");
    if (sign != FFTW_FORWARD) refuse("only the forward transform is provided");
    if (!in || !out) refuse("a plan needs its buffers");
    fftwf_plan p = malloc(sizeof *p);
    if (!p) refuse("out of memory");
    p->in = in;
    p->out = out;
    ft8o_init();
    return p;
}

void fftwf_execute(const fftwf_plan p) {
    float re[FT8O_NFFT], im[FT8O_NFFT];
    for (int i = 0; i < FT8O_NFFT; i++) {
        re[i] = p->in[i][0];
        im[i] = p->in[i][1];
    }
    ft8o_fft1024(re, im);
    for (int i = 0; i < FT8O_NFFT; i++) {
        p->out[i][0] = re[i];
        p->out[i][1] = im[i];
    }
    ref_fftw_executions++;
}

void fftwf_destroy_plan(fftwf_plan p) { free(p); }

int fftwf_import_wisdom_from_file(FILE *input_file) {
    (void)input_file;
    return 0;
}

void fftwf_export_wisdom_to_file(FILE *output_file) { (void)output_file; }
