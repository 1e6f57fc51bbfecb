/*
 * ref_harness.c -- runs the reference's own rtlsdr_ft8d.c (test infrastructure, `make -C oracle ref`).
 *
 * The reference is compiled where it lies, in THIS translation unit: REF_SOURCE names its rtlsdr_ft8d.c (the recipe
 * passes -DREF_SOURCE="\"<checkout>/rtlsdr_ft8d.c\""), its main() is renamed rtlsdr_ft8d_main, and being in the same
 * unit lets the harness call the file-static rtlsdr_callback().  Nothing of the reference is copied here.  What it
 * needs besides libc comes from three places the link chooses:
 *   - ref_stubs.c        rtlsdr_* and curl_* as abort(): no device and no network can be reached
 *   - ref_fftw_shim.c    the fftwf_* names over the oracle's ft8o_fft1024, counting the transforms
 *   - the ft8_lib names  ft8_find_sync / ft8_decode / pack77 / ft8_encode: from the oracle
 *                        (tools/pin_ft8_lib/oracle_as_ft8_lib.c, binary ref_oracle) or from libft8gpu.so (ref_gpu)
 * The reference's call of ft8_find_sync() is routed through ref_find_sync() below, which may append the waterfall it
 * is handed (mag_power of ft8_subsystem, 94 208 bytes) to a file, then calls the ft8_find_sync of the link.
 *
 * Modes (binary on stdin and stdout, native byte order):
 *   daemon ARGS...          the reference's main(ARGS...)
 *   rx CHUNK                stdin: raw u8 I/Q capture.  initSampleStorage(), then rtlsdr_callback() per CHUNK bytes.
 *                           stdout: iSamples[0][48000], qSamples[0][48000] (float32), iqIndex[0] (uint32)
 *   subsystem N FILL [WF]   stdin: N frames of I[48000], Q[48000].  Per frame: dec_results filled with byte FILL,
 *                           ft8_subsystem().  stdout per frame: n_results (int32), 50 records (28 B each),
 *                           fftwf_execute calls of that frame (uint32).  WF: the waterfalls are appended to this file.
 *   read-iq PATH FILL       readRawIQfile() into I/Q buffers filled with byte FILL.
 *   read-c2 PATH FILL       readC2file() likewise.  Both write: return value (int32), rx_options.dialfreq (uint32),
 *                           I[48000], Q[48000]
 *   write-iq PATH           stdin: I[48000], Q[48000].  writeRawIQfile(); stdout: return value (int32)
 *   print-spots N DIAL Y M D H MIN
 *                           stdin: 50 records.  printSpots(N) with dec_options.freq = DIAL and rx_state.gtm at the
 *                           given UTC date (tm_year = Y - 1900, tm_mon = M - 1), so that the n == 0 line is fixed.
 *
 * ONE CAPTURE PER PROCESS: rtlsdr_callback() keeps its CIC and FIR state in function-static variables and
 * whiteGaussianNoise() its phase and rand() sequence, none of which can be reset from outside.  A second capture in
 * the same process would continue the first one's filters, so the tests start a fresh process for every capture and
 * every self-test.  (subsystem mode may run many frames: ft8_subsystem keeps no state between calls.)
 */
#define main rtlsdr_ft8d_main
#define ft8_find_sync ref_find_sync
#include REF_SOURCE
#undef ft8_find_sync
#undef main

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

int ft8_find_sync(const waterfall_t *power, int num_candidates, candidate_t heap[], int min_score);
extern unsigned long ref_fftw_executions;               /* ref_fftw_shim.c */

static FILE *g_waterfall_out = NULL;

int ref_find_sync(const waterfall_t *power, int num_candidates, candidate_t heap[], int min_score) {
    if (g_waterfall_out && fwrite(power->mag, 1, MAG_ARRAY, g_waterfall_out) != MAG_ARRAY) {
        fprintf(stderr, "ref_harness: cannot write the waterfall\n");
        exit(3);
    }
    return ft8_find_sync(power, num_candidates, heap, min_score);
}

enum { kSamples = SIGNAL_LENGHT * SIGNAL_SAMPLE_RATE };

static void read_exact(void *dst, size_t n) {
    if (fread(dst, 1, n, stdin) != n) {
        fprintf(stderr, "ref_harness: short input\n");
        exit(2);
    }
}

static void write_all(const void *src, size_t n) {
    if (fwrite(src, 1, n, stdout) != n) {
        fprintf(stderr, "ref_harness: short output\n");
        exit(2);
    }
}

static unsigned char *read_stdin(size_t *len) {
    size_t cap = 1 << 20, n = 0;
    unsigned char *buf = malloc(cap);
    for (;;) {
        if (!buf) { fprintf(stderr, "ref_harness: out of memory\n"); exit(2); }
        n += fread(buf + n, 1, cap - n, stdin);
        if (n < cap) break;
        cap *= 2;
        buf = realloc(buf, cap);
    }
    *len = n;
    return buf;
}

static int mode_rx(long chunk) {
    if (chunk <= 0 || chunk % 8) { fprintf(stderr, "ref_harness: CHUNK must be a positive multiple of 8\n"); return 2; }
    size_t len;
    unsigned char *raw = read_stdin(&len);
    if (len % 8) { fprintf(stderr, "ref_harness: capture length must be a multiple of 8 bytes\n"); return 2; }
    initSampleStorage();
    for (size_t off = 0; off < len; off += (size_t)chunk) {
        const size_t n = len - off < (size_t)chunk ? len - off : (size_t)chunk;
        rtlsdr_callback(raw + off, (uint32_t)n, NULL);
    }
    write_all(rx_state.iSamples[0], sizeof(float) * kSamples);
    write_all(rx_state.qSamples[0], sizeof(float) * kSamples);
    write_all(&rx_state.iqIndex[0], sizeof(uint32_t));
    free(raw);
    return 0;
}

static int mode_subsystem(long nframes, int fill, const char *waterfall_path) {
    static float iSamples[kSamples], qSamples[kSamples];
    if (waterfall_path && !(g_waterfall_out = fopen(waterfall_path, "wb"))) {
        fprintf(stderr, "ref_harness: cannot open %s\n", waterfall_path);
        return 2;
    }
    initFFTW();
    for (long f = 0; f < nframes; f++) {
        read_exact(iSamples, sizeof iSamples);
        read_exact(qSamples, sizeof qSamples);
        memset(dec_results, fill, sizeof dec_results);
        int32_t n_results = -1;
        const unsigned long before = ref_fftw_executions;
        ft8_subsystem(iSamples, qSamples, kSamples, dec_results, &n_results);
        const uint32_t ffts = (uint32_t)(ref_fftw_executions - before);
        write_all(&n_results, sizeof n_results);
        write_all(dec_results, sizeof dec_results);
        write_all(&ffts, sizeof ffts);
    }
    if (g_waterfall_out && fclose(g_waterfall_out) != 0) return 3;
    return 0;
}

static int mode_read(int c2, char *path, int fill) {
    static float iSamples[kSamples], qSamples[kSamples];
    memset(iSamples, fill, sizeof iSamples);
    memset(qSamples, fill, sizeof qSamples);
    rx_options.dialfreq = 0;
    const int32_t rc = c2 ? readC2file(iSamples, qSamples, path) : readRawIQfile(iSamples, qSamples, path);
    const uint32_t dial = rx_options.dialfreq;
    write_all(&rc, sizeof rc);
    write_all(&dial, sizeof dial);
    write_all(iSamples, sizeof iSamples);
    write_all(qSamples, sizeof qSamples);
    return 0;
}

static int mode_write(char *path) {
    static float iSamples[kSamples], qSamples[kSamples];
    read_exact(iSamples, sizeof iSamples);
    read_exact(qSamples, sizeof qSamples);
    const int32_t rc = writeRawIQfile(iSamples, qSamples, path);
    write_all(&rc, sizeof rc);
    return 0;
}

static int mode_print_spots(char **a) {
    static struct tm when;
    const int32_t n = atoi(a[0]);
    read_exact(dec_results, sizeof dec_results);
    dec_options.freq = (uint32_t)strtoul(a[1], NULL, 10);
    when.tm_year = atoi(a[2]) - 1900;
    when.tm_mon = atoi(a[3]) - 1;
    when.tm_mday = atoi(a[4]);
    when.tm_hour = atoi(a[5]);
    when.tm_min = atoi(a[6]);
    rx_state.gtm = &when;
    printSpots(n);
    return fflush(stdout) == 0 ? 0 : 2;
}

int main(int argc, char **argv) {
    _Static_assert(sizeof(struct decoder_results) == 28, "record layout");
    const char *mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "daemon")) return rtlsdr_ft8d_main(argc - 1, argv + 1);
    if (!strcmp(mode, "rx") && argc == 3) return mode_rx(atol(argv[2]));
    if (!strcmp(mode, "subsystem") && (argc == 4 || argc == 5))
        return mode_subsystem(atol(argv[2]), (int)strtol(argv[3], NULL, 0), argc == 5 ? argv[4] : NULL);
    if (!strcmp(mode, "read-iq") && argc == 4) return mode_read(0, argv[2], (int)strtol(argv[3], NULL, 0));
    if (!strcmp(mode, "read-c2") && argc == 4) return mode_read(1, argv[2], (int)strtol(argv[3], NULL, 0));
    if (!strcmp(mode, "write-iq") && argc == 3) return mode_write(argv[2]);
    if (!strcmp(mode, "print-spots") && argc == 9) return mode_print_spots(argv + 2);
    fprintf(stderr, "usage: %s daemon ARGS... | rx CHUNK | subsystem N FILL [WATERFALL_FILE] | read-iq PATH FILL |"
                    " read-c2 PATH FILL | write-iq PATH | print-spots N DIAL YEAR MONTH MDAY HOUR MIN\n", argv[0]);
    return 2;
}
