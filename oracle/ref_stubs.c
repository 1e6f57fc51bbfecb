/*
 * ref_stubs.c -- librtlsdr and libcurl for oracle/_ref/ref_* (ref_harness.c): every function the reference names
 * aborts.  The harness drives only the parts of the reference that never touch a receiver or the network (the -t and
 * -r modes of main return before the first rtlsdr call; webClusterSpots, the only libcurl user, is never called), so
 * reaching one of these is a harness bug that must end the run, and with them the binaries need neither library and
 * leave no network name for the dynamic linker (tests/test_reference_exec.py checks `nm -u`).
 * Signatures: the declaration-only headers of tests/stub_sys.
 */
#include <stdio.h>
#include <stdlib.h>

#include <rtl-sdr.h>
#include <curl/curl.h>

static _Noreturn void unreachable(const char *name) {
    fprintf(stderr, "ref_harness: the reference called %s, which this harness never provides\n", name);
    abort();
}

#define STUB(ret, name, ...) ret name(__VA_ARGS__) { unreachable(#name); }

STUB(uint32_t, rtlsdr_get_device_count, void)
STUB(const char *, rtlsdr_get_device_name, uint32_t index)
STUB(int, rtlsdr_get_device_usb_strings, uint32_t index, char *manufact, char *product, char *serial)
STUB(int, rtlsdr_open, rtlsdr_dev_t **dev, uint32_t index)
STUB(int, rtlsdr_close, rtlsdr_dev_t *dev)
STUB(int, rtlsdr_set_center_freq, rtlsdr_dev_t *dev, uint32_t freq)
STUB(int, rtlsdr_set_freq_correction, rtlsdr_dev_t *dev, int ppm)
STUB(int, rtlsdr_set_tuner_gain, rtlsdr_dev_t *dev, int gain)
STUB(int, rtlsdr_set_tuner_gain_mode, rtlsdr_dev_t *dev, int manual)
STUB(int, rtlsdr_set_sample_rate, rtlsdr_dev_t *dev, uint32_t rate)
STUB(int, rtlsdr_set_direct_sampling, rtlsdr_dev_t *dev, int on)
STUB(int, rtlsdr_reset_buffer, rtlsdr_dev_t *dev)
STUB(int, rtlsdr_read_async, rtlsdr_dev_t *dev, rtlsdr_read_async_cb_t cb, void *ctx, uint32_t buf_num, uint32_t buf_len)
STUB(int, rtlsdr_cancel_async, rtlsdr_dev_t *dev)

STUB(CURLcode, curl_global_init, long flags)
STUB(CURL *, curl_easy_init, void)
STUB(CURLcode, curl_easy_setopt, CURL *handle, CURLoption option, ...)
STUB(CURLcode, curl_easy_perform, CURL *handle)
STUB(void, curl_easy_cleanup, CURL *handle)
STUB(const char *, curl_easy_strerror, CURLcode code)
STUB(CURLFORMcode, curl_formadd, struct curl_httppost **first, struct curl_httppost **last, ...)
STUB(void, curl_formfree, struct curl_httppost *form)
