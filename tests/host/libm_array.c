/* The machine's own libm over an array: log10f(x[i]) and powf(x[i], y), one call per element (tests/test_gpu_libm_device.py
 * compares them with the library's restatement; a call per element from Python would take a minute for 22 million values).
 * Built with -fno-builtin so that every call reaches libm.so.6. */
#include <math.h>

void libm_log10f_array(const float* x, float* out, long long n) {
    for (long long i = 0; i < n; ++i) out[i] = log10f(x[i]);
}

void libm_powf_array(const float* x, float y, float* out, long long n) {
    for (long long i = 0; i < n; ++i) out[i] = powf(x[i], y);
}
