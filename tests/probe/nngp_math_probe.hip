// nngp_math_probe.hip -- TEST INFRASTRUCTURE: the device routines of csrc/nngp_math.h, one lane per
// element, so tests/test_gpu_math_probe.py can compare them with the oracle's copy (and with IEEE
// sqrt / division) bit for bit at arguments no kernel test produces.  It includes the product's
// header itself and is built with the product's flags (csrc/Makefile) into a library of its own,
// lib/libnngp_mathprobe.so; nothing of it is linked into libnngp_hip.so or declared in nngp.h.
// Arguments come from memory, so nothing folds at compile time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nngp_math.h"

namespace {

// the `fn` codes (tests/math_probe.py FN restates them)
enum : int {
    FN_EXP = 0,
    FN_EXP_NONPOS = 1,
    FN_EXP_NONPOS_SEP = 2,
    FN_EXP_DD = 3,           // (a, b) = (hi, lo)
    FN_POW10 = 4,
    FN_LOG = 5,
    FN_SINCOS = 6,           // out0 = sin, out1 = cos
    FN_SIN = 7,
    FN_COS = 8,
    FN_SIN_PI = 9,
    FN_SQRT_MID = 10,        // out1 = the device's sqrt(a)
    FN_RCP_MID = 11,         // out1 = the device's 1.0 / a
    FN_IN_MID_RANGE = 12,    // 0.0 / 1.0
    FN_SQRT_RCP_EXACT = 13,  // out0 = ljj, out1 = ri
    FN_COUNT = 14
};

__global__ void __launch_bounds__(256) math_probe_kernel(int fn, int64_t n, const double *__restrict__ a,
                                                         const double *__restrict__ b, double *__restrict__ out0,
                                                         double *__restrict__ out1) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    double r0 = 0.0, r1 = 0.0;
    bool two = false;
    switch (fn) {
        case FN_EXP: r0 = nngp::nn_exp(x); break;
        case FN_EXP_NONPOS: r0 = nngp::nn_exp_nonpos(x); break;
        case FN_EXP_NONPOS_SEP: r0 = nngp::nn_exp_nonpos_sep(x); break;
        case FN_EXP_DD: r0 = nngp::nn_exp_dd(x, b[i]); break;
        case FN_POW10: r0 = nngp::nn_pow10(x); break;
        case FN_LOG: r0 = nngp::nn_log(x); break;
        case FN_SINCOS: nngp::nn_sincos(x, r0, r1); two = true; break;
        case FN_SIN: r0 = nngp::nn_sin(x); break;
        case FN_COS: r0 = nngp::nn_cos(x); break;
        case FN_SIN_PI: r0 = nngp::nn_sin_pi(x); break;
        case FN_SQRT_MID: r0 = nngp::sqrt_mid(x); r1 = sqrt(x); two = true; break;
        case FN_RCP_MID: r0 = nngp::rcp_mid(x); r1 = 1.0 / x; two = true; break;
        case FN_IN_MID_RANGE: r0 = nngp::in_mid_range(x) ? 1.0 : 0.0; break;
        case FN_SQRT_RCP_EXACT: nngp::sqrt_rcp_exact(x, r0, r1); two = true; break;
        default: break;
    }
    out0[i] = r0;
    if (two) out1[i] = r1;
}

}  // namespace

// fn over a[0 .. n) (and b for nn_exp_dd) into out0 (and out1 for the two-output codes, which need
// it).  Returns the HIP error code of the launch (hipErrorInvalidValue for a bad argument, nothing
// launched); no synchronisation: the caller owns the buffers and the stream.
extern "C" __attribute__((visibility("default"))) int nngp_math_probe(int fn, int64_t n, const double *a,
                                                                      const double *b, double *out0, double *out1,
                                                                      void *stream) {
    const bool two = fn == FN_SINCOS || fn == FN_SQRT_MID || fn == FN_RCP_MID || fn == FN_SQRT_RCP_EXACT;
    if (fn < 0 || fn >= FN_COUNT || n < 0 || n > ((int64_t)1 << 31) || (n > 0 && (!a || !out0)) ||
        (n > 0 && fn == FN_EXP_DD && !b) || (n > 0 && two && !out1))
        return (int)hipErrorInvalidValue;
    if (n == 0) return (int)hipSuccess;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    math_probe_kernel<<<dim3(blocks), dim3(256), 0, (hipStream_t)stream>>>(fn, n, a, b, out0, out1);
    return (int)hipGetLastError();
}
