// What every host file of libgsr_hip.so needs (gsr_api.cpp: the handle; gsr_ops.cpp: the entry points without one): the
// library's one error buffer, fail(), HIPCHK, and the Adam step sizes both files compute.
#pragma once
#include "../../include/gsr.h"

#include <math.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>

namespace gsr_host {

// gsr_last_error_string's text: one buffer per thread for the whole library (defined in gsr_api.cpp)
extern thread_local char g_err[512];

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail(e_ == hipErrorOutOfMemory ? GSR_E_OOM : GSR_E_HIP, "%s failed: %s (%s:%d)", #expr,   \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                          \
    } while (0)

// gsr_ssim_precision's process-wide default (defined in gsr_api.cpp, with the other process-wide switches): the planar SSIM
// entry points of gsr_ops.cpp read it too
extern std::atomic<int> g_ssim_exact;

// Adam's step size with both debiasing factors folded in (Kingma & Ba §2); current_step counts from 1
inline float adam_lr_t(float lr, float beta1, float beta2, uint32_t current_step) {
    const float t = (float)current_step;
    return lr * sqrtf(1.0f - powf(beta2, t)) / (1.0f - powf(beta1, t));
}

// lr_t of the trainer's six groups, after checking their arrays and counters; rest_empty: the scene has no features_rest
// (group 2), whose arrays are then not looked at (training.jl:770)
inline int tail_lr_t(float* const theta[6], float* const mu[6], float* const nu[6], const float lr[6],
                     const uint32_t current_step[6], float beta1, float beta2, bool rest_empty, float lr_t[6]) {
    for (int g = 0; g < 6; g++) {
        if (g == 2 && rest_empty) { lr_t[g] = 0.0f; continue; }
        if (!theta[g] || !mu[g] || !nu[g]) return fail(GSR_E_INVALID_ARG, "group %d: null array", g);
        if (current_step[g] == 0) return fail(GSR_E_INVALID_ARG, "group %d: current_step counts from 1", g);
        lr_t[g] = adam_lr_t(lr[g], beta1, beta2, current_step[g]);
    }
    return GSR_OK;
}

}  // namespace gsr_host
