// The project's counter-based random generator: 32 well-mixed bits from (seed, row, draw) — integer only, so a host
// restatement (oracle/densify.py: _mix32, uniform01, randn3) reproduces the stream bit for bit.  The reference draws
// from the backend's device RNG (`randn(Float32)`, densification.jl:128, mcmc.jl:310) or the host's `rand()`
// (mcmc.jl:224), which no implementation can reproduce.  Shared by densify.hip (split noise) and mcmc.hip (multinomial
// draws, position noise); both are compiled with -ffp-contract=off, and the float expressions below are the ones
// tests/test_gpu_densify.py pins.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t rand_bits(uint32_t seed, uint32_t row, uint32_t draw) {
    return mix32(mix32(seed ^ (row * 0x9E3779B9u)) + draw * 0x85EBCA6Bu);
}
__device__ __forceinline__ float uniform01(uint32_t seed, uint32_t row, uint32_t draw) {
    return ((float)(rand_bits(seed, row, draw) >> 8) + 0.5f) * (1.0f / 16777216.0f);  // (0, 1)
}

// Box-Muller: two pairs of uniforms (draws 0..3 of `row`) -> three normals
__device__ __forceinline__ void randn3(uint32_t seed, uint32_t row, float (&xi)[3]) {
    const float u1 = uniform01(seed, row, 0), u2 = uniform01(seed, row, 1);
    const float u3 = uniform01(seed, row, 2), u4 = uniform01(seed, row, 3);
    const float r1 = sqrtf(-2.0f * logf(u1)), r2 = sqrtf(-2.0f * logf(u3));
    const float two_pi = 6.2831853071795864f;
    xi[0] = r1 * cosf(two_pi * u2);
    xi[1] = r1 * sinf(two_pi * u2);
    xi[2] = r2 * cosf(two_pi * u4);
}

}  // namespace gsr
