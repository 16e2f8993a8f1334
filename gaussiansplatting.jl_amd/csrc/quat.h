// Quaternion helpers of the per-Gaussian kernels that rotate a sample into a Gaussian's frame: densify.hip (split noise) and
// mcmc.hip (position noise).  Both are compiled with -ffp-contract=off; the expression below is the one
// tests/test_gpu_densify.py pins against oracle/densify.py: unnorm_quat2rot.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

// unnorm_quat2rot (render.jl:322-333), row-major, q = (w, x, y, z) not normalised
__device__ __forceinline__ void unnorm_quat2rot(const float4 q4, float (&R)[3][3]) {
    const float inv = 1.0f / sqrtf(q4.x * q4.x + q4.y * q4.y + q4.z * q4.z + q4.w * q4.w);
    const float w = q4.x * inv, x = q4.y * inv, y = q4.z * inv, z = q4.w * inv;
    const float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0][0] = 1.0f - 2.0f * (y2 + z2); R[0][1] = 2.0f * (xy - wz); R[0][2] = 2.0f * (xz + wy);
    R[1][0] = 2.0f * (xy + wz); R[1][1] = 1.0f - 2.0f * (x2 + z2); R[1][2] = 2.0f * (yz - wx);
    R[2][0] = 2.0f * (xz - wy); R[2][1] = 2.0f * (yz + wx); R[2][2] = 1.0f - 2.0f * (x2 + y2);
}

}  // namespace gsr
