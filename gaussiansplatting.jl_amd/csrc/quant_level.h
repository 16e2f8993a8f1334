// THE 8-bit quantiser of the frame exports: eval.hip (gsr_eval_metrics, gsr_frame_rgb8) and frames.hip (gsr_frame_normal8)
// call this one device function.  Meant for translation units compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

// The integer level of `quantize8` (utils.jl:118) as a float.  Each operation is its own fp32 operation (the product is
// rounded before the sum: not rintf, not a float -> integer conversion of x · 255).
__device__ __forceinline__ float quant_level(float x) { return floorf(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f + 0.5f); }
