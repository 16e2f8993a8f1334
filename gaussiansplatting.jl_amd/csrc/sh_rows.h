// The two cooperative SH row writers, device-only: a workgroup of 256 threads writes (store_sh_rows) or Adam-updates
// (tail_sh_group) the contiguous slice of SH rows of its 256 Gaussians element-major, as full cache lines.  Shared by the
// epilogue of the per-Gaussian backward (pergauss.hip: store_or_apply_sh) and by the multi-view SH sums (sh_views.hip).
//
// bench.py's hashes of the kernel sources, which mark profiles/pmc_traffic.json stale, cover pergauss.hip and not this
// file: after a change here, run tools/measure_pmc.sh again.
#pragma once
#include <stdint.h>
#include "adam_math.h"

namespace gsr {

// One SH optimizer group (features_dc: R = 3, k0 = 0; features_rest: R = 3 (K-1), k0 = 1) of the cnt Gaussians of a
// workgroup starting at i0, updated element-major by the whole workgroup so that θ, μ, ν stream as full cache lines
// (float4); grad(il, k, c) supplies the gradient of Gaussian il (0-based inside the workgroup), band k, channel c.  The
// updated coefficient is also written into the hcat copy `shs` the next forward reads (rasterizer.jl:218-228).  Shared by
// the backward's fused epilogue and by the multi-view tail (sh_views_tail_kernel): one definition, identical bits.
template <class Grad>
__device__ __forceinline__ void tail_sh_group(const gsr::TailState& TS, int i0, int cnt, int K3, float* __restrict__ th,
                                              float* __restrict__ mu, float* __restrict__ nu, int R, int k0,
                                              const gsr::AdamHyper& hy, Grad grad) {
    const size_t base = (size_t)i0 * R;
    const int total = cnt * R;
    const uint32_t inv = (1u << 20) / (uint32_t)R + 1u;  // e / R == (e * inv) >> 20 for e < 2^20 / R (R <= 45, e < 256 R)
    th += base; mu += base; nu += base;
    const bool aligned = ((((uintptr_t)th) | ((uintptr_t)mu) | ((uintptr_t)nu)) & 15) == 0;
    const int total4 = aligned ? total >> 2 : 0;
    auto element = [&](int e, float& t, float& m, float& v) {
        const int il = (int)(((uint32_t)e * inv) >> 20);
        const int j = e - il * R;
        const int kb = j / 3, c = j - 3 * kb, k = k0 + kb;
        const float g = grad(il, k, c);
        t = gsr::adam_update(t, g, m, v, hy);
        TS.shs[(size_t)(i0 + il) * K3 + 3 * k0 + j] = t;  // hcat(sh_color, sh_remainder) of the next forward
    };
    for (int f = threadIdx.x; f < total4; f += 256) {
        float4 t4 = reinterpret_cast<float4*>(th)[f], m4 = reinterpret_cast<float4*>(mu)[f],
               v4 = reinterpret_cast<float4*>(nu)[f];
        element(4 * f, t4.x, m4.x, v4.x);
        element(4 * f + 1, t4.y, m4.y, v4.y);
        element(4 * f + 2, t4.z, m4.z, v4.z);
        element(4 * f + 3, t4.w, m4.w, v4.w);
        reinterpret_cast<float4*>(th)[f] = t4;
        reinterpret_cast<float4*>(mu)[f] = m4;
        reinterpret_cast<float4*>(nu)[f] = v4;
    }
    for (int e = 4 * total4 + threadIdx.x; e < total; e += 256) {
        float t = th[e], m = mu[e], v = nu[e];
        element(e, t, m, v);
        th[e] = t; mu[e] = m; nu[e] = v;
    }
}

// The ∇shs rows of the cnt Gaussians of a workgroup starting at i0 (K3 = 3 K floats each): a lane's row is 12 K bytes apart
// from its neighbour's, so storing it directly is 3 K store instructions of 64 different cache lines each; the workgroup's
// slice is contiguous and goes out element-major as coalesced float4.  value(il, j): float j of the row of Gaussian il
// (0-based inside the workgroup), read from LDS.
template <class Value>
__device__ __forceinline__ void store_sh_rows(float* __restrict__ vshs, int i0, int cnt, int K3, Value value) {
    const uint32_t inv = (1u << 20) / (uint32_t)K3 + 1u;  // e / K3 == (e * inv) >> 20 for e < 2^20 / K3 (K3 <= 48, e < 256 K3)
    float* __restrict__ dst = vshs + (size_t)i0 * K3;
    const int total = cnt * K3;
    auto element = [&](int e) {
        const int il = (int)(((uint32_t)e * inv) >> 20);
        return value(il, e - il * K3);
    };
    const int total4 = (((uintptr_t)dst & 15) == 0) ? total >> 2 : 0;
    for (int f = threadIdx.x; f < total4; f += 256)
        reinterpret_cast<float4*>(dst)[f] = make_float4(element(4 * f), element(4 * f + 1), element(4 * f + 2), element(4 * f + 3));
    for (int e = 4 * total4 + threadIdx.x; e < total; e += 256) dst[e] = element(e);
}

// ... where only some rows are this launch's to write: keep(il) says whether Gaussian il's row is.  A float4 that spans the
// rows of two Gaussians goes out when either is kept (value() of the other's floats is what its own writer stores).
template <class Value, class Keep>
__device__ __forceinline__ void store_sh_rows_where(float* __restrict__ vshs, int i0, int cnt, int K3, Value value, Keep keep) {
    const uint32_t inv = (1u << 20) / (uint32_t)K3 + 1u;
    float* __restrict__ dst = vshs + (size_t)i0 * K3;
    const int total = cnt * K3;
    auto owner = [&](int e) { return (int)(((uint32_t)e * inv) >> 20); };
    auto element = [&](int e) {
        const int il = owner(e);
        return value(il, e - il * K3);
    };
    const int total4 = (((uintptr_t)dst & 15) == 0) ? total >> 2 : 0;
    for (int f = threadIdx.x; f < total4; f += 256)
        if (keep(owner(4 * f)) || keep(owner(4 * f + 3)))
            reinterpret_cast<float4*>(dst)[f] = make_float4(element(4 * f), element(4 * f + 1), element(4 * f + 2), element(4 * f + 3));
    for (int e = 4 * total4 + threadIdx.x; e < total; e += 256)
        if (keep(owner(e))) dst[e] = element(e);
}

}  // namespace gsr
