// The 3-D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024, §4.1), the world-space half of the pair whose screen-space
// half is GSR_FLAG_ANTIALIASED: every Gaussian is low-pass filtered by the highest rate at which any training
// camera samples it.  DESIGN.md §20.
//
//   sweep : all N points against all V cameras in one kernel.  A lane keeps F3D_PPL points in registers; the camera row is
//           read at a wave-uniform address (the loop counter alone: scalar loads), so a row costs one scalar fetch per wave
//           for 4 x 64 pairs.  Per pair, every operation is one rounded fp32 operation in this association
//           (-ffp-contract=off):
//               xc[i] = ((R[i]*p0 + R[i+3]*p1) + R[i+6]*p2) + t[i]     i = 0,1,2 ;  z = xc[2]
//               u[j]  = focal[j]*xc[j] + pp[j]*z                         j = 0,1
//               valid = (z > near) && (lo[j]*z <= u[j]) && (u[j] <= hi[j]*z) for both j     (any NaN: not valid)
//               tau   = z * inv_f
//           tmin = min of tau over the valid cameras, seen = some camera is valid, filter = k * tmin where seen.
//   final : ONE workgroup folds the per-workgroup maxima and counts of the sweep;
//   fill  : the points no camera saw get the largest filter of those that were seen (0 when none was).
// Minimum, maximum and the integer count are exact in any order: the result is the same bits in every run, whatever the
// reduction tree.  No atomics.
//
//   apply / apply_backward : the filter folded into the activated scales and opacities in front of `rasterize`, and its
//           pullback (the filter is a constant).  One lane per Gaussian.
#include "gsr_kernels.h"
#include "block_reduce.h"

namespace {

constexpr int F3D_THREADS = 256;
constexpr int F3D_PPL = 4;                              // points per lane
constexpr int F3D_WG_POINTS = F3D_THREADS * F3D_PPL;    // 1024
constexpr int F3D_CAM = 22;                             // GSR_FILTER3D_CAMERA_FLOATS (include/gsr.h)

__device__ __forceinline__ float wave_max_all(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// Maximum over a workgroup of four full waves, every thread gets it.  red: 4 floats of LDS.
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max_all(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// `seen` is never NULL here: the caller's array, or n bytes of the scratch.  An unseen point's filter is written as 0 and
// overwritten by the fill.
__global__ __launch_bounds__(F3D_THREADS) void filter3d_sweep_kernel(long long n, int n_cameras, const float* __restrict__ points,
                                                                     const float* __restrict__ cams, float near_plane, float k,
                                                                     float* __restrict__ filter, uint8_t* __restrict__ seen,
                                                                     float* __restrict__ part_max,
                                                                     uint32_t* __restrict__ part_cnt) {
    __shared__ float red_max[4];
    __shared__ uint32_t red_cnt[4];
    const long long base = (long long)blockIdx.x * F3D_WG_POINTS + threadIdx.x;
    const float inf = __builtin_inff();
    float p0[F3D_PPL], p1[F3D_PPL], p2[F3D_PPL], tmin[F3D_PPL];
    bool any[F3D_PPL];
#pragma unroll
    for (int u = 0; u < F3D_PPL; u++) {
        const long long p = base + (long long)u * F3D_THREADS;
        const size_t q = p < n ? (size_t)p : 0;   // (a lane past the end works on row 0 and stores nothing)
        p0[u] = points[3 * q]; p1[u] = points[3 * q + 1]; p2[u] = points[3 * q + 2];
        tmin[u] = inf;
        any[u] = false;
    }
    for (int v = 0; v < n_cameras; v++) {
        const float* __restrict__ c = cams + (size_t)v * F3D_CAM;   // wave-uniform: scalar loads
        const float R0 = c[0], R1 = c[1], R2 = c[2], R3 = c[3], R4 = c[4], R5 = c[5], R6 = c[6], R7 = c[7], R8 = c[8];
        const float t0 = c[9], t1 = c[10], t2 = c[11];
        const float f0 = c[12], f1 = c[13], pp0 = c[14], pp1 = c[15];
        const float lo0 = c[16], lo1 = c[17], hi0 = c[18], hi1 = c[19], inv_f = c[20];
#pragma unroll
        for (int u = 0; u < F3D_PPL; u++) {
            const float x = ((R0 * p0[u] + R3 * p1[u]) + R6 * p2[u]) + t0;
            const float y = ((R1 * p0[u] + R4 * p1[u]) + R7 * p2[u]) + t1;
            const float z = ((R2 * p0[u] + R5 * p1[u]) + R8 * p2[u]) + t2;
            const float u0 = f0 * x + pp0 * z;
            const float u1 = f1 * y + pp1 * z;
            const bool valid = (z > near_plane) && (lo0 * z <= u0) && (u0 <= hi0 * z) && (lo1 * z <= u1) && (u1 <= hi1 * z);
            const float tau = z * inv_f;
            tmin[u] = valid ? fminf(tmin[u], tau) : tmin[u];
            any[u] = any[u] || valid;
        }
    }
    float wmax = -inf;
    uint32_t cnt = 0;
#pragma unroll
    for (int u = 0; u < F3D_PPL; u++) {
        const long long p = base + (long long)u * F3D_THREADS;
        if (p < n) {
            const float f = k * tmin[u];
            filter[p] = any[u] ? f : 0.0f;
            seen[p] = any[u] ? 1 : 0;
            if (any[u]) {
                wmax = fmaxf(wmax, f);
                cnt++;
            }
        }
    }
    wmax = block_max(wmax, red_max);
    cnt = gsr::block_sum<uint32_t, 4>(cnt, red_cnt);
    if (threadIdx.x == 0) {
        part_max[blockIdx.x] = wmax;
        part_cnt[blockIdx.x] = cnt;
    }
}

// ONE workgroup: fill[0] <- the largest filter of the seen points (0 when there is none), *count_out <- how many were seen.
__global__ __launch_bounds__(F3D_THREADS) void filter3d_final_kernel(int n_wg, const float* __restrict__ part_max,
                                                                     const uint32_t* __restrict__ part_cnt,
                                                                     float* __restrict__ fill, uint32_t* __restrict__ count_out) {
    __shared__ float red_max[4];
    __shared__ uint32_t red_cnt[4];
    float m = -__builtin_inff();
    uint32_t cnt = 0;
    for (int i = threadIdx.x; i < n_wg; i += F3D_THREADS) {
        m = fmaxf(m, part_max[i]);
        cnt += part_cnt[i];
    }
    m = block_max(m, red_max);
    cnt = gsr::block_sum<uint32_t, 4>(cnt, red_cnt);
    if (threadIdx.x == 0) {
        fill[0] = cnt ? m : 0.0f;
        if (count_out) *count_out = cnt;
    }
}

__global__ __launch_bounds__(F3D_THREADS) void filter3d_fill_kernel(long long n, const uint8_t* __restrict__ seen,
                                                                    const float* __restrict__ fill, float* __restrict__ filter) {
    const long long p = (long long)blockIdx.x * F3D_THREADS + threadIdx.x;
    if (p < n && !seen[p]) filter[p] = fill[0];
}

// What both apply kernels form of one row: se[i] = sqrtf(s[i]*s[i] + f*f), r[i] = s[i] / se[i].
struct F3dRow {
    float s[3], se[3], r[3], f2;
};
__device__ __forceinline__ F3dRow f3d_row(const float* __restrict__ scales, const float* __restrict__ filter, size_t p) {
    F3dRow w;
    const float f = filter[p];
    w.f2 = f * f;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        w.s[i] = scales[3 * p + i];
        w.se[i] = sqrtf(w.s[i] * w.s[i] + w.f2);
        w.r[i] = w.s[i] / w.se[i];
    }
    return w;
}

// RAW: logf(se[i]) and the logit of o_eff, the values a .ply holds.  1 - o_eff is formed without the cancellation of
// 1 - o*c near o_eff = 1: 1 - r[i] = f2 / (se[i]*(se[i] + s[i])), 1 - c = (1-r0) + r0*((1-r1) + r1*(1-r2)), a sum of
// non-negative terms, and 1 - o*c = (1 - o) + o*(1 - c).
template <bool RAW>
__global__ __launch_bounds__(F3D_THREADS) void filter3d_apply_kernel(long long n, const float* __restrict__ opac,
                                                                     const float* __restrict__ scales,
                                                                     const float* __restrict__ filter, float* __restrict__ opac_out,
                                                                     float* __restrict__ scales_out) {
    const long long pl = (long long)blockIdx.x * F3D_THREADS + threadIdx.x;
    if (pl >= n) return;
    const size_t p = (size_t)pl;
    const F3dRow w = f3d_row(scales, filter, p);
    const float o = opac[p];
    const float c = (w.r[0] * w.r[1]) * w.r[2];
    const float oe = o * c;
    if (RAW) {
        float d[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            d[i] = w.f2 / (w.se[i] * (w.se[i] + w.s[i]));
            scales_out[3 * p + i] = logf(w.se[i]);
        }
        const float one_minus_c = d[0] + w.r[0] * (d[1] + w.r[1] * d[2]);
        const float one_minus_oe = (1.0f - o) + o * one_minus_c;
        opac_out[p] = logf(oe / one_minus_oe);
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++) scales_out[3 * p + i] = w.se[i];
        opac_out[p] = oe;
    }
}

// vo = g_o * c ;  vs[i] = g_s[i]*r[i] + ((g_o*o)*P[i]) * (f2 / ((se[i]*se[i])*se[i])),  P[i] the product of the other two r.
// v_opac / v_scales may be g_opac / g_scales (no __restrict__ on the four): a lane reads its row before it writes it.
__global__ __launch_bounds__(F3D_THREADS) void filter3d_apply_bwd_kernel(long long n, const float* __restrict__ opac,
                                                                         const float* __restrict__ scales,
                                                                         const float* __restrict__ filter, const float* g_opac,
                                                                         const float* g_scales, float* v_opac, float* v_scales) {
    const long long pl = (long long)blockIdx.x * F3D_THREADS + threadIdx.x;
    if (pl >= n) return;
    const size_t p = (size_t)pl;
    const F3dRow w = f3d_row(scales, filter, p);
    const float o = opac[p];
    const float go = g_opac[p];
    const float gs[3] = {g_scales[3 * p], g_scales[3 * p + 1], g_scales[3 * p + 2]};
    const float c = (w.r[0] * w.r[1]) * w.r[2];
    const float P[3] = {w.r[1] * w.r[2], w.r[0] * w.r[2], w.r[0] * w.r[1]};
    const float goo = go * o;
    float vs[3];
#pragma unroll
    for (int i = 0; i < 3; i++) vs[i] = gs[i] * w.r[i] + (goo * P[i]) * (w.f2 / ((w.se[i] * w.se[i]) * w.se[i]));
    v_opac[p] = go * c;
#pragma unroll
    for (int i = 0; i < 3; i++) v_scales[3 * p + i] = vs[i];
}

inline long long f3d_workgroups(long long n) { return (n + F3D_WG_POINTS - 1) / F3D_WG_POINTS; }
inline size_t f3d_align8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

// scratch (8-byte aligned): the fill value (8 bytes), the per-workgroup maxima and counts of the sweep, n `seen` bytes
size_t gsr_filter3d_scratch_size(long long n) {
    if (n <= 0) return 0;
    return 8 + f3d_align8((size_t)f3d_workgroups(n) * 8) + (size_t)n;
}

void gsr_launch_filter3d_compute(hipStream_t s, long long n, const float* points, int n_cameras, const float* cams,
                                 float near_plane, float k, float* filter, uint8_t* seen, uint32_t* count, void* scratch) {
    if (n <= 0) return;
    const int n_wg = (int)f3d_workgroups(n);
    float* fill = reinterpret_cast<float*>(scratch);
    float* part_max = fill + 2;
    uint32_t* part_cnt = reinterpret_cast<uint32_t*>(part_max + n_wg);
    uint8_t* seen_s = reinterpret_cast<uint8_t*>(scratch) + 8 + f3d_align8((size_t)n_wg * 8);
    uint8_t* seen_w = seen ? seen : seen_s;
    hipLaunchKernelGGL(filter3d_sweep_kernel, dim3((unsigned)n_wg), dim3(F3D_THREADS), 0, s, n, n_cameras, points, cams,
                       near_plane, k, filter, seen_w, part_max, part_cnt);
    hipLaunchKernelGGL(filter3d_final_kernel, dim3(1), dim3(F3D_THREADS), 0, s, n_wg, part_max, part_cnt, fill, count);
    const unsigned blocks = (unsigned)((n + F3D_THREADS - 1) / F3D_THREADS);
    hipLaunchKernelGGL(filter3d_fill_kernel, dim3(blocks), dim3(F3D_THREADS), 0, s, n, seen_w, fill, filter);
}

void gsr_launch_filter3d_apply(hipStream_t s, long long n, const float* opac, const float* scales, const float* filter, int raw,
                               float* opac_out, float* scales_out) {
    if (n <= 0) return;
    const unsigned blocks = (unsigned)((n + F3D_THREADS - 1) / F3D_THREADS);
    if (raw)
        hipLaunchKernelGGL(filter3d_apply_kernel<true>, dim3(blocks), dim3(F3D_THREADS), 0, s, n, opac, scales, filter, opac_out,
                           scales_out);
    else
        hipLaunchKernelGGL(filter3d_apply_kernel<false>, dim3(blocks), dim3(F3D_THREADS), 0, s, n, opac, scales, filter, opac_out,
                           scales_out);
}

void gsr_launch_filter3d_apply_bwd(hipStream_t s, long long n, const float* opac, const float* scales, const float* filter,
                                   const float* g_opac, const float* g_scales, float* v_opac, float* v_scales) {
    if (n <= 0) return;
    const unsigned blocks = (unsigned)((n + F3D_THREADS - 1) / F3D_THREADS);
    hipLaunchKernelGGL(filter3d_apply_bwd_kernel, dim3(blocks), dim3(F3D_THREADS), 0, s, n, opac, scales, filter, g_opac,
                       g_scales, v_opac, v_scales);
}
