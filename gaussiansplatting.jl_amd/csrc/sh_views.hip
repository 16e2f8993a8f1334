// The factored SH-gradient exchange of the distributed trainer: ∇shs summed over a batch of views from the per-view
// colour cotangents, stored (sh_grad_views_kernel) or handed straight to the trainer tail (sh_views_tail_kernel).  A
// single-GPU step never launches these.
//
// Reference behaviour: src/rasterization/spherical_harmonics.jl:32-37, 41-48, training.jl:768-779.
//
// This translation unit is compiled with -ffp-contract=off: the sums and the Adam updates are the bits of the per-view
// backward (pergauss.hip) followed by the stand-alone tail (trainer.hip).
//
// bench.py's hashes of the kernel sources, which mark profiles/pmc_traffic.json stale, cover pergauss.hip and not this
// file: after a change here, run tools/measure_pmc.sh again.
#include "gsr_kernels.h"
#include "gsr_dispatch.h"
#include "splat_math.h"
#include "sh_rows.h"

namespace {
using namespace gsr::splat;
using gsr::dispatch_degree;
using gsr::store_sh_rows;
using gsr::tail_sh_group;

// ∇shs of a batch of views from the factored per-view colour cotangents:
//   vshs[i, k, c] = Σ_v basis_k(normalize(mean_i - center_v)) · vc_v[i, c]
// — exactly the ∇spherical_harmonics! coefficient gradient (spherical_harmonics.jl:32-37) of each
// view, summed over views in ascending view order on every rank.  The exchange then carries
// 3 floats per (Gaussian, view) instead of an all-reduce over 3K floats per Gaussian.
template <int DEG>
__global__ __launch_bounds__(256) void sh_grad_views_kernel(int n, int K, int n_views, const float* __restrict__ centers,
                                                            const float* __restrict__ means,
                                                            const float* __restrict__ vc_all,
                                                            float* __restrict__ vshs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    constexpr int NB = (DEG + 1) * (DEG + 1);
    float acc[3 * NB];
#pragma unroll
    for (int k = 0; k < 3 * NB; k++) acc[k] = 0.0f;
    if (i < n) {
        const float p[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
        for (int v = 0; v < n_views; v++) {
            const float* vcp = vc_all + ((size_t)v * n + i) * 3;
            const float vc[3] = {vcp[0], vcp[1], vcp[2]};
            if (vc[0] == 0.0f && vc[1] == 0.0f && vc[2] == 0.0f) continue;  // culled in this view (or zero cotangent)
            float d0[3], dir[3];
            view_dir(p, centers + 3 * v, d0, dir);
            float b[16];
            sh_basis<DEG>(dir, b);
#pragma unroll
            for (int k = 0; k < NB; k++)
#pragma unroll
                for (int c = 0; c < 3; c++) acc[3 * k + c] = acc[3 * k + c] + b[k] * vc[c];
        }
    }
    // The rows leave through LDS (store_sh_rows; same lesson as pergauss_bwd's ∇shs store).
    __shared__ float stage[256 * (3 * NB + 1)];  // odd stride: conflict-free
    constexpr int ST = 3 * NB + 1;
#pragma unroll
    for (int k = 0; k < 3 * NB; k++) stage[threadIdx.x * ST + k] = acc[k];
    __syncthreads();
    const int i0 = blockIdx.x * 256;
    // (bands above the active degree: zeros)
    store_sh_rows(vshs, i0, min(256, n - i0), 3 * K, [&](int il, int j) { return j < 3 * NB ? stage[il * ST + j] : 0.0f; });
}

// The multi-GPU trainer step made self-contained (training.jl:768-779): after the exchange of the
// factored arena — the 11·N small gradients all-reduced, the per-view colour cotangents all-gathered — ONE pass rebuilds
// Σ_v basis(dir_v) ⊗ vc_v per Gaussian (as sh_grad_views_kernel), keeps it in LDS instead of writing the 3K·N-float
// ∇shs, and applies the trainer tail right there: pullback of the functor prologue + the six NU.Adam updates + the
// activated copies of the next forward (adam_math.h / tail_sh_group: the definitions gsr_trainer_tail_step and the
// backward's fused epilogue use).  Bit-identical θ, μ, ν to gsr_sh_grad_from_views followed by gsr_trainer_tail_step;
// 192 B/Gaussian of gradient writes and reads less.  `S.points` are the means the directions are taken from; they are
// read before they are updated (same thread).
// (The loop over the views is written out in both kernels: as one __forceinline__ function template it costs DEG 3 20 VGPRs and
//  a wave per SIMD, 88 / 90 -> 108 / 109, and 67-71 instructions — profiles/pergauss_split/codegen_compare.txt.)
template <int DEG>
__global__ __launch_bounds__(256) void sh_views_tail_kernel(int n, int K, int n_views, const float* __restrict__ centers,
                                                            const float* __restrict__ vc_all,
                                                            const float* __restrict__ vmeans,
                                                            const float* __restrict__ vopac_act,
                                                            const float* __restrict__ vscales_act,
                                                            const float* __restrict__ vrot, gsr::TailState S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    constexpr int NB = (DEG + 1) * (DEG + 1);
    constexpr int ST = 3 * NB + 1;                 // odd stride: conflict-free
    __shared__ float stage[256 * ST];
    float acc[3 * NB];
#pragma unroll
    for (int k = 0; k < 3 * NB; k++) acc[k] = 0.0f;
    if (i < n) {
        const float p[3] = {S.points[3 * (size_t)i], S.points[3 * (size_t)i + 1], S.points[3 * (size_t)i + 2]};
        for (int v = 0; v < n_views; v++) {
            const float* vcp = vc_all + ((size_t)v * n + i) * 3;
            const float vc[3] = {vcp[0], vcp[1], vcp[2]};
            if (vc[0] == 0.0f && vc[1] == 0.0f && vc[2] == 0.0f) continue;  // culled in this view (or zero cotangent)
            float d0[3], dir[3];
            view_dir(p, centers + 3 * v, d0, dir);
            float b[16];
            sh_basis<DEG>(dir, b);
#pragma unroll
            for (int k = 0; k < NB; k++)
#pragma unroll
                for (int c = 0; c < 3; c++) acc[3 * k + c] = acc[3 * k + c] + b[k] * vc[c];
        }
    }
#pragma unroll
    for (int k = 0; k < 3 * NB; k++) stage[threadIdx.x * ST + k] = acc[k];
    if (i < n) {
        const float vm[3] = {vmeans[3 * (size_t)i], vmeans[3 * (size_t)i + 1], vmeans[3 * (size_t)i + 2]};
        const float vs[3] = {vscales_act[3 * (size_t)i], vscales_act[3 * (size_t)i + 1], vscales_act[3 * (size_t)i + 2]};
        const float vq[4] = {vrot[4 * (size_t)i], vrot[4 * (size_t)i + 1], vrot[4 * (size_t)i + 2], vrot[4 * (size_t)i + 3]};
        gsr::tail_gauss_apply(S, i, vm, vopac_act[i], vs, vq);
    }
    __syncthreads();
    const int i0 = blockIdx.x * 256, cnt = min(256, n - i0), K3 = 3 * K;
    auto grad = [&](int il, int k, int c) { return k < NB ? stage[il * ST + 3 * k + c] : 0.0f; };  // bands above the degree: 0
    tail_sh_group(S, i0, cnt, K3, S.dc, S.dc_mu, S.dc_nu, 3, 0, S.h_dc, grad);
    if (K > 1) tail_sh_group(S, i0, cnt, K3, S.rest, S.rest_mu, S.rest_nu, 3 * (K - 1), 1, S.h_rest, grad);
}

}  // namespace

void gsr_launch_sh_grad_views(hipStream_t s, int n, int K, int degree, int n_views, const float* centers,
                              const float* means, const float* vc_all, float* vshs) {
    if (n <= 0) return;
    dim3 grid((n + 255) / 256), block(256);
    dispatch_degree(degree, [&](auto d) {
        constexpr int DEG = d;
        hipLaunchKernelGGL(sh_grad_views_kernel<DEG>, grid, block, 0, s, n, K, n_views, centers, means, vc_all, vshs);
    });
}

void gsr_launch_sh_views_tail(hipStream_t s, int n, int K, int degree, int n_views, const float* centers,
                              const float* vc_all, const float* vmeans, const float* vopac_act, const float* vscales_act,
                              const float* vrot, const gsr::TailState& S) {
    if (n <= 0) return;
    dim3 grid((n + 255) / 256), block(256);
    dispatch_degree(degree, [&](auto d) {
        constexpr int DEG = d;
        hipLaunchKernelGGL(sh_views_tail_kernel<DEG>, grid, block, 0, s, n, K, n_views, centers, vc_all, vmeans, vopac_act,
                           vscales_act, vrot, S);
    });
}
