// Sky dome, the per-pixel part (src/sky_dome.jl:246-250 `composite_sky`, :217-228 `composite_sky!`, :315-320
// `sky_opacity_loss`; `step!`, training.jl:634-639,673-676,721-725): the dome's :rgb render composited behind the scene's
// frame, the sky-mask loss on the scene's alpha, and the pullback of both.  The scene frame is the rasterizer's (C,W,H)
// image, C = 5 or 8, rendered over a ZERO background: channels 0-2 rgb, 4 alpha (raw, never clamped: a saturated pixel keeps
// its gradient, sky_dome.jl:306-309); the sky frame is (3,W,H); the mask is (W,H) in [0, 1].
// Compiled with -ffp-contract=off: every product and sum below is its own fp32 operation, in the order written.
//
// One pixel per lane and load: a wave's loads of one channel touch 64 consecutive 20 / 32 / 12-byte records (in memory
// order), and the loads of the other channels of the same records use up the same lines.  The backward takes 256 pixels per
// workgroup; the forward takes 1024 — a thread's pixels are i, i + 256, i + 512, i + 768 of its workgroup's — so that the
// one-workgroup final pass, whose threads walk the partials one dependent load at a time, has a quarter of the rows.
//
//   forward : t = 1 - alpha;  out[c] = image[c] + t * sky[c], c = 0..2 (a product, then a sum);  channels >= 3 are copied
//             when out is not the frame itself (elementwise: out == image is the in-place form).  With a mask, the
//             workgroup's partials of Σw and Σ w·alpha² in double: per pixel (double)w and (double)w · ((double)alpha ·
//             (double)alpha); a thread adds its four pixels in ascending order, ((x0 + x1) + x2) + x3, a pixel past the end
//             counting 0.0; the 256 thread sums go through gsr::block_sum (xor butterfly per wave, then the four waves in
//             order).
//   final   : one workgroup, gsr::sum_partials (block_reduce.h: each thread its rows ascending, then thread 0 the 256
//             thread sums ascending) -> d = max(Σw, 1);  scratch[0] = (float)(1 / d);  loss = loss_weight ·
//             (float)(Σ w·alpha² / d).  A mask of zeros gives exactly 0: no division by zero.
//   backward: g = vpixels[0..2] (the cotangent of the composite; left as it is: ∂composite/∂image = 1);  t = 1 - alpha;
//             vsky[c] = t * g[c];  dot = (g0 * sky0 + g1 * sky1) + g2 * sky2;
//             without a mask  vpixels[4] = vpixels[4] + (-dot)
//             with a mask     m = ((2 * w) * alpha) * (loss_weight * scratch[0]);  vpixels[4] = vpixels[4] + ((-dot) + m)
//             — ONE add onto what the channel held, so this pass and the depth / normal terms compose in either order to
//             the rounding of that add.  Channels 0-3 and >= 5 of vpixels are not written.
// No float atomics; every result is run-to-run bit-identical; every scratch word that is read was written by the forward.
#include "gsr_kernels.h"
#include "block_reduce.h"

namespace {

constexpr int THREADS = 256;
constexpr int FWD_PIXELS = 4;  // pixels per thread of the forward
constexpr size_t HEAD_BYTES = 16;  // scratch: [0] float 1/max(Σw, 1), padding, then 2 doubles per workgroup of the forward

// (the kernels are not called sky_composite_*: tests/test_gpu_poisoned_buffers.py finds composite.hip's instantiations by
// their names in the library's symbols, and a name that ends in one of them would be counted among them)
// image and out may be the same array: no __restrict__ on either
template <int C>
__global__ __launch_bounds__(THREADS) void sky_behind_fwd_kernel(size_t n, const float* image, const float* __restrict__ sky,
                                                                    const float* __restrict__ mask, float* out,
                                                                    double* __restrict__ partial) {
    __shared__ double red[4];
    const size_t first = (size_t)blockIdx.x * (THREADS * FWD_PIXELS) + threadIdx.x;
    double s_w = 0.0, s_wa = 0.0;
#pragma unroll
    for (int k = 0; k < FWD_PIXELS; k++) {
        const size_t i = first + (size_t)k * THREADS;
        if (i >= n) break;
        const float* p = image + i * C;
        float v[C];
#pragma unroll
        for (int c = 0; c < C; c++) v[c] = p[c];
        const float s0 = sky[i * 3 + 0], s1 = sky[i * 3 + 1], s2 = sky[i * 3 + 2];
        const float alpha = v[4], t = 1.0f - alpha;
        float* o = out + i * C;
        o[0] = v[0] + t * s0;
        o[1] = v[1] + t * s1;
        o[2] = v[2] + t * s2;
        if (out != image) {
#pragma unroll
            for (int c = 3; c < C; c++) o[c] = v[c];
        }
        if (mask) {
            const double w = (double)mask[i], a = (double)alpha;
            s_w += w;
            s_wa += w * (a * a);
        }
    }
    if (!mask) return;  // uniform over the grid
    s_w = gsr::block_sum<double>(s_w, red);
    s_wa = gsr::block_sum<double>(s_wa, red);
    if (threadIdx.x == 0) {
        partial[(size_t)blockIdx.x * 2 + 0] = s_w;
        partial[(size_t)blockIdx.x * 2 + 1] = s_wa;
    }
}

__global__ __launch_bounds__(THREADS) void sky_final_kernel(int n_partial, const double* __restrict__ partial, float loss_weight,
                                                            float* __restrict__ loss_out, float* __restrict__ head) {
    __shared__ double red[2][256];
    double s[2];
    gsr::sum_partials<2>(n_partial, partial, red, s);
    if (threadIdx.x != 0) return;
    const double d = s[0] > 1.0 ? s[0] : 1.0;
    head[0] = (float)(1.0 / d);
    *loss_out = loss_weight * (float)(s[1] / d);
}

template <int C>
__global__ __launch_bounds__(THREADS) void sky_behind_bwd_kernel(size_t n, const float* __restrict__ image,
                                                                    const float* __restrict__ sky, const float* __restrict__ mask,
                                                                    float loss_weight, const float* __restrict__ head,
                                                                    float* __restrict__ vpixels, float* __restrict__ vsky) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    float* vp = vpixels + i * C;
    const float g0 = vp[0], g1 = vp[1], g2 = vp[2], v4 = vp[4];
    const float s0 = sky[i * 3 + 0], s1 = sky[i * 3 + 1], s2 = sky[i * 3 + 2];
    const float alpha = image[i * C + 4], t = 1.0f - alpha;
    vsky[i * 3 + 0] = t * g0;
    vsky[i * 3 + 1] = t * g1;
    vsky[i * 3 + 2] = t * g2;
    const float dot = (g0 * s0 + g1 * s1) + g2 * s2;
    float add = -dot;
    if (mask) {
        const float k = loss_weight * head[0];
        add = add + ((2.0f * mask[i]) * alpha) * k;
    }
    vp[4] = v4 + add;
}

unsigned blocks_of(size_t n, int per_thread = 1) {
    const size_t tile = (size_t)THREADS * per_thread;
    return (unsigned)((n + tile - 1) / tile);
}

}  // namespace

size_t gsr_sky_scratch_size(int W, int H) {
    return HEAD_BYTES + (size_t)blocks_of((size_t)W * H, FWD_PIXELS) * 2 * sizeof(double);
}

void gsr_launch_sky_composite_fwd(hipStream_t s, int W, int H, int C, const float* image, const float* sky_rgb,
                                  const float* sky_weight, float loss_weight, float* out, float* loss_out, void* scratch) {
    const size_t n = (size_t)W * H;
    const unsigned nb = blocks_of(n, FWD_PIXELS);
    double* partial = sky_weight ? (double*)((char*)scratch + HEAD_BYTES) : nullptr;
    if (C == 5)
        hipLaunchKernelGGL(sky_behind_fwd_kernel<5>, dim3(nb), dim3(THREADS), 0, s, n, image, sky_rgb, sky_weight, out, partial);
    else
        hipLaunchKernelGGL(sky_behind_fwd_kernel<8>, dim3(nb), dim3(THREADS), 0, s, n, image, sky_rgb, sky_weight, out, partial);
    if (sky_weight)
        hipLaunchKernelGGL(sky_final_kernel, dim3(1), dim3(THREADS), 0, s, (int)nb, partial, loss_weight, loss_out, (float*)scratch);
}

void gsr_launch_sky_composite_bwd(hipStream_t s, int W, int H, int C, const float* image, const float* sky_rgb,
                                  const float* sky_weight, float loss_weight, float* vpixels, float* vsky, const void* scratch) {
    const size_t n = (size_t)W * H;
    const unsigned nb = blocks_of(n);
    if (C == 5)
        hipLaunchKernelGGL(sky_behind_bwd_kernel<5>, dim3(nb), dim3(THREADS), 0, s, n, image, sky_rgb, sky_weight, loss_weight,
                           (const float*)scratch, vpixels, vsky);
    else
        hipLaunchKernelGGL(sky_behind_bwd_kernel<8>, dim3(nb), dim3(THREADS), 0, s, n, image, sky_rgb, sky_weight, loss_weight,
                           (const float*)scratch, vpixels, vsky);
}
