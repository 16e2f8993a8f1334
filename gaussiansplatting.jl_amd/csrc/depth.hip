// Anchored depth supervision of :rgbd / :rgbdn training (src/depth_supervision.jl:406-536; `use_depth_loss`, `step!`
// training.jl:604-620,709-718): `depth_target` and `ssi_depth_loss` over a rendered (C,W,H) frame, C = 5 or 8, of which
// only channel 3 (blended depth D) and channel 4 (alpha) are read, and the pullback onto those two channels of the
// frame's cotangent.  Compiled with -ffp-contract=off: every mask decision (valid, far_extrap, the deadband) is the
// reference's own fp32 expression, so the masks are a function of the inputs and not of the arithmetic mode.
//
// Passes.  All of them run on 64x16 tiles, one workgroup of 256 threads per tile, four rows per thread:
//   1. stats  : frame + prior -> the per-pixel record (p, target, half_band, ±w) in scratch, 16 B per pixel, and the
//               tile's partials of Σα, Σw_s, Σw_s·p, Σw_s·p² in double.  The sign of the fourth field carries far_extrap:
//               w_s = w where it is positive, 0 where it is negative.
//   2. header : one workgroup sums the partials in index order (strided per thread, then an LDS tree) and writes
//               Σα' = max(Σα, 1), Σα, Σw_s, μ, σ = max(√max(var, 0), 1e-6), iscale = 1 / (2σ).  The variance comes from the
//               moments in double: fp32 values squared are exact in double, and var/μ² of a depth map is far above 2^-53.
//   3. loss   : stages the tile's records with one more column and row in LDS; every pixel evaluates its data term and
//               the x- and y-pair it leads; partials in double.
//   4. final  : the partials in index order -> weight · (data + λ(gx + gy)) / Σα', and stats_out.
//   backward  : stages the records with a 1-pixel ring; a pixel's ∂/∂p is its own data term, the x-pair it leads, the
//               x-pair it trails, then the same for y, summed in this order (a gather: no atomics), then the quotient
//               rule onto D and alpha, ADDED onto channels 3 and 4 of vpixels.
// Later passes stream the 16-byte records instead of the 20 / 32-byte frame records plus the prior.
//
// Intended deviation from the reference (the same as the depth-normal term's): a pixel with w = 0 contributes exactly
// nothing to the loss, to σ and to the gradients, also when its D or its prior is NaN / Inf (the reference's `sum(w .* ...)`
// would turn NaN on 0 · NaN); its record is written as zeros.  So does a pair whose min(w_s, w_s') = 0.  A non-finite alpha
// counts as 0 in Σα.  No float atomics anywhere; every result is run-to-run bit-identical; every scratch word that is
// read was written by an earlier pass of the same call.
#include "gsr_kernels.h"
#include "block_reduce.h"

namespace {

constexpr float MIN_ALPHA = 1e-3f, ALPHA_FLOOR = 1e-6f, RESIDUAL_SCALE = 2.0f;  // depth_supervision.jl:19-20, :495
constexpr int TX = 64, TY = 16, THREADS = 256;
constexpr int N_STAT = 4, N_LOSS = 3, HEAD_FLOATS = 16;

struct Anchor { float a, b, floor, disparity, p_far; };

// `depth_target` of one pixel (depth_supervision.jl:425-438).  Julia's min keeps a NaN: so does the select.
__device__ __forceinline__ void target_of(const Anchor& an, float qstep, float t, float& target, float& half_band, bool& valid,
                                          bool& far_extrap) {
    const float affine = an.a * t + an.b;
    valid = isfinite(t) && t > 0.0f && affine > 0.0f;
    const float half_step = 0.5f * qstep * fabsf(an.a);
    if (an.disparity > 0.0f) {
        const float cap = 1.0f / an.floor;
        target = affine > cap ? cap : affine;
        half_band = half_step;
    } else {
        target = 1.0f / (affine + an.floor);
        half_band = half_step * (target * target);
    }
    far_extrap = target < an.p_far;
}

__device__ __forceinline__ float deadband(float r, float half) {
    const float m = fabsf(r) - half;
    return m <= 0.0f ? 0.0f : copysignf(m, r);  // a NaN residual stays NaN, as in sign(r)·max(|r| - half, 0)
}
__device__ __forceinline__ float geman_mcclure(float x) { const float x2 = x * x; return 0.5f * x2 / (1.0f + x2); }
__device__ __forceinline__ float geman_mcclure_d(float x) { const float q = 1.0f + x * x; return x / (q * q); }

// the target maps alone (`depth_target`): one thread per pixel
__global__ __launch_bounds__(THREADS) void depth_target_kernel(size_t n, const float* __restrict__ prior, Anchor an, float qstep,
                                                               float* __restrict__ target_out, float* __restrict__ half_out,
                                                               uint8_t* __restrict__ flags_out) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    float target, half;
    bool valid, far;
    target_of(an, qstep, prior[i], target, half, valid, far);
    if (target_out) target_out[i] = target;
    if (half_out) half_out[i] = half;
    if (flags_out) flags_out[i] = (uint8_t)((valid ? 1 : 0) | (far ? 2 : 0));
}

// ---- pass 1: records + partials of (Σα, Σw_s, Σw_s·p, Σw_s·p²) ----
__global__ __launch_bounds__(THREADS) void depth_stats_kernel(int W, int H, int C, const float* __restrict__ image,
                                                              const float* __restrict__ prior, Anchor an, float qstep,
                                                              float* __restrict__ target_out, float* __restrict__ half_out,
                                                              uint8_t* __restrict__ flags_out, float4* __restrict__ rec,
                                                              double* __restrict__ partial) {
    __shared__ double red[4];
    const int x = blockIdx.x * TX + (threadIdx.x & 63);
    double s_a = 0.0, s_w = 0.0, s_wp = 0.0, s_wpp = 0.0;
#pragma unroll
    for (int k = 0; k < TY / 4; k++) {
        const int y = blockIdx.y * TY + (threadIdx.x >> 6) + 4 * k;
        if (x >= W || y >= H) continue;
        const size_t i = (size_t)y * W + x;
        const float d = image[i * C + 3], alpha = image[i * C + 4];
        float target, half;
        bool valid, far;
        target_of(an, qstep, prior[i], target, half, valid, far);
        if (target_out) target_out[i] = target;
        if (half_out) half_out[i] = half;
        if (flags_out) flags_out[i] = (uint8_t)((valid ? 1 : 0) | (far ? 2 : 0));
        // clamp(alpha, 0, 1); a non-finite alpha counts as 0, in Σα and as a weight
        const float ac = !isfinite(alpha) ? 0.0f : (alpha > 1.0f ? 1.0f : (alpha > 0.0f ? alpha : 0.0f));
        s_a += (double)ac;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (valid && ac > MIN_ALPHA) {
            const float p = 1.0f / (d / (alpha < ALPHA_FLOOR ? ALPHA_FLOOR : alpha) + an.floor);
            r = make_float4(p, target, half, far ? -ac : ac);
            if (!far) {
                const double w = (double)ac, pd = (double)p;
                s_w += w;
                s_wp += w * pd;
                s_wpp += w * pd * pd;
            }
        }
        rec[i] = r;
    }
    s_a = gsr::block_sum<double>(s_a, red);
    s_w = gsr::block_sum<double>(s_w, red);
    s_wp = gsr::block_sum<double>(s_wp, red);
    s_wpp = gsr::block_sum<double>(s_wpp, red);
    if (threadIdx.x == 0) {
        double* p = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * N_STAT;
        p[0] = s_a; p[1] = s_w; p[2] = s_wp; p[3] = s_wpp;
    }
}

// N sums of the partials (n_partial rows of N doubles): each thread its rows in index order, then a tree over the threads.
// The one TREE-ordered final pass: every other one is gsr::sum_partials (block_reduce.h), which adds the 256 thread sums
// serially.  The two orders round double sums differently, so folding this one into it would move the loss, μ and σ.
template <int N>
__device__ __forceinline__ void sum_partials(int n_partial, const double* __restrict__ partial, double (*red)[THREADS], double* s) {
#pragma unroll
    for (int a = 0; a < N; a++) s[a] = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += THREADS)
#pragma unroll
        for (int a = 0; a < N; a++) s[a] += partial[(size_t)i * N + a];
#pragma unroll
    for (int a = 0; a < N; a++) red[a][threadIdx.x] = s[a];
    __syncthreads();
    for (int off = THREADS / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off)
#pragma unroll
            for (int a = 0; a < N; a++) red[a][threadIdx.x] += red[a][threadIdx.x + off];
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < N; a++) s[a] = red[a][0];
}

// ---- pass 2: head = (Σα', Σα, Σw_s, μ, σ, iscale) (depth_supervision.jl:485, :506-511) ----
__global__ __launch_bounds__(THREADS) void depth_header_kernel(int n_partial, const double* __restrict__ partial, float* head) {
    __shared__ double red[N_STAT][THREADS];
    double s[N_STAT];
    sum_partials<N_STAT>(n_partial, partial, red, s);
    if (threadIdx.x != 0) return;
    const double sw = s[1] > 1e-6 ? s[1] : 1e-6;
    const double mu = s[2] / sw;
    const double var = (s[3] - 2.0 * mu * s[2] + mu * mu * s[1]) / sw;
    const double sd = sqrt(var > 0.0 ? var : 0.0);
    const float sigma = sd > 1e-6 ? (float)sd : 1e-6f;
    head[0] = (float)(s[0] > 1.0 ? s[0] : 1.0);
    head[1] = (float)s[0];
    head[2] = (float)s[1];
    head[3] = (float)mu;
    head[4] = sigma;
    head[5] = 1.0f / (RESIDUAL_SCALE * sigma);
}

// records of the tile at (x0, y0) with LO pixels before and one pixel after it -> LDS; zeros outside the image
template <int LO>
__device__ __forceinline__ void stage_records(const float4* __restrict__ rec, int W, int H, int x0, int y0, float4* sr) {
    constexpr int SW = TX + LO + 1, SH = TY + LO + 1;
    for (int i = threadIdx.x; i < SW * SH; i += THREADS) {
        const int ly = i / SW, lx = i - ly * SW;
        const int x = x0 - LO + lx, y = y0 - LO + ly;
        sr[i] = (x >= 0 && x < W && y >= 0 && y < H) ? rec[(size_t)y * W + x] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

__device__ __forceinline__ float supported(const float4& r) { return r.w > 0.0f ? r.w : 0.0f; }

// the data term's residual, already scaled: one-sided on far_extrap pixels (depth_supervision.jl:515-516)
__device__ __forceinline__ float data_x(const float4& r, float iscale) {
    float v = deadband(r.x - r.y, r.z);
    if (r.w < 0.0f && v < 0.0f) v = 0.0f;
    return v * iscale;
}
// a forward-difference pair, `a` leads `b` (depth_supervision.jl:521-533): its weight (0: the pair takes no part)
__device__ __forceinline__ float pair_x(const float4& a, const float4& b, float iscale, float& w) {
    const float wa = supported(a), wb = supported(b);
    w = wa < wb ? wa : wb;
    const float h = (b.x - a.x) - (b.y - a.y);
    return deadband(h, b.z + a.z) * iscale;
}

// ---- pass 3: partials of (data, grad_x, grad_y) ----
__global__ __launch_bounds__(THREADS) void depth_loss_kernel(int W, int H, const float4* __restrict__ rec,
                                                             const float* __restrict__ head, double* __restrict__ partial) {
    constexpr int SW = TX + 1;
    __shared__ float4 sr[SW * (TY + 1)];
    __shared__ double red[4];
    const float iscale = head[5];
    stage_records<0>(rec, W, H, blockIdx.x * TX, blockIdx.y * TY, sr);
    __syncthreads();
    const int lx = threadIdx.x & 63;
    double s_d = 0.0, s_x = 0.0, s_y = 0.0;
#pragma unroll
    for (int k = 0; k < TY / 4; k++) {
        const int ly = (threadIdx.x >> 6) + 4 * k;
        const float4 c = sr[ly * SW + lx];
        if (c.w == 0.0f) continue;  // w = 0 (or outside the image): no data term, and every pair it is in weighs 0
        s_d += (double)(fabsf(c.w) * geman_mcclure(data_x(c, iscale)));
        float w;
        const float hx = pair_x(c, sr[ly * SW + lx + 1], iscale, w);
        if (w > 0.0f) s_x += (double)(w * geman_mcclure(hx));
        const float hy = pair_x(c, sr[(ly + 1) * SW + lx], iscale, w);
        if (w > 0.0f) s_y += (double)(w * geman_mcclure(hy));
    }
    s_d = gsr::block_sum<double>(s_d, red);
    s_x = gsr::block_sum<double>(s_x, red);
    s_y = gsr::block_sum<double>(s_y, red);
    if (threadIdx.x == 0) {
        double* p = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * N_LOSS;
        p[0] = s_d; p[1] = s_x; p[2] = s_y;
    }
}

// ---- pass 4: the loss (depth_supervision.jl:535) and stats_out = (Σα, Σw_s, μ, σ) ----
__global__ __launch_bounds__(THREADS) void depth_final_kernel(int n_partial, const double* __restrict__ partial,
                                                              const float* __restrict__ head, float lambda_grad, float weight,
                                                              float* loss_out, float* stats_out) {
    __shared__ double red[N_LOSS][THREADS];
    double s[N_LOSS];
    sum_partials<N_LOSS>(n_partial, partial, red, s);
    if (threadIdx.x != 0) return;
    *loss_out = weight * (float)((s[0] + (double)lambda_grad * (s[1] + s[2])) / (double)head[0]);
    if (stats_out) {
        stats_out[0] = head[1]; stats_out[1] = head[2]; stats_out[2] = head[3]; stats_out[3] = head[4];
    }
}

// ---- backward: adds weight · ∂loss/∂(D, alpha) onto channels 3, 4 of vpixels ----
__global__ __launch_bounds__(THREADS) void depth_bwd_kernel(int W, int H, int C, const float* __restrict__ image,
                                                            const float4* __restrict__ rec, const float* __restrict__ head,
                                                            float lambda_grad, float weight, float* __restrict__ vpixels) {
    constexpr int SW = TX + 2;
    __shared__ float4 sr[SW * (TY + 2)];
    const float iscale = head[5];
    const float k = weight / head[0];
    if (k == 0.0f) return;  // a zero weight adds nothing: vpixels is not touched
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    stage_records<1>(rec, W, H, x0, y0, sr);
    __syncthreads();
    const int lx = threadIdx.x & 63, x = x0 + lx;
#pragma unroll
    for (int j = 0; j < TY / 4; j++) {
        const int ly = (threadIdx.x >> 6) + 4 * j, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int s = (ly + 1) * SW + lx + 1;
        const float4 c = sr[s];
        if (c.w == 0.0f) continue;  // w = 0: no term reaches this pixel
        // ∂/∂p of: the data term, the x-pair it leads, the x-pair it trails, the y-pair it leads, the y-pair it trails
        const float t0 = fabsf(c.w) * geman_mcclure_d(data_x(c, iscale));
        float w, h;
        h = pair_x(c, sr[s + 1], iscale, w);
        const float t1 = w > 0.0f ? -(w * geman_mcclure_d(h)) : 0.0f;
        h = pair_x(sr[s - 1], c, iscale, w);
        const float t2 = w > 0.0f ? w * geman_mcclure_d(h) : 0.0f;
        h = pair_x(c, sr[s + SW], iscale, w);
        const float t3 = w > 0.0f ? -(w * geman_mcclure_d(h)) : 0.0f;
        h = pair_x(sr[s - SW], c, iscale, w);
        const float t4 = w > 0.0f ? w * geman_mcclure_d(h) : 0.0f;
        const float g = (k * iscale) * (t0 + lambda_grad * (((t1 + t2) + t3) + t4));
        if (g == 0.0f) continue;  // inside every deadband: nothing is added
        const size_t i = ((size_t)y * W + x) * C;
        const float d = image[i + 3], alpha = image[i + 4];
        const float gp2 = g * (c.x * c.x);
        vpixels[i + 3] += -(gp2 / (alpha < ALPHA_FLOOR ? ALPHA_FLOOR : alpha));  // ∂p/∂D = -p² / max(α, 1e-6)
        if (alpha > ALPHA_FLOOR) vpixels[i + 4] += gp2 * d / (alpha * alpha);    // ∂p/∂α = p²·D/α² · [α > 1e-6]
    }
}

dim3 tile_grid(int W, int H) { return dim3((unsigned)((W + TX - 1) / TX), (unsigned)((H + TY - 1) / TY)); }
Anchor make_anchor(const float* a) { return Anchor{a[0], a[1], a[2], a[3], a[4]}; }

// scratch: header | stats partials | loss partials | records (16-byte aligned)
struct Layout { size_t stats, loss, rec, total; };
Layout layout(int W, int H) {
    const dim3 g = tile_grid(W, H);
    const size_t nt = (size_t)g.x * g.y;
    Layout l;
    l.stats = HEAD_FLOATS * sizeof(float);
    l.loss = l.stats + nt * N_STAT * sizeof(double);
    l.rec = (l.loss + nt * N_LOSS * sizeof(double) + 15) & ~(size_t)15;
    l.total = l.rec + (size_t)W * H * sizeof(float4);
    return l;
}

}  // namespace

size_t gsr_depth_loss_scratch_size(int W, int H) { return layout(W, H).total; }

void gsr_launch_depth_target(hipStream_t s, int W, int H, const float* prior, const float* anchor, float qstep, float* target_out,
                             float* half_band_out, uint8_t* flags_out) {
    const size_t n = (size_t)W * H;
    hipLaunchKernelGGL(depth_target_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, n, prior,
                       make_anchor(anchor), qstep, target_out, half_band_out, flags_out);
}

void gsr_launch_depth_loss_fwd(hipStream_t s, int W, int H, int C, const float* image, const float* prior, const float* anchor,
                               float qstep, float lambda_grad, float weight, float* loss_out, float* stats_out, float* target_out,
                               float* half_band_out, uint8_t* flags_out, void* scratch) {
    const dim3 g = tile_grid(W, H);
    const int nt = (int)(g.x * g.y);
    const Layout l = layout(W, H);
    char* base = (char*)scratch;
    float* head = (float*)base;
    double* p_stats = (double*)(base + l.stats);
    double* p_loss = (double*)(base + l.loss);
    float4* rec = (float4*)(base + l.rec);
    hipLaunchKernelGGL(depth_stats_kernel, g, dim3(THREADS), 0, s, W, H, C, image, prior, make_anchor(anchor), qstep, target_out,
                       half_band_out, flags_out, rec, p_stats);
    hipLaunchKernelGGL(depth_header_kernel, dim3(1), dim3(THREADS), 0, s, nt, p_stats, head);
    hipLaunchKernelGGL(depth_loss_kernel, g, dim3(THREADS), 0, s, W, H, rec, head, p_loss);
    hipLaunchKernelGGL(depth_final_kernel, dim3(1), dim3(THREADS), 0, s, nt, p_loss, head, lambda_grad, weight, loss_out,
                       stats_out);
}

void gsr_launch_depth_loss_bwd(hipStream_t s, int W, int H, int C, const float* image, float lambda_grad, float weight,
                               float* vpixels, const void* scratch) {
    const Layout l = layout(W, H);
    const char* base = (const char*)scratch;
    hipLaunchKernelGGL(depth_bwd_kernel, tile_grid(W, H), dim3(THREADS), 0, s, W, H, C, image, (const float4*)(base + l.rec),
                       (const float*)base, lambda_grad, weight, vpixels);
}
