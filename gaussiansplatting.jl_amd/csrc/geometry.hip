// Geometry regularisation of :rgbdn training (src/geometry_regularization.jl; `use_normal_loss`, training.jl:625-733):
// the depth-normal consistency loss over a rendered (8,W,H) frame, its pullback onto channels 3..7 of the frame's
// cotangent, and the flatten loss over the raw scales with its gradient.  Compiled with -ffp-contract=off: which centres
// are valid is decided by the reference's own fp32 expressions (IEEE division for e = D/α, jump = 0.05f·e_c, ...), so the
// mask is a function of the inputs and not of the arithmetic mode.
//
// Layout: image / vpixels (8,W,H) = the rasterizer's :rgbdn frame, one 32-byte record per pixel: rgb | D | α | normal.
// A 128-byte line holds four whole records, so every kernel here moves whole lines: 32 B per pixel per pass.
//
// No float atomics anywhere.  The forward's scalars are per-workgroup partials summed in index order by
// a one-workgroup pass, which also applies the "too little evidence" gate on the device and leaves the normaliser for
// the backward.  In the backward, cosθ of a centre does not depend on its own e, so a pixel's ∂/∂e is what its up to four
// neighbouring centres send it: a workgroup stages (e, α) of its 64x16 tile with a 2-pixel halo in LDS, evaluates every
// centre of the tile and of the 1-pixel ring around it ONCE into LDS (the four ∂/∂e of its stencil arms), and every pixel
// then gathers its four terms in a fixed order.  A centre on a tile's ring is evaluated by two or more workgroups, by the
// same instruction sequence on the same inputs: the same bits, so the result does not depend on the tiling.
//
// The fused gsr_backward_trainer_tail never materialises ∇scales, so it cannot take the flatten gradient: steps with the
// regulariser on run gsr_backward + gsr_flatten_loss (adds onto vscales) + gsr_trainer_tail_step.
#include "gsr_kernels.h"
#include "block_reduce.h"

namespace {

// thresholds of geometry_regularization.jl:37-43
constexpr float MIN_ALPHA = 0.5f, MAX_REL_JUMP = 0.05f, MIN_DEPTH = 1e-6f, MIN_RENDER_NORM = 0.1f;
constexpr float MIN_COUNT = 64.0f, MIN_WEIGHT = 16.0f, MIN_CROSS_SQ = 1e-24f;

constexpr int TX = 64, TY = 16, THREADS = 256;  // pixels of a tile; four rows per thread

struct Rays { float cx, cy, fx, fy; };  // pixel_rays (geometry_regularization.jl:53-62), 0-based pixel index
__device__ __forceinline__ float ray_x(const Rays& r, int x) { return ((float)x + 0.5f - r.cx) / r.fx; }
__device__ __forceinline__ float ray_y(const Rays& r, int y) { return ((float)y + 0.5f - r.cy) / r.fy; }

// `max.(depth, 0f0) ./ max.(alpha, 1f-6)` (:115): Julia's max keeps a NaN, fmaxf would drop it
__device__ __forceinline__ float alpha_floor(float a) { return a < MIN_DEPTH ? MIN_DEPTH : a; }
__device__ __forceinline__ float expected_depth(float d, float a) { return (d < 0.0f ? 0.0f : d) / alpha_floor(a); }

// (e, α) of the tile at (x0, y0) with a HALO-pixel border -> LDS; pixels outside the image get α = 0 (never opaque)
template <int HALO>
__device__ __forceinline__ void stage_tile(const float* __restrict__ image, int W, int H, int x0, int y0, float* se,
                                           float* sa) {
    constexpr int SW = TX + 2 * HALO, SH = TY + 2 * HALO;
    for (int i = threadIdx.x; i < SW * SH; i += THREADS) {
        const int ly = i / SW, lx = i - ly * SW;
        const int x = x0 - HALO + lx, y = y0 - HALO + ly;
        float e = 0.0f, a = 0.0f;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const float* px = image + ((size_t)y * W + x) * 8;
            a = px[4];
            e = expected_depth(px[3], a);
        }
        se[i] = e;
        sa[i] = a;
    }
}

// One centre (geometry_regularization.jl:117-175).  The stencil's (e, α) come from the staged tile (row stride `sw`,
// `i` = the centre's index in it), nr from the frame.  Returns the detached weight w (0 = the centre takes no part) and
// 1 - cosθ; with GRAD also ∂(1 - cosθ)/∂(e_xp, e_xm, e_yp, e_ym) and ∂(1 - cosθ)/∂nr.  An invalid centre returns zeros
// whatever its stencil holds: the one intended deviation from the reference's `sum(w .* (1 .- cosθ))`, where 0 · NaN of
// a non-finite depth in an invalid region would cost the whole step.
template <bool GRAD>
__device__ __forceinline__ float centre_eval(const float* se, const float* sa, int i, int sw, const Rays& r, int x, int y,
                                             float nr1, float nr2, float nr3, float& one_minus_cos, float* ge, float* gn) {
    const float e_c = se[i], e_xp = se[i + 1], e_xm = se[i - 1], e_yp = se[i + sw], e_ym = se[i - sw];
    const float a_c = sa[i];
    const float rx_c = ray_x(r, x), rx_p = ray_x(r, x + 1), rx_m = ray_x(r, x - 1);
    const float ry_c = ray_y(r, y), ry_p = ray_y(r, y + 1), ry_m = ray_y(r, y - 1);
    const float dx = e_xp - e_xm, dy = e_yp - e_ym;
    const float tx1 = e_xp * rx_p - e_xm * rx_m, tx2 = dx * ry_c, tx3 = dx;
    const float ty1 = dy * rx_c, ty2 = e_yp * ry_p - e_ym * ry_m, ty3 = dy;
    const float n1 = tx2 * ty3 - tx3 * ty2, n2 = tx3 * ty1 - tx1 * ty3, n3 = tx1 * ty2 - tx2 * ty1;
    const float n_sq = n1 * n1 + n2 * n2 + n3 * n3;
    const float nr_sq = nr1 * nr1 + nr2 * nr2 + nr3 * nr3;
    const float jump = MAX_REL_JUMP * e_c;
    const bool opaque = a_c >= MIN_ALPHA && sa[i + 1] >= MIN_ALPHA && sa[i - 1] >= MIN_ALPHA && sa[i + sw] >= MIN_ALPHA &&
                        sa[i - sw] >= MIN_ALPHA;
    const bool continuous = e_c >= MIN_DEPTH && fabsf(e_xp - e_c) <= jump && fabsf(e_xm - e_c) <= jump &&
                            fabsf(e_yp - e_c) <= jump && fabsf(e_ym - e_c) <= jump;
    const bool ok = opaque && continuous && isfinite(e_c) && n_sq >= MIN_CROSS_SQ && nr_sq >= MIN_RENDER_NORM * MIN_RENDER_NORM;
    one_minus_cos = 0.0f;
    if (GRAD) {
        ge[0] = ge[1] = ge[2] = ge[3] = 0.0f;
        gn[0] = gn[1] = gn[2] = 0.0f;
    }
    if (!ok) return 0.0f;
    // valid: n_sq and nr_sq are above their floors, so neither clamp of the reference is active
    const float n_norm = sqrtf(n_sq), nr_norm = sqrtf(nr_sq);
    const float facing = n1 * rx_c + n2 * ry_c + n3;
    const float flip = (facing > 0.0f ? -1.0f : 1.0f) / n_norm;  // the sign is detached (:138-142)
    const float nd1 = n1 * flip, nd2 = n2 * flip, nd3 = n3 * flip;
    const float dot = nd1 * nr1 + nd2 * nr2 + nd3 * nr3;
    const float cosv = dot / nr_norm;
    one_minus_cos = 1.0f - cosv;
    if (GRAD) {
        // ∂(1-cos)/∂nr = -(nd/|nr| - cos·nr/|nr|²)
        const float q = cosv / nr_sq;
        gn[0] = q * nr1 - nd1 / nr_norm;
        gn[1] = q * nr2 - nd2 / nr_norm;
        gn[2] = q * nr3 - nd3 / nr_norm;
        // ∂(1-cos)/∂n = -flip/|nr| · (nr - (n·nr)/|n|² · n)
        const float s = flip / nr_norm, p = (n1 * nr1 + n2 * nr2 + n3 * nr3) / n_sq;
        const float g1 = -s * (nr1 - p * n1), g2 = -s * (nr2 - p * n2), g3 = -s * (nr3 - p * n3);
        // n = tx × ty:  ∂/∂tx = ty × g,  ∂/∂ty = g × tx
        const float gtx1 = ty2 * g3 - ty3 * g2, gtx2 = ty3 * g1 - ty1 * g3, gtx3 = ty1 * g2 - ty2 * g1;
        const float gty1 = g2 * tx3 - g3 * tx2, gty2 = g3 * tx1 - g1 * tx3, gty3 = g1 * tx2 - g2 * tx1;
        const float gx = gtx2 * ry_c + gtx3, gy = gty1 * rx_c + gty3;
        ge[0] = gtx1 * rx_p + gx;
        ge[1] = -(gtx1 * rx_m + gx);
        ge[2] = gty2 * ry_p + gy;
        ge[3] = -(gty2 * ry_m + gy);
    }
    return fminf(fmaxf(a_c, 0.0f), 1.0f);
}

// ---- forward: one workgroup per tile -> partial[wg] = (Σ w(1-cos), Σ w, count) ----
__global__ __launch_bounds__(THREADS) void normal_fwd_kernel(int W, int H, const float* __restrict__ image, Rays rays,
                                                             float* __restrict__ weights_out, float* __restrict__ partial) {
    constexpr int SW = TX + 2, SH = TY + 2;
    __shared__ float se[SW * SH], sa[SW * SH], red[4];
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    stage_tile<1>(image, W, H, x0, y0, se, sa);
    __syncthreads();
    const int lx = threadIdx.x & 63, x = x0 + lx;
    float s_loss = 0.0f, s_w = 0.0f, s_n = 0.0f;
#pragma unroll
    for (int k = 0; k < TY / 4; k++) {
        const int ly = (threadIdx.x >> 6) + 4 * k, y = y0 + ly;
        if (x >= W || y >= H) continue;
        float w = 0.0f, omc = 0.0f;
        if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2) {
            const float4 hi = *reinterpret_cast<const float4*>(image + ((size_t)y * W + x) * 8 + 4);
            w = centre_eval<false>(se, sa, (ly + 1) * SW + lx + 1, SW, rays, x, y, hi.y, hi.z, hi.w, omc, nullptr, nullptr);
        }
        if (w > 0.0f) {  // (w = α_c >= 0.5 on a valid centre)
            s_loss += w * omc;
            s_w += w;
            s_n += 1.0f;
        }
        if (weights_out) weights_out[(size_t)y * W + x] = w;
    }
    s_loss = gsr::block_sum(s_loss, red);
    s_w = gsr::block_sum(s_w, red);
    s_n = gsr::block_sum(s_n, red);
    if (threadIdx.x == 0) {
        float* p = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        p[0] = s_loss; p[1] = s_w; p[2] = s_n;
    }
}

// the partials in index order (in double: a few thousand terms) -> loss, stats = (Σw, count) and the backward's header
// head = (Σ w(1-cos), Σw, count, scale), scale = 1 / max(Σw, 1), or 0 for a gated view (geometry_regularization.jl:177-182)
__global__ __launch_bounds__(THREADS) void normal_final_kernel(int n_partial, const float* __restrict__ partial, float weight,
                                                               float* loss_out, float* stats_out, float* head) {
    __shared__ double red[3][THREADS];
    double s[3];
    gsr::sum_partials<3>(n_partial, partial, red, s);
    if (threadIdx.x != 0) return;
    const float sum_w = (float)s[1], count = (float)s[2];
    const bool enough = count >= MIN_COUNT && sum_w >= MIN_WEIGHT;
    const double norm = s[1] > 1.0 ? s[1] : 1.0;
    const float scale = enough ? (float)(1.0 / norm) : 0.0f;
    *loss_out = enough ? weight * (float)(s[0] / norm) : 0.0f;
    stats_out[0] = sum_w;
    stats_out[1] = count;
    head[0] = (float)s[0]; head[1] = sum_w; head[2] = count; head[3] = scale;
}

// ---- backward: adds weight · ∂loss/∂(D, α, normal) onto channels 3..7 of vpixels ----
__global__ __launch_bounds__(THREADS) void normal_bwd_kernel(int W, int H, const float* __restrict__ image, Rays rays,
                                                             float weight, const float* __restrict__ head,
                                                             float* __restrict__ vpixels) {
    constexpr int SW = TX + 4, SH = TY + 4;   // staged (e, α): 2-pixel halo
    constexpr int CW = TX + 2, CH = TY + 2;   // evaluated centres: 1-pixel ring
    __shared__ float se[SW * SH], sa[SW * SH];
    __shared__ float g_xp[CW * CH], g_xm[CW * CH], g_yp[CW * CH], g_ym[CW * CH];
    const float k = weight * head[3];
    if (k == 0.0f) return;  // a gated view (or a zero weight) adds nothing: vpixels is not touched
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    stage_tile<2>(image, W, H, x0, y0, se, sa);
    __syncthreads();
    for (int i = threadIdx.x; i < CW * CH; i += THREADS) {
        const int cy = i / CW, cx = i - cy * CW;
        const int x = x0 - 1 + cx, y = y0 - 1 + cy;
        float ge[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gn[3] = {0.0f, 0.0f, 0.0f};
        float w = 0.0f, omc;
        if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2) {
            const float4 hi = *reinterpret_cast<const float4*>(image + ((size_t)y * W + x) * 8 + 4);
            w = centre_eval<true>(se, sa, (cy + 1) * SW + cx + 1, SW, rays, x, y, hi.y, hi.z, hi.w, omc, ge, gn);
        }
        const float kw = k * w;
        g_xp[i] = kw * ge[0]; g_xm[i] = kw * ge[1]; g_yp[i] = kw * ge[2]; g_ym[i] = kw * ge[3];
        // the normal's cotangent has one source, the pixel's own centre: written by the tile that owns the pixel
        if (w > 0.0f && cx >= 1 && cx <= TX && cy >= 1 && cy <= TY) {
            float* v = vpixels + ((size_t)y * W + x) * 8;
            v[5] += kw * gn[0]; v[6] += kw * gn[1]; v[7] += kw * gn[2];
        }
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, x = x0 + lx;
#pragma unroll
    for (int j = 0; j < TY / 4; j++) {
        const int ly = (threadIdx.x >> 6) + 4 * j, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int c = (ly + 1) * CW + lx + 1;
        // what the centres left, right, above and below send this pixel, in this order
        const float t0 = g_xp[c - 1], t1 = g_xm[c + 1], t2 = g_yp[c - CW], t3 = g_ym[c + CW];
        if (t0 == 0.0f && t1 == 0.0f && t2 == 0.0f && t3 == 0.0f) continue;  // no valid neighbour: nothing is added
        const float g = ((t0 + t1) + t2) + t3;
        // a pixel in the stencil of a valid centre has finite e > 0 and α >= 0.5; the general form is kept all the same
        const int s = (ly + 2) * SW + lx + 2;
        float* v = vpixels + ((size_t)y * W + x) * 8;
        const float d = image[((size_t)y * W + x) * 8 + 3], a = sa[s], af = alpha_floor(a);
        if (d > 0.0f) v[3] += g / af;                      // ∂e/∂D = [D > 0] / max(α, 1e-6)
        if (a > MIN_DEPTH) v[4] += -(se[s] / af) * g;      // ∂e/∂α = -e / max(α, 1e-6) · [α > 1e-6]
    }
}

// ---- flatten loss (geometry_regularization.jl:197-211) ----
constexpr int FL_PER = 8, FL_CHUNK = THREADS * FL_PER;

// scales (scale_dims, N) raw.  partial[wg] = Σ exp(min_j s[j, i]) over the workgroup's chunk; vscales (3, N), unless NULL,
// gets `grad` added on the first axis that holds the minimum (the reference's cumsum tie-break)
__global__ __launch_bounds__(THREADS) void flatten_kernel(int n, int sd, const float* __restrict__ scales, float grad,
                                                          float* __restrict__ vscales, float* __restrict__ partial) {
    __shared__ float red[4];
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < FL_PER; k++) {
        const int i = blockIdx.x * FL_CHUNK + k * THREADS + threadIdx.x;
        if (i >= n) continue;
        const float* s = scales + (size_t)i * sd;
        float m = s[0];
        int arg = 0;
        for (int j = 1; j < sd; j++)
            if (s[j] < m) { m = s[j]; arg = j; }
        sum += expf(m);
        if (vscales) vscales[(size_t)i * 3 + arg] += grad;
    }
    sum = gsr::block_sum(sum, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(THREADS) void flatten_final_kernel(int n_partial, const float* __restrict__ partial, float weight,
                                                                int n, float* loss_out) {
    __shared__ double red[1][THREADS];
    double t;
    gsr::sum_partials<1>(n_partial, partial, red, &t);
    if (threadIdx.x != 0) return;
    *loss_out = n > 0 ? weight * (float)(t / (double)n) : 0.0f;
}

Rays make_rays(int W, int H, const float* focal, const float* principal) {
    return Rays{principal[0] * (float)W, principal[1] * (float)H, focal[0], focal[1]};
}
dim3 tile_grid(int W, int H) { return dim3((unsigned)((W + TX - 1) / TX), (unsigned)((H + TY - 1) / TY)); }

}  // namespace

// floats: the 4-float header + 3 per tile
size_t gsr_normal_loss_scratch_floats(int W, int H) {
    const dim3 g = tile_grid(W, H);
    return 4 + (size_t)g.x * g.y * 3;
}

void gsr_launch_normal_loss_fwd(hipStream_t s, int W, int H, const float* image, const float* focal, const float* principal,
                                float weight, float* loss_out, float* stats_out, float* weights_out, float* scratch) {
    const dim3 g = tile_grid(W, H);
    // W <= 2 or H <= 2 has no interior pixel (geometry_regularization.jl:93): every partial is zero and the gate closes
    hipLaunchKernelGGL(normal_fwd_kernel, g, dim3(THREADS), 0, s, W, H, image, make_rays(W, H, focal, principal), weights_out,
                       scratch + 4);
    hipLaunchKernelGGL(normal_final_kernel, dim3(1), dim3(THREADS), 0, s, (int)(g.x * g.y), scratch + 4, weight, loss_out,
                       stats_out, scratch);
}

void gsr_launch_normal_loss_bwd(hipStream_t s, int W, int H, const float* image, const float* focal, const float* principal,
                                float weight, float* vpixels, const float* scratch) {
    hipLaunchKernelGGL(normal_bwd_kernel, tile_grid(W, H), dim3(THREADS), 0, s, W, H, image, make_rays(W, H, focal, principal),
                       weight, scratch, vpixels);
}

size_t gsr_flatten_loss_scratch_floats(int64_t n) { return n <= 0 ? 0 : (size_t)((n + FL_CHUNK - 1) / FL_CHUNK); }

void gsr_launch_flatten_loss(hipStream_t s, int n, int scale_dims, const float* scales, float weight, float* loss_out,
                             float* vscales, float* scratch) {
    const int wgs = (int)gsr_flatten_loss_scratch_floats(n);
    if (wgs > 0)
        hipLaunchKernelGGL(flatten_kernel, dim3((unsigned)wgs), dim3(THREADS), 0, s, n, scale_dims, scales, weight / (float)n,
                           vscales, scratch);
    hipLaunchKernelGGL(flatten_final_kernel, dim3(1), dim3(THREADS), 0, s, wgs, scratch, weight, n, loss_out);
}
