// The MCMC densification strategy on the device ("3D Gaussian Splatting as Markov Chain Monte Carlo"): the dead mask and the
// sampling weights, the multinomial draw, the Eq. 9 split, the relocation of dead rows, the per-step position noise and the
// opacity / scale regulariser of the reference's MCMCStrategy.
// Reference behaviour: src/mcmc.jl:104-107 (regularization_loss), :132-178 (relocate_gaussians!), :184-217 (add_gaussians!),
// :220-225 (multinomial_sample), :232-260 (split_sampled!), :266-280 (relocation_params), :288-325 (inject_noise!).
// Two intended deviations (include/gsr.h): the random numbers come from the project's counter-based generator
// (rng.h), and the multinomial draw runs on integer weights with exact 64-bit prefix sums.
// Compiled with -ffp-contract=off, like densify.hip: the fp32 expression trees are the reference's, only the transcendental
// calls (exp / log / pow / cos / sin) differ from a host libm by ulps.
#include "gsr_kernels.h"
#include "block_reduce.h"
#include "quat.h"
#include "rng.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ float sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }  // NU.sigmoid

// ---- weights and dead mask (mcmc.jl:135-140, :189-190) ----
// q = floor(sigmoid(opacity) · 2^30) — the product is exact in fp32 —, 0 for a dead row; dead = (o <= min_opacity) |
// (max_j scales[j] > log_max_scale).  dead == nullptr: every row is weighted (add_gaussians!).
__global__ __launch_bounds__(256) void mcmc_weights_kernel(long long n, int sd, const float* __restrict__ opac,
                                                           const float* __restrict__ scales, float min_opacity,
                                                           float log_max_scale, uint32_t* __restrict__ q,
                                                           uint8_t* __restrict__ dead) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float o = sigmoid_(opac[i]);
    bool d = false;
    if (dead) {
        float smax = scales[i * sd];
        for (int j = 1; j < sd; j++) smax = fmaxf(smax, scales[i * sd + j]);
        d = (o <= min_opacity) | (smax > log_max_scale);
        dead[i] = d ? 1 : 0;
    }
    const float w = o * 1073741824.0f;  // in [0, 2^30]; a NaN opacity weighs nothing
    q[i] = (d || !(w >= 0.0f)) ? 0u : (uint32_t)floorf(w);
}

// ---- multinomial sampling (mcmc.jl:220-225, counts: :237-240) ----
// Exact inclusive prefix sums of q in uint64, in the three-pass form of findall (trainer.hip): sums of 1024-row blocks, a
// one-workgroup scan of the block sums, per-block prefixes.  A thread owns 4 consecutive rows.
constexpr int MS_BLOCK = 1024;

__device__ __forceinline__ u64 load_rows4(long long n, const uint32_t* __restrict__ q, long long first, uint32_t (&v)[4]) {
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = first + k < n ? q[first + k] : 0u;
        s += v[k];
    }
    return s;
}

__global__ __launch_bounds__(256) void mcmc_block_sum_kernel(long long n, const uint32_t* __restrict__ q,
                                                             u64* __restrict__ block_sum) {
    __shared__ u64 wsum[4];
    uint32_t v[4];
    const u64 s = load_rows4(n, q, (long long)blockIdx.x * MS_BLOCK + 4 * threadIdx.x, v);
    const int lane = threadIdx.x & 63;
    const u64 x = gsr::wave_inclusive_scan(s, lane);
    if (lane == 63) wsum[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) block_sum[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(1024) void mcmc_scan_blocks_kernel(int nb, u64* __restrict__ block_sum /* in: sums, out: exclusive offsets */,
                                                                u64* __restrict__ total) {
    gsr::block_scan_carry(nb, block_sum, total);
}

__global__ __launch_bounds__(256) void mcmc_prefix_kernel(long long n, const uint32_t* __restrict__ q,
                                                          const u64* __restrict__ block_off, u64* __restrict__ prefix) {
    __shared__ u64 wsum[4];
    uint32_t v[4];
    const long long first = (long long)blockIdx.x * MS_BLOCK + 4 * threadIdx.x;
    const u64 s = load_rows4(n, q, first, v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 x = gsr::wave_inclusive_scan(s, lane);
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    u64 run = block_off[blockIdx.x] + x - s;
    for (int w = 0; w < wave; w++) run += wsum[w];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        run += v[k];
        if (first + k < n) prefix[first + k] = run;
    }
}

// draw j: r = mulhi64(h, total) with h = 64 bits of (seed, j, draw 0 | draw 1), uniform on [0, total); selects the first row
// whose inclusive prefix is > r — never a zero-weight row.  total == 0: nothing is written.
__global__ __launch_bounds__(256) void mcmc_draw_kernel(long long n, long long m, uint32_t seed, const u64* __restrict__ prefix,
                                                        const u64* __restrict__ total, uint32_t* __restrict__ sampled,
                                                        int32_t* __restrict__ counts) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const u64 tot = *total;
    if (tot == 0) return;
    const u64 h = ((u64)gsr::rand_bits(seed, (uint32_t)j, 0) << 32) | (u64)gsr::rand_bits(seed, (uint32_t)j, 1);
    const u64 r = __umul64hi(h, tot);
    long long lo = 0, hi = n - 1;  // r < total = prefix[n-1]: the answer exists
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (prefix[mid] > r) hi = mid; else lo = mid + 1;
    }
    sampled[j] = (uint32_t)lo;
    atomicAdd(&counts[lo], 1);
}

// ---- Eq. 9 (relocation_params, mcmc.jl:266-280): the reference's fp32 expression, `i` outer, `k` inner ----
// binoms: (n_max, n_max) row-major, binoms[n][k] = C(n, k)·(-1)^k/√(k+1) (mcmc_binom_coefficients, :79-90).
__device__ __forceinline__ void relocation_params(float o, int ratio, float min_opacity, const float* __restrict__ binoms,
                                                  int n_max, float& new_o_out, float& coeff_out) {
    const float hi = 1.0f - 1e-6f;
    o = fminf(fmaxf(o, 1e-6f), hi);
    float new_o = 1.0f - powf(1.0f - o, 1.0f / (float)ratio);
    new_o = fminf(fmaxf(new_o, fmaxf(1e-6f, min_opacity)), hi);
    float denom = 0.0f;
    for (int i = 1; i <= ratio; i++)
        for (int k = 0; k < i; k++) denom += binoms[(i - 1) * n_max + k] * powf(new_o, (float)(k + 1));
    denom = copysignf(fmaxf(fabsf(denom), 1e-8f), denom);  // sign-preserving floor
    new_o_out = new_o;
    coeff_out = fminf(fmaxf(o / denom, -1e6f), 1e6f);
}

__global__ __launch_bounds__(256) void mcmc_relocation_params_kernel(long long m, const float* __restrict__ o,
                                                                     const int32_t* __restrict__ ratio,
                                                                     const float* __restrict__ binoms, int n_max,
                                                                     float min_opacity, float* __restrict__ new_o,
                                                                     float* __restrict__ coeff) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int r = min(max(ratio[i], 1), n_max);
    float a, c;
    relocation_params(o[i], r, min_opacity, binoms, n_max, a, c);
    new_o[i] = a;
    coeff[i] = c;
}

// split_sampled! (mcmc.jl:232-260) in place, one thread per ROW: a source drawn several times is rewritten once, from its own
// opacity before the rewrite.
__global__ __launch_bounds__(256) void mcmc_split_kernel(long long n, int sd, const int32_t* __restrict__ counts,
                                                         const float* __restrict__ binoms, int n_max, float min_opacity,
                                                         float* __restrict__ opac, float* __restrict__ scales) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = counts[i];
    if (c <= 0) return;
    const int ratio = min(max(c + 1, 1), n_max);
    float new_o, coeff;
    relocation_params(sigmoid_(opac[i]), ratio, min_opacity, binoms, n_max, new_o, coeff);
    opac[i] = logf(new_o / (1.0f - new_o));  // inverse_sigmoid
    for (int j = 0; j < sd; j++) scales[i * sd + j] = logf(fmaxf(fabsf(coeff * expf(scales[i * sd + j])), 1e-10f));
}

// ---- relocation of the dead rows (mcmc.jl:153-172), in place: x[dead[j]] = x[sampled[j]]; moments: both rows zeroed ----
struct RelocGroups {
    uint32_t* x[GSR_COMPOSE_MAX_GROUPS];
    int row_words[GSR_COMPOSE_MAX_GROUPS];
    int new_zero[GSR_COMPOSE_MAX_GROUPS];
    long long block_start[GSR_COMPOSE_MAX_GROUPS + 1];
    int n;
};
__global__ __launch_bounds__(256) void mcmc_relocate_kernel(RelocGroups G, long long n, const uint32_t* __restrict__ dead,
                                                            const uint32_t* __restrict__ sampled, long long m) {
    int g = 0;
    for (int k = 1; k < G.n; k++)
        if ((long long)blockIdx.x >= G.block_start[k]) g = k;
    const int rw = G.row_words[g];
    const long long e = ((long long)blockIdx.x - G.block_start[g]) * 256 + threadIdx.x;
    if (e >= m * rw) return;
    const long long j = e / rw;
    const int w = (int)(e - j * rw);
    const long long d = dead[j], s = sampled[j];
    if (d >= n || s >= n) return;  // never outside the arrays, whatever the index vectors hold
    uint32_t* __restrict__ x = G.x[g];
    if (G.new_zero[g]) {
        x[d * rw + w] = 0u;
        x[s * rw + w] = 0u;
    } else {
        x[d * rw + w] = x[s * rw + w];  // dead ∩ sampled = ∅: no row is both read and written
    }
}

// ---- _inject_noise! (mcmc.jl:306-325) ----
// One thread per Gaussian, one pass: 44 B read + 12 B written.  Rotations arrive as one float4 per lane; points and
// anisotropic scales are read — and the points written — as the FLAT float stream of the wave's 64 rows (three fully
// coalesced dwords per lane) and transposed between "element 64k + lane" and "component c of row lane" inside the wave: lane
// s holds component c in exactly one of its three registers, number (c - s) mod 3, so one lane permute per component does
// it.  No LDS allocation, no atomics.
__device__ __forceinline__ float sel3(const float (&v)[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

__device__ __forceinline__ void wave_flat_to_rows(const float (&flat)[3], int lane, float (&row)[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int k = (c + 66 - lane) % 3;  // the register of THIS lane that holds a component c
        row[c] = __shfl(sel3(flat, k), (3 * lane + c) & 63);
    }
}
__device__ __forceinline__ void wave_rows_to_flat(const float (&row)[3], int lane, float (&flat)[3]) {
    float t[3];
    int kc[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        kc[c] = (c + 66 - lane) % 3;  // register kc[c] of this lane is component c of row (64·kc[c] + lane) / 3
        t[c] = __shfl(row[c], (64 * kc[c] + lane) / 3);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) flat[k] = kc[0] == k ? t[0] : (kc[1] == k ? t[1] : t[2]);
}

__global__ __launch_bounds__(256) void mcmc_noise_kernel(long long n, int sd, float* __restrict__ points,
                                                         const float* __restrict__ opac, const float* __restrict__ scales,
                                                         const float4* __restrict__ rots, float lr, float max_kick,
                                                         uint32_t seed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // (rows >= n stay in: the wave permutes need every lane)
    const int lane = threadIdx.x & 63;
    const long long fbase = 3 * (i - lane);  // first flat element of the wave's 64 rows
    const long long nf = 3 * n;
    const bool live = i < n;
    float pf[3], sf[3], p[3], s[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const long long e = fbase + 64 * k + lane;
        pf[k] = e < nf ? points[e] : 0.0f;
        sf[k] = (sd == 3 && e < nf) ? scales[e] : 0.0f;
    }
    wave_flat_to_rows(pf, lane, p);
    if (sd == 3) wave_flat_to_rows(sf, lane, s);
    else s[0] = s[1] = s[2] = live ? scales[i] : 0.0f;
    const float4 q4 = live ? rots[i] : make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    const float op = sigmoid_(live ? opac[i] : 0.0f);

    float xi[3], R[3][3], t[3], d[3];
    gsr::randn3(seed, (uint32_t)i, xi);
    gsr::unnorm_quat2rot(q4, R);
    // Σ·ξ = R·S²·Rᵀ·ξ with the variance capped: `exp` overflow would give ±Inf and poison the position
#pragma unroll
    for (int c = 0; c < 3; c++)
        t[c] = fminf(expf(2.0f * s[c]), 1e8f) * ((R[0][c] * xi[0] + R[1][c] * xi[1]) + R[2][c] * xi[2]);
    // the gate: essentially off above o ≈ 0.05, fully on below o ≈ 0.005; the exponent is capped against overflow
    const float factor = lr / (1.0f + expf(fminf(100.0f * op - 0.5f, 80.0f)));
#pragma unroll
    for (int r = 0; r < 3; r++) d[r] = factor * ((R[r][0] * t[0] + R[r][1] * t[1]) + R[r][2] * t[2]);
    const float l = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (l > max_kick) {
        const float k = max_kick / l;
#pragma unroll
        for (int r = 0; r < 3; r++) d[r] = d[r] * k;
    }
#pragma unroll
    for (int r = 0; r < 3; r++) p[r] = p[r] + d[r];
    wave_rows_to_flat(p, lane, pf);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const long long e = fbase + 64 * k + lane;
        if (e < nf) points[e] = pf[k];
    }
}

// ---- regularization_loss (mcmc.jl:104-107) ----
// One pass over the flat index e in [0, 3n): e < n sums sigmoid(opacity[e]), e < n·sd sums exp(scale[e]); the constant gradients
// w.r.t. the ACTIVATED values are added onto vopacities (1,N) and vscales (3,N) (isotropic: row 0 only — the prologue
// pullback sums the three tiled rows).  partial[wg] = (Σ sigmoid, Σ exp) of the workgroup's chunk, summed in a fixed order.
constexpr int RG_PER = 8, RG_CHUNK = 256 * RG_PER;

__global__ __launch_bounds__(256) void mcmc_reg_kernel(long long n, int sd, const float* __restrict__ opac,
                                                       const float* __restrict__ scales, float grad_o, float grad_s,
                                                       float* __restrict__ vopac, float* __restrict__ vscales,
                                                       float* __restrict__ partial) {
    __shared__ float red[4];
    float so = 0.0f, ss = 0.0f;
    const long long ns = n * sd, n3 = 3 * n;
#pragma unroll
    for (int k = 0; k < RG_PER; k++) {
        const long long e = (long long)blockIdx.x * RG_CHUNK + k * 256 + threadIdx.x;
        if (e < n) {
            so += sigmoid_(opac[e]);
            if (vopac) vopac[e] = vopac[e] + grad_o;
        }
        if (e < ns) ss += expf(scales[e]);
        if (vscales && e < n3 && (sd == 3 || e % 3 == 0)) vscales[e] = vscales[e] + grad_s;
    }
    so = gsr::block_sum(so, red);
    ss = gsr::block_sum(ss, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = so;
        partial[2 * blockIdx.x + 1] = ss;
    }
}

__global__ __launch_bounds__(256) void mcmc_reg_final_kernel(int n_partial, const float* __restrict__ partial, long long n, int sd,
                                                             float opacity_reg, float scale_reg, float* loss_out) {
    __shared__ double red[2][256];
    double t[2];  // (Σ sigmoid, Σ exp)
    gsr::sum_partials<2>(n_partial, partial, red, t);
    if (threadIdx.x != 0) return;
    *loss_out = n > 0 ? opacity_reg * (float)(t[0] / (double)n) + scale_reg * (float)(t[1] / (double)(n * sd)) : 0.0f;
}

unsigned blocks_for(long long work, int per_block) { return (unsigned)((work + per_block - 1) / per_block); }

}  // namespace

void gsr_launch_mcmc_weights(hipStream_t s, long long n, int scale_dims, const float* opac, const float* scales, float min_opacity,
                             float log_max_scale, uint32_t* q, uint8_t* dead) {
    if (n <= 0) return;
    hipLaunchKernelGGL(mcmc_weights_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, n, scale_dims, opac, scales, min_opacity,
                       log_max_scale, q, dead);
}

// scratch: the block sums (one u64 per 1024 rows), then the n inclusive prefixes
static long long mcmc_sample_blocks(long long n) { return (n + MS_BLOCK - 1) / MS_BLOCK; }
size_t gsr_mcmc_sample_scratch_words(long long n) { return n <= 0 ? 0 : (size_t)(mcmc_sample_blocks(n) + n); }

void gsr_launch_mcmc_sample(hipStream_t s, long long n, const uint32_t* q, long long m, uint32_t seed, uint32_t* sampled,
                            int32_t* counts, unsigned long long* total, unsigned long long* scratch) {
    if (n <= 0) {
        (void)hipMemsetAsync(total, 0, sizeof(u64), s);
        return;
    }
    const long long nb = mcmc_sample_blocks(n);
    u64* block_sum = scratch;
    u64* prefix = scratch + nb;
    (void)hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n, s);
    hipLaunchKernelGGL(mcmc_block_sum_kernel, dim3((unsigned)nb), dim3(256), 0, s, n, q, block_sum);
    hipLaunchKernelGGL(mcmc_scan_blocks_kernel, dim3(1), dim3(1024), 0, s, (int)nb, block_sum, total);
    hipLaunchKernelGGL(mcmc_prefix_kernel, dim3((unsigned)nb), dim3(256), 0, s, n, q, block_sum, prefix);
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3(blocks_for(m, 256)), dim3(256), 0, s, n, m, seed, prefix, total, sampled, counts);
}

void gsr_launch_mcmc_split_sampled(hipStream_t s, long long n, int scale_dims, const int32_t* counts, const float* binoms, int n_max,
                                   float min_opacity, float* opac, float* scales) {
    if (n <= 0) return;
    hipLaunchKernelGGL(mcmc_split_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, n, scale_dims, counts, binoms, n_max,
                       min_opacity, opac, scales);
}

void gsr_launch_mcmc_relocation_params(hipStream_t s, long long m, const float* o, const int32_t* ratio, const float* binoms,
                                       int n_max, float min_opacity, float* new_o, float* coeff) {
    if (m <= 0) return;
    hipLaunchKernelGGL(mcmc_relocation_params_kernel, dim3(blocks_for(m, 256)), dim3(256), 0, s, m, o, ratio, binoms, n_max,
                       min_opacity, new_o, coeff);
}

void gsr_launch_mcmc_relocate_rows(hipStream_t s, int n_groups, void* const* x, const int* row_words, const int* new_zero,
                                   long long n, const uint32_t* dead, const uint32_t* sampled, long long m) {
    RelocGroups G;
    G.n = n_groups;
    long long blocks = 0;
    for (int g = 0; g < GSR_COMPOSE_MAX_GROUPS; g++) {
        const bool on = g < n_groups;
        G.x[g] = on ? (uint32_t*)x[g] : nullptr;
        G.row_words[g] = on ? row_words[g] : 1;
        G.new_zero[g] = on ? new_zero[g] : 0;
        G.block_start[g] = blocks;
        if (on) blocks += (m * row_words[g] + 255) / 256;
    }
    G.block_start[GSR_COMPOSE_MAX_GROUPS] = blocks;
    if (blocks == 0) return;
    hipLaunchKernelGGL(mcmc_relocate_kernel, dim3((unsigned)blocks), dim3(256), 0, s, G, n, dead, sampled, m);
}

void gsr_launch_mcmc_inject_noise(hipStream_t s, long long n, int scale_dims, float* points, const float* opac, const float* scales,
                                  const float* rots, float lr, float max_kick, uint32_t seed) {
    if (n <= 0) return;
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, n, scale_dims, points, opac, scales,
                       reinterpret_cast<const float4*>(rots), lr, max_kick, seed);
}

size_t gsr_mcmc_regularization_scratch_floats(long long n) { return n <= 0 ? 0 : 2 * (size_t)((3 * n + RG_CHUNK - 1) / RG_CHUNK); }

void gsr_launch_mcmc_regularization(hipStream_t s, long long n, int scale_dims, const float* opac, const float* scales,
                                    float opacity_reg, float scale_reg, float* loss_out, float* vopac, float* vscales,
                                    float* scratch) {
    const int wgs = (int)(gsr_mcmc_regularization_scratch_floats(n) / 2);
    if (wgs > 0)
        hipLaunchKernelGGL(mcmc_reg_kernel, dim3((unsigned)wgs), dim3(256), 0, s, n, scale_dims, opac, scales,
                           opacity_reg / (float)n, scale_reg / (float)(n * scale_dims), vopac, vscales, scratch);
    hipLaunchKernelGGL(mcmc_reg_final_kernel, dim3(1), dim3(256), 0, s, wgs, scratch, n, scale_dims, opacity_reg, scale_reg,
                       loss_out);
}
