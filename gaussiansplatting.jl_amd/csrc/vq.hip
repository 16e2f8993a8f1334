// SH codebook compression: exact k-means (Lloyd) on (n, dim) float32 rows, the nearest-code search on the f32 matrix cores.
// DESIGN.md §23; the definition is the header's (include/gsr.h, gsr_vq_*).  Every operation is one rounded fp32 operation,
// the fused ones written out (the MFMA builtin, __builtin_fmaf), so the result is the restatement's bits (tests/vq_ref.py).
//
//   prep   : one lane per code.  nh_j = -(0.5f * n2_j), n2_j the fmaf chain of the code's squares; the codebook is laid out
//            for the assign kernel in chunks of VQ_CH codes, transposed ([d][code], rows of VQ_ROW floats) and padded: columns
//            dim .. DP-1 are 0, codes past n_codes are 0 with nh = NaN, which no comparison ever selects.
//   assign : v_mfma_f32_32x32x2_f32, D = A·B + C with A = 32 codes x 2 columns, B = 2 columns x 32 points, C = nh_j in every
//            column.  One instruction is the two chain steps d = 2s, 2s+1 of 32 x 32 (code, point) pairs, bit for bit
//            fmaf(x_d1, c_d1, fmaf(x_d0, c_d0, acc)).  Tile shape: the instruction's dependent latency equals its issue
//            interval (64 cycles), and four independent accumulators per wave reach the issue rate from one wave per SIMD,
//            so a wave keeps FOUR point tiles (128 points, 4 x 16 accumulator registers) against ONE code tile: a code
//            operand is read from LDS once per four instructions, the points never leave their registers (4 x STEPS VGPRs).
//            A workgroup is four waves, 512 points; the codebook streams through LDS a chunk of 256 codes (<= 55 KiB) at a
//            time.  A lane's 16 accumulators of a tile are 16 codes of ONE point (lane & 31), the other 16 are in lane ^ 32:
//            the arg-max is a per-lane pass in ascending code order plus one exchange.  STEPS is a template argument (the
//            point registers must be indexed by constants), rounded up to a multiple of four: a padded column contributes
//            fmaf(0, 0, acc), which changes at most the sign of a zero and no comparison.
//   err    : one lane per row, the fmaf chain of the squared residual against the chosen code.
//   accumulate : a wave walks 64 consecutive rows, lane d owns column d (lane dim: the weight).  Sums of runs of equal
//            codes stay in registers; a run ends in ONE 64-bit integer atomic per column.  Integer sums: any order, same bits.
//   update / empty / decode : one lane per (code, column) / one workgroup / one lane per (row, column).
#include "gsr_kernels.h"
#include "block_reduce.h"

namespace {

constexpr int VQ_THREADS = 256;
constexpr int VQ_CH = 256;              // codes per LDS chunk
constexpr int VQ_ROW = VQ_CH + 32;      // floats from one column's codes to the next: the two half-waves read other banks
constexpr int VQ_WAVE_POINTS = 128;     // 4 tiles of 32 points per wave
constexpr int VQ_WG_POINTS = 512;       // 4 waves
constexpr uint32_t VQ_NONE = 0xFFFFFFFFu;
constexpr int VQ_ACC_ROWS = 64;         // rows one wave of the accumulate kernel walks

typedef float f32x16 __attribute__((ext_vector_type(16)));

inline int vq_steps(int dim) { return ((dim + 1) / 2 + 3) & ~3; }                 // 4, 8, ... 24
inline int vq_chunks(int n_codes) { return (n_codes + VQ_CH - 1) / VQ_CH; }
__host__ __device__ inline size_t vq_chunk_floats(int steps) { return (size_t)2 * steps * VQ_ROW + VQ_CH; }

__global__ __launch_bounds__(VQ_THREADS) void vq_prep_kernel(int n_codes, int dim, int steps, const float* __restrict__ codebook,
                                                             float* __restrict__ chunks, uint32_t* __restrict__ changed) {
    const int slot = blockIdx.x * VQ_THREADS + threadIdx.x;   // blockIdx.x is the chunk: VQ_CH == VQ_THREADS
    if (slot == 0 && changed) *changed = 0;
    float* __restrict__ out = chunks + (size_t)blockIdx.x * vq_chunk_floats(steps);
    const int jj = threadIdx.x;
    const bool valid = slot < n_codes;
    float n2 = 0.0f;
    const int dp = 2 * steps;
    for (int d = 0; d < dp; d++) {
        const float v = (valid && d < dim) ? codebook[(size_t)slot * dim + d] : 0.0f;
        n2 = __builtin_fmaf(v, v, n2);
        out[(size_t)d * VQ_ROW + jj] = v;
    }
    out[(size_t)dp * VQ_ROW + jj] = valid ? -(0.5f * n2) : __builtin_nanf("");
}

// Is the candidate (ov, oi) in front of (bv, bi)?  Any order of candidates gives the lowest index of the largest non-NaN value.
__device__ __forceinline__ bool vq_better(float ov, uint32_t oi, float bv, uint32_t bi) {
    return oi != VQ_NONE && (bi == VQ_NONE || ov > bv || (ov == bv && oi < bi));
}

template <int STEPS>
__global__ __launch_bounds__(VQ_THREADS) void vq_assign_kernel(int n, int n_codes, int dim, const float* __restrict__ rows,
                                                               const float* __restrict__ chunks, const uint16_t* prev,
                                                               uint16_t* indices, uint32_t* __restrict__ changed) {
    constexpr int DP = 2 * STEPS;
    constexpr int CHUNK_FLOATS = DP * VQ_ROW + VQ_CH;
    __shared__ __attribute__((aligned(16))) float lds[CHUNK_FLOATS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const int pbase = blockIdx.x * VQ_WG_POINTS + wave * VQ_WAVE_POINTS + col;

    float xb[4][STEPS];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int p = pbase + t * 32;
#pragma unroll
        for (int s = 0; s < STEPS; s++) {
            const int d = 2 * s + h;
            xb[t][s] = (p < n && d < dim) ? rows[(size_t)p * dim + d] : 0.0f;
        }
    }
    float bv[4];
    uint32_t bi[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        bv[t] = __builtin_nanf("");
        bi[t] = VQ_NONE;
    }

    const int n_chunks = (n_codes + VQ_CH - 1) / VQ_CH;
    for (int c = 0; c < n_chunks; c++) {
        __syncthreads();   // the previous chunk has been consumed
        const float4* __restrict__ src = reinterpret_cast<const float4*>(chunks + (size_t)c * CHUNK_FLOATS);
        float4* dst = reinterpret_cast<float4*>(lds);
        for (int i = threadIdx.x; i < CHUNK_FLOATS / 4; i += VQ_THREADS) dst[i] = src[i];
        __syncthreads();
        const int left = n_codes - c * VQ_CH;
        const int n_tiles = ((left < VQ_CH ? left : VQ_CH) + 31) >> 5;
        for (int ct = 0; ct < n_tiles; ct++) {
            // C: row (code) = (reg & 3) + 8*(reg >> 2) + 4*h of the tile, the same value in every column
            const float* nh = lds + DP * VQ_ROW + ct * 32 + 4 * h;
            f32x16 acc0, acc1, acc2, acc3;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 v = *reinterpret_cast<const float4*>(nh + 8 * q);
                acc0[4 * q] = v.x; acc0[4 * q + 1] = v.y; acc0[4 * q + 2] = v.z; acc0[4 * q + 3] = v.w;
            }
            acc1 = acc0; acc2 = acc0; acc3 = acc0;
            const float* a_col = lds + h * VQ_ROW + ct * 32 + col;
#pragma unroll
            for (int s = 0; s < STEPS; s++) {
                const float a = a_col[2 * s * VQ_ROW];   // A[code = lane & 31][k = lane >> 5]
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xb[0][s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xb[1][s], acc1, 0, 0, 0);
                acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xb[2][s], acc2, 0, 0, 0);
                acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xb[3][s], acc3, 0, 0, 0);
            }
            const uint32_t jb = (uint32_t)(c * VQ_CH + ct * 32);
            // ascending code order within the lane: a candidate wins only when it is LARGER (or the first that is not NaN)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const uint32_t jr = jb + 8 * (r >> 2) + (r & 3);   // + 4*h: added once, after the walk
                const float v0 = acc0[r], v1 = acc1[r], v2 = acc2[r], v3 = acc3[r];
                const bool k0 = !(v0 <= bv[0]) && (v0 == v0);
                const bool k1 = !(v1 <= bv[1]) && (v1 == v1);
                const bool k2 = !(v2 <= bv[2]) && (v2 == v2);
                const bool k3 = !(v3 <= bv[3]) && (v3 == v3);
                bv[0] = k0 ? v0 : bv[0]; bi[0] = k0 ? jr : bi[0];
                bv[1] = k1 ? v1 : bv[1]; bi[1] = k1 ? jr : bi[1];
                bv[2] = k2 ? v2 : bv[2]; bi[2] = k2 ? jr : bi[2];
                bv[3] = k3 ? v3 : bv[3]; bi[3] = k3 ? jr : bi[3];
            }
        }
    }

    uint32_t n_changed = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint32_t mine = bi[t] == VQ_NONE ? VQ_NONE : bi[t] + 4u * (uint32_t)h;
        const float ov = __shfl_xor(bv[t], 32, 64);
        const uint32_t oi = (uint32_t)__shfl_xor((int)mine, 32, 64);
        uint32_t best = vq_better(ov, oi, bv[t], mine) ? oi : mine;
        if (best == VQ_NONE) best = 0;   // every t_ij is NaN
        const int p = pbase + t * 32;
        if (h == 0 && p < n) {
            const bool diff = prev ? prev[p] != (uint16_t)best : true;   // read before the write: prev may be indices
            indices[p] = (uint16_t)best;
            n_changed += diff ? 1u : 0u;
        }
    }
    if (changed) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n_changed += (uint32_t)__shfl_xor((int)n_changed, off, 64);
        if (lane == 0 && n_changed) atomicAdd(changed, n_changed);   // integer: any order, the same count
    }
}

__global__ __launch_bounds__(VQ_THREADS) void vq_err_kernel(int n, int n_codes, int dim, const float* __restrict__ rows,
                                                            const float* __restrict__ codebook,
                                                            const uint16_t* __restrict__ indices, float* __restrict__ err) {
    const int p = blockIdx.x * VQ_THREADS + threadIdx.x;
    if (p >= n) return;
    int j = indices[p];
    j = j < n_codes ? j : n_codes - 1;
    const float* __restrict__ x = rows + (size_t)p * dim;
    const float* __restrict__ c = codebook + (size_t)j * dim;
    float e = 0.0f;
    for (int d = 0; d < dim; d++) {
        const float r = x[d] - c[d];
        e = __builtin_fmaf(r, r, e);
    }
    err[p] = e;
}

// rne(clamp(x, -128, 128) * 2^24): the product is exact (a power of two, no overflow, |q| <= 2^31); NaN counts as 0.
__device__ __forceinline__ long long vq_quant(float x) {
    if (!(x == x)) return 0;
    const float c = x < -128.0f ? -128.0f : (x > 128.0f ? 128.0f : x);
    return (long long)__builtin_rintf(c * 16777216.0f);
}

__device__ __forceinline__ void vq_flush(int cur, int lane, int dim, long long acc, long long* __restrict__ sums,
                                         unsigned long long* __restrict__ wsum) {
    if (cur < 0 || acc == 0) return;
    if (lane < dim)
        atomicAdd(reinterpret_cast<unsigned long long*>(sums) + (size_t)cur * dim + lane, (unsigned long long)acc);
    else if (lane == dim)
        atomicAdd(wsum + cur, (unsigned long long)acc);
}

__global__ __launch_bounds__(VQ_THREADS) void vq_accumulate_kernel(int n, int n_codes, int dim, const float* __restrict__ rows,
                                                                   const uint16_t* __restrict__ indices,
                                                                   const uint8_t* __restrict__ wq, long long* __restrict__ sums,
                                                                   unsigned long long* __restrict__ wsum) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (VQ_THREADS / 64) + (threadIdx.x >> 6);
    const long long r0l = wave * VQ_ACC_ROWS;
    if (r0l >= n) return;
    const int r0 = (int)r0l;
    const int r1 = n - r0 < VQ_ACC_ROWS ? n : r0 + VQ_ACC_ROWS;
    int cur = -1;
    long long acc = 0;
    for (int r = r0; r < r1; r += 4) {
        int j[4];
        long long w[4];
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int q = r + u < r1 ? r + u : r1 - 1;   // (a slot past the end repeats the last row with weight 0)
            const int jq = __builtin_amdgcn_readfirstlane((int)indices[q]);   // q is wave-uniform
            j[u] = jq < n_codes ? jq : n_codes - 1;
            w[u] = r + u < r1 ? (wq ? (long long)wq[q] : 1ll) : 0ll;
            v[u] = lane < dim ? rows[(size_t)q * dim + lane] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (j[u] != cur) {   // wave-uniform
                vq_flush(cur, lane, dim, acc, sums, wsum);
                cur = j[u];
                acc = 0;
            }
            acc += lane < dim ? w[u] * vq_quant(v[u]) : w[u];
        }
    }
    vq_flush(cur, lane, dim, acc, sums, wsum);
}

__global__ __launch_bounds__(VQ_THREADS) void vq_update_kernel(int n_codes, int dim, const long long* __restrict__ sums,
                                                               const unsigned long long* __restrict__ wsum,
                                                               float* __restrict__ codebook) {
    const int e = blockIdx.x * VQ_THREADS + threadIdx.x;
    if (e >= n_codes * dim) return;
    const unsigned long long w = wsum[e / dim];
    if (w > 0) codebook[e] = (float)((double)sums[e] / ((double)w * 16777216.0));
}

// ONE workgroup: *empty <- the number of codes with wsum == 0.
__global__ __launch_bounds__(VQ_THREADS) void vq_empty_kernel(int n_codes, const unsigned long long* __restrict__ wsum,
                                                              uint32_t* __restrict__ empty) {
    __shared__ uint32_t red[4];
    uint32_t cnt = 0;
    for (int j = threadIdx.x; j < n_codes; j += VQ_THREADS) cnt += wsum[j] == 0 ? 1u : 0u;
    cnt = gsr::block_sum<uint32_t, 4>(cnt, red);
    if (threadIdx.x == 0) *empty = cnt;
}

__global__ __launch_bounds__(VQ_THREADS) void vq_decode_kernel(long long total, int n_codes, int dim,
                                                               const float* __restrict__ codebook,
                                                               const uint16_t* __restrict__ indices, float* __restrict__ rows_out) {
    const long long e = (long long)blockIdx.x * VQ_THREADS + threadIdx.x;
    if (e >= total) return;
    const long long p = e / dim;
    const int d = (int)(e - p * dim);
    int j = indices[p];
    j = j < n_codes ? j : n_codes - 1;
    rows_out[e] = codebook[(size_t)j * dim + d];
}

template <int STEPS>
void vq_launch_assign(hipStream_t s, int n, int n_codes, int dim, const float* rows, const float* chunks, const uint16_t* prev,
                      uint16_t* indices, uint32_t* changed) {
    const unsigned blocks = (unsigned)((n + VQ_WG_POINTS - 1) / VQ_WG_POINTS);
    hipLaunchKernelGGL(vq_assign_kernel<STEPS>, dim3(blocks), dim3(VQ_THREADS), 0, s, n, n_codes, dim, rows, chunks, prev, indices,
                       changed);
}

}  // namespace

// scratch (16-byte aligned): the codebook as the assign kernel reads it, ceil(n_codes / 256) chunks
size_t gsr_vq_scratch_size(int n_codes, int dim) {
    return (size_t)vq_chunks(n_codes) * vq_chunk_floats(vq_steps(dim)) * sizeof(float);
}

void gsr_launch_vq_assign(hipStream_t s, int n, int n_codes, int dim, const float* rows, const float* codebook,
                          const uint16_t* prev, uint16_t* indices, float* err, uint32_t* changed, void* scratch) {
    if (n <= 0) return;
    float* chunks = reinterpret_cast<float*>(scratch);
    const int steps = vq_steps(dim);
    hipLaunchKernelGGL(vq_prep_kernel, dim3((unsigned)vq_chunks(n_codes)), dim3(VQ_THREADS), 0, s, n_codes, dim, steps, codebook,
                       chunks, changed);
    switch (steps) {
        case 4: vq_launch_assign<4>(s, n, n_codes, dim, rows, chunks, prev, indices, changed); break;
        case 8: vq_launch_assign<8>(s, n, n_codes, dim, rows, chunks, prev, indices, changed); break;
        case 12: vq_launch_assign<12>(s, n, n_codes, dim, rows, chunks, prev, indices, changed); break;
        case 16: vq_launch_assign<16>(s, n, n_codes, dim, rows, chunks, prev, indices, changed); break;
        case 20: vq_launch_assign<20>(s, n, n_codes, dim, rows, chunks, prev, indices, changed); break;
        default: vq_launch_assign<24>(s, n, n_codes, dim, rows, chunks, prev, indices, changed); break;
    }
    if (err) {
        const unsigned blocks = (unsigned)((n + VQ_THREADS - 1) / VQ_THREADS);
        hipLaunchKernelGGL(vq_err_kernel, dim3(blocks), dim3(VQ_THREADS), 0, s, n, n_codes, dim, rows, codebook, indices, err);
    }
}

void gsr_launch_vq_accumulate(hipStream_t s, int n, int n_codes, int dim, const float* rows, const uint16_t* indices,
                              const uint8_t* wq, long long* sums, unsigned long long* wsum) {
    if (n <= 0) return;
    const int rows_per_wg = VQ_ACC_ROWS * (VQ_THREADS / 64);
    const unsigned blocks = (unsigned)((n + rows_per_wg - 1) / rows_per_wg);
    hipLaunchKernelGGL(vq_accumulate_kernel, dim3(blocks), dim3(VQ_THREADS), 0, s, n, n_codes, dim, rows, indices, wq, sums, wsum);
}

void gsr_launch_vq_update(hipStream_t s, int n_codes, int dim, const long long* sums, const unsigned long long* wsum,
                          float* codebook, uint32_t* empty) {
    const unsigned blocks = (unsigned)((n_codes * dim + VQ_THREADS - 1) / VQ_THREADS);
    hipLaunchKernelGGL(vq_update_kernel, dim3(blocks), dim3(VQ_THREADS), 0, s, n_codes, dim, sums, wsum, codebook);
    if (empty) hipLaunchKernelGGL(vq_empty_kernel, dim3(1), dim3(VQ_THREADS), 0, s, n_codes, wsum, empty);
}

void gsr_launch_vq_decode(hipStream_t s, int n, int n_codes, int dim, const float* codebook, const uint16_t* indices,
                          float* rows_out) {
    if (n <= 0) return;
    const long long total = (long long)n * dim;
    const unsigned blocks = (unsigned)((total + VQ_THREADS - 1) / VQ_THREADS);
    hipLaunchKernelGGL(vq_decode_kernel, dim3(blocks), dim3(VQ_THREADS), 0, s, total, n_codes, dim, codebook, indices, rows_out);
}
