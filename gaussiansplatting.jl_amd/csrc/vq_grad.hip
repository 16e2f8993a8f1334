// SH codebook fine-tuning: the pullback of features_rest[i] = codebook[indices[i]], a scatter-add of n rows into n_codes rows
// without float atomics (the definition is the header's, include/gsr.h gsr_vq_group / gsr_vq_codebook_grad).
// Every sum is a chain of single rounded fp32 adds in a fixed order, so the result is the restatement's bits
// (tests/vq_grad_ref.py) in every run.
//
//   group  : once per set of indices.  offsets = the exclusive scan of the per-code counts (integer atomics: counts only);
//            order = the stable LSD radix sort of the row numbers by the clamped 16-bit code, two 8-bit passes.  A pass is
//            hist (one wave per GROUP_ROWS rows: its 256 digit counts), block_scan_carry over (digit, workgroup), and
//            scatter: the same wave walks its rows 64 at a time IN ROW ORDER; a lane's rank among the lanes of its digit
//            comes from eight ballots, its position is the scanned base + the digit's running count + that rank.  No atomic
//            decides a position: order is the same integers in every run.
//   prefix : ONE workgroup, per call.  pre_l[j] = the first output slot of code j at level l, K + 1 entries per level:
//            the exclusive scan of c_l[j] = ceil(c_{l-1}[j] / R), c_0 the code's row count.
//   level  : a wave owns one slot = one chunk of <= R consecutive entries of one code's list at that level.  It finds its
//            code with a 64-ary search of pre_l (three dependent loads for 65536 codes), lane d owns column d, the loads of
//            VQG_AHEAD rows are issued before their serial adds.  Level 1 reads g_rows through `order`, the later levels
//            read the partial rows of the level before from the scratch.  A chunk that is its code's only one writes
//            g_codebook, any other writes its slot of the scratch; a code that was complete at an earlier level is skipped.
//            The first launch also writes the +0 rows of the empty codes (extra workgroups behind the slots).
// Robustness: every index that comes from `order`, `offsets` or a prefix derived from them is clamped before it is used.
#include "gsr_kernels.h"
#include "block_reduce.h"
#include "../../include/gsr.h"

namespace {

constexpr int R = GSR_VQ_SUM_RADIX;
static_assert(R == 64, "a chunk is walked by one wave whose lane i holds the chunk's i-th source index");
constexpr int VQG_THREADS = 256;            // level kernel: four waves, four slots
constexpr int VQG_AHEAD = 16;               // rows whose loads are in flight before the first of their adds
constexpr int GROUP_ROWS = 1024;            // rows of one sort workgroup (ONE wave: 16 steps of 64 rows, in row order)
constexpr int SCAN_THREADS = 1024;          // block_scan_carry's workgroup

__host__ __device__ inline int vqg_levels(long long n) { return n <= 64 ? 1 : n <= 4096 ? 2 : n <= 262144 ? 3 : 4; }
__host__ __device__ inline long long vqg_pow(int l) { return 1ll << (6 * l); }
// the slots of level l: at most floor(n / R^l) + min(K, n)
__host__ __device__ inline long long vqg_cap(long long n, int K, int l) { return n / vqg_pow(l) + (K < n ? K : n); }
inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
inline int group_wgs(long long n) { return (int)((n + GROUP_ROWS - 1) / GROUP_ROWS); }

// ---------------------------------------------------------------- group ----
__global__ __launch_bounds__(VQG_THREADS) void vqg_zero_kernel(int count, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * VQG_THREADS + threadIdx.x;
    if (i < count) out[i] = 0;
}

__global__ __launch_bounds__(VQG_THREADS) void vqg_count_kernel(int n, int K, const uint16_t* __restrict__ indices,
                                                                uint32_t* __restrict__ counts) {
    const int i = blockIdx.x * VQG_THREADS + threadIdx.x;
    if (i >= n) return;
    int j = indices[i];
    j = j < K ? j : K - 1;
    atomicAdd(counts + j, 1u);   // integer: any order, the same count
}

// ONE workgroup: a[0..nb) <- its exclusive prefix sums, a[nb] <- the total
__global__ __launch_bounds__(SCAN_THREADS) void vqg_scan_kernel(int nb, uint32_t* __restrict__ a) {
    gsr::block_scan_carry<uint32_t>(nb, a, a + nb);
}

// the digit of row i in pass PASS: pass 0 reads the indices (clamped), pass 1 the keys pass 0 wrote
template <int PASS>
__device__ __forceinline__ uint32_t vqg_key(int i, int K, const uint16_t* __restrict__ keys) {
    uint32_t k = keys[i];
    if (PASS == 0) k = k < (uint32_t)K ? k : (uint32_t)(K - 1);
    return k;
}

template <int PASS>
__global__ __launch_bounds__(64) void vqg_hist_kernel(int n, int K, int n_wg, const uint16_t* __restrict__ keys,
                                                      uint32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[256];
    const int lane = threadIdx.x;
    for (int d = lane; d < 256; d += 64) cnt[d] = 0;
    __syncthreads();
    const int r0 = blockIdx.x * GROUP_ROWS;
    for (int s = 0; s < GROUP_ROWS; s += 64) {
        const int i = r0 + s + lane;
        if (i < n) {
            const uint32_t k = vqg_key<PASS>(i, K, keys);
            atomicAdd(&cnt[PASS == 0 ? (k & 255u) : (k >> 8)], 1u);
        }
    }
    __syncthreads();
    for (int d = lane; d < 256; d += 64) hist[(size_t)d * n_wg + blockIdx.x] = cnt[d];
}

template <int PASS>
__global__ __launch_bounds__(64) void vqg_scatter_kernel(int n, int K, int n_wg, const uint16_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ vals_in, const uint32_t* __restrict__ hist,
                                                         uint16_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
    __shared__ uint32_t base[256];
    const int lane = threadIdx.x;
    for (int d = lane; d < 256; d += 64) base[d] = hist[(size_t)d * n_wg + blockIdx.x];
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    const int r0 = blockIdx.x * GROUP_ROWS;
    for (int s = 0; s < GROUP_ROWS; s += 64) {   // 64 rows at a time, in row order
        if (r0 + s >= n) break;                  // wave-uniform
        const int i = r0 + s + lane;
        const bool valid = i < n;
        const uint32_t k = valid ? vqg_key<PASS>(i, K, keys) : 0u;
        const uint32_t d = PASS == 0 ? (k & 255u) : (k >> 8);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const unsigned long long m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below);
        const uint32_t pos = valid ? base[d] + rank : 0u;
        __syncthreads();   // every lane has read base[] before the digits' leaders move it on
        if (valid && (peers >> lane) == 1ull) base[d] += (uint32_t)__popcll(peers);   // the digit's highest lane
        __syncthreads();
        if (valid && pos < (uint32_t)n) {
            if (PASS == 0) {
                keys_out[pos] = (uint16_t)k;
                vals_out[pos] = (uint32_t)i;
            } else {
                vals_out[pos] = vals_in[i];
            }
        }
    }
}

// ---------------------------------------------------------------- gradient ----
// rows of code j, from offsets read as min(offsets[.], n); an end before its start is an empty code
__device__ __forceinline__ void vqg_code_range(const uint32_t* __restrict__ offsets, uint32_t n, int j, uint32_t& start,
                                               uint32_t& count) {
    uint32_t a = offsets[j], b = offsets[j + 1];
    a = a < n ? a : n;
    b = b < n ? b : n;
    start = a;
    count = b > a ? b - a : 0u;
}

// ONE workgroup: pre[l - 1][0 .. K] for l = 1 .. levels
__global__ __launch_bounds__(SCAN_THREADS) void vqg_prefix_kernel(uint32_t n, int K, int levels, const uint32_t* __restrict__ offsets,
                                                                  uint32_t* __restrict__ pre) {
    for (int l = 0; l < levels; l++) {
        uint32_t* __restrict__ cur = pre + (size_t)l * (K + 1);
        const uint32_t* prev = l ? cur - (K + 1) : cur;
        for (int j = threadIdx.x; j < K; j += SCAN_THREADS) {
            uint32_t c, start = 0;
            if (l == 0) vqg_code_range(offsets, n, j, start, c);
            else c = prev[j + 1] - prev[j];
            (void)start;
            cur[j] = (c + (uint32_t)(R - 1)) / (uint32_t)R;
        }
        __syncthreads();
        gsr::block_scan_carry<uint32_t>(K, cur, cur + K);
        __syncthreads();
    }
}

// the largest j in [0, K) with pre[j] <= s, for a non-decreasing pre; some j in [0, K) for any other.  Wave-uniform.
__device__ __forceinline__ int vqg_find_code(const uint32_t* __restrict__ pre, int K, uint32_t s, int lane) {
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int step = (hi - lo + 63) >> 6;
        const int idx = lo + lane * step;
        const bool le = idx < hi && pre[idx] <= s;
        const unsigned long long m = __ballot(le);
        const int t = m ? 63 - __builtin_clzll(m) : 0;
        lo += t * step;
        hi = hi < lo + step ? hi : lo + step;
    }
    return lo;
}

// LEVEL1: the sources are g_rows[order[.]], else the partial rows `src` of the level before.
//   pre      : this level's slot prefix (K + 1);  pre_prev: the level before's (LEVEL1: unused)
//   cap      : the slots this launch covers;  cap_prev: the slots of `src`
//   dst      : this level's partial rows, or nullptr at the last level (every slot then writes g_codebook)
//   zero_wg0 : LEVEL1 — the first of the workgroups that write the +0 rows of the empty codes
template <bool LEVEL1>
__global__ __launch_bounds__(VQG_THREADS) void vqg_level_kernel(uint32_t n, int K, int dim, const float* __restrict__ g_rows,
                                                                long long row_stride, const uint32_t* __restrict__ order,
                                                                const uint32_t* __restrict__ offsets,
                                                                const uint32_t* __restrict__ pre,
                                                                const uint32_t* __restrict__ pre_prev, uint32_t cap,
                                                                uint32_t cap_prev, const float* __restrict__ src,
                                                                float* __restrict__ dst, float* __restrict__ g_codebook,
                                                                uint32_t zero_wg0) {
    const int lane = threadIdx.x & 63;
    if (LEVEL1 && blockIdx.x >= zero_wg0) {
        const long long e = (long long)(blockIdx.x - zero_wg0) * VQG_THREADS + threadIdx.x;
        if (e >= (long long)K * dim) return;
        uint32_t start, count;
        vqg_code_range(offsets, n, (int)(e / dim), start, count);
        if (count == 0) g_codebook[e] = 0.0f;
        return;
    }
    const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (VQG_THREADS / 64) + (threadIdx.x >> 6)));
    if (s >= cap || s >= pre[K]) return;
    const int j = __builtin_amdgcn_readfirstlane(vqg_find_code(pre, K, s, lane));
    const unsigned long long first = 64ull * (unsigned long long)(s - pre[j]);   // of this chunk, within the code's list
    unsigned long long base;   // of the code's list, in `order` / in `src`
    uint32_t len;              // the list's length
    if (LEVEL1) {
        uint32_t start;
        vqg_code_range(offsets, n, j, start, len);
        base = start;
    } else {
        base = pre_prev[j];
        len = pre_prev[j + 1] - pre_prev[j];
        if (len <= 1) return;   // complete at an earlier level
    }
    if (first >= len) return;
    const int m = __builtin_amdgcn_readfirstlane(len - first < 64ull ? (int)(len - first) : 64);
    // lane i: the chunk's i-th source row
    unsigned long long p = base + first + (unsigned long long)(lane < m ? lane : m - 1);
    uint32_t mine;
    if (LEVEL1) {
        p = p < n ? p : n - 1;
        mine = order[p];
        mine = mine < n ? mine : n - 1;
    } else {
        mine = (uint32_t)(p < cap_prev ? p : cap_prev - 1);
    }
    const float* __restrict__ from = LEVEL1 ? g_rows : src;
    const size_t stride = LEVEL1 ? (size_t)row_stride : (size_t)dim;
    const bool col = lane < dim;
    float acc = 0.0f;
    for (int i0 = 0; i0 < m; i0 += VQG_AHEAD) {   // m is wave-uniform
        float v[VQG_AHEAD];
#pragma unroll
        for (int u = 0; u < VQG_AHEAD; u++) {
            const int i = i0 + u < m ? i0 + u : m - 1;
            const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)mine, i);
            v[u] = col ? from[(size_t)r * stride + lane] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < VQG_AHEAD; u++) {
            if (i0 + u < m) acc = (i0 + u == 0) ? v[u] : acc + v[u];   // the first entry is taken, not added
        }
    }
    if (!col) return;
    const bool last = (pre[j + 1] - pre[j]) == 1u || dst == nullptr;
    if (last) g_codebook[(size_t)j * dim + lane] = acc;
    else dst[(size_t)s * dim + lane] = acc;
}

struct GradPlan {
    int levels;
    size_t pre_bytes;
    size_t part_off[4];   // partial rows of level l = 1 .. levels - 1 at part_off[l]
    size_t total;
};

GradPlan grad_plan(long long n, int K, int dim) {
    GradPlan p{};
    p.levels = vqg_levels(n);
    p.pre_bytes = align16((size_t)p.levels * (K + 1) * sizeof(uint32_t));
    size_t off = p.pre_bytes;
    for (int l = 1; l < p.levels; l++) {
        p.part_off[l] = off;
        off += align16((size_t)vqg_cap(n, K, l) * dim * sizeof(float));
    }
    p.total = off;
    return p;
}

}  // namespace

// scratch (16-byte aligned): [ pass 0's row numbers, n uint32 | hist, 256 * workgroups + 1 uint32 | pass 0's keys, n uint16 ]
size_t gsr_vq_group_scratch_size(long long n, int n_codes) {
    return align16((size_t)n * 4) + align16(((size_t)256 * group_wgs(n) + 1) * 4) + align16((size_t)n * 2);
}

void gsr_launch_vq_group(hipStream_t s, int n, int n_codes, const uint16_t* indices, uint32_t* order, uint32_t* offsets,
                         void* scratch) {
    if (n <= 0) return;
    const int n_wg = group_wgs(n);
    char* base = reinterpret_cast<char*>(scratch);
    uint32_t* vals = reinterpret_cast<uint32_t*>(base);
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + align16((size_t)n * 4));
    uint16_t* keys = reinterpret_cast<uint16_t*>(base + align16((size_t)n * 4) + align16(((size_t)256 * n_wg + 1) * 4));
    const unsigned row_blocks = (unsigned)((n + VQG_THREADS - 1) / VQG_THREADS);
    hipLaunchKernelGGL(vqg_zero_kernel, dim3((unsigned)((n_codes + 1 + VQG_THREADS - 1) / VQG_THREADS)), dim3(VQG_THREADS), 0, s,
                       n_codes + 1, offsets);
    hipLaunchKernelGGL(vqg_count_kernel, dim3(row_blocks), dim3(VQG_THREADS), 0, s, n, n_codes, indices, offsets);
    hipLaunchKernelGGL(vqg_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, n_codes, offsets);
    hipLaunchKernelGGL(vqg_hist_kernel<0>, dim3((unsigned)n_wg), dim3(64), 0, s, n, n_codes, n_wg, indices, hist);
    hipLaunchKernelGGL(vqg_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, 256 * n_wg, hist);
    hipLaunchKernelGGL(vqg_scatter_kernel<0>, dim3((unsigned)n_wg), dim3(64), 0, s, n, n_codes, n_wg, indices,
                       (const uint32_t*)nullptr, hist, keys, vals);
    hipLaunchKernelGGL(vqg_hist_kernel<1>, dim3((unsigned)n_wg), dim3(64), 0, s, n, n_codes, n_wg, keys, hist);
    hipLaunchKernelGGL(vqg_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, 256 * n_wg, hist);
    hipLaunchKernelGGL(vqg_scatter_kernel<1>, dim3((unsigned)n_wg), dim3(64), 0, s, n, n_codes, n_wg, keys, vals, hist,
                       (uint16_t*)nullptr, order);
}

// scratch (16-byte aligned): [ the slot prefixes, levels x (n_codes + 1) uint32 | the partial rows of level 1 | level 2 | .. ]
size_t gsr_vq_codebook_grad_scratch_size(long long n, int n_codes, int dim) { return grad_plan(n, n_codes, dim).total; }

void gsr_launch_vq_codebook_grad(hipStream_t s, int n, int n_codes, int dim, const float* g_rows, long long row_stride,
                                 const uint32_t* order, const uint32_t* offsets, float* g_codebook, void* scratch) {
    if (n <= 0) return;
    const GradPlan plan = grad_plan(n, n_codes, dim);
    char* base = reinterpret_cast<char*>(scratch);
    uint32_t* pre = reinterpret_cast<uint32_t*>(base);
    hipLaunchKernelGGL(vqg_prefix_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, (uint32_t)n, n_codes, plan.levels, offsets, pre);
    const int wps = VQG_THREADS / 64;
    for (int l = 1; l <= plan.levels; l++) {
        const uint32_t cap = (uint32_t)vqg_cap(n, n_codes, l);
        const uint32_t slot_wgs = (cap + wps - 1) / wps;
        const uint32_t* pre_l = pre + (size_t)(l - 1) * (n_codes + 1);
        float* dst = l < plan.levels ? reinterpret_cast<float*>(base + plan.part_off[l]) : nullptr;
        if (l == 1) {
            const uint32_t zero_wgs = (uint32_t)(((long long)n_codes * dim + VQG_THREADS - 1) / VQG_THREADS);
            hipLaunchKernelGGL(vqg_level_kernel<true>, dim3(slot_wgs + zero_wgs), dim3(VQG_THREADS), 0, s, (uint32_t)n, n_codes, dim,
                               g_rows, row_stride, order, offsets, pre_l, (const uint32_t*)nullptr, cap, 0u,
                               (const float*)nullptr, dst, g_codebook, slot_wgs);
        } else {
            const float* src = reinterpret_cast<const float*>(base + plan.part_off[l - 1]);
            hipLaunchKernelGGL(vqg_level_kernel<false>, dim3(slot_wgs), dim3(VQG_THREADS), 0, s, (uint32_t)n, n_codes, dim, g_rows,
                               row_stride, order, offsets, pre_l, pre_l - (n_codes + 1), cap, (uint32_t)vqg_cap(n, n_codes, l - 1),
                               src, dst, g_codebook, 0u);
        }
    }
}
