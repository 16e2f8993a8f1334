// The quantised model container (include/gsr.h gsr_quant_*): per-(block, column) ranges of an (n, cols) float32
// group, 8/16-bit codes, the decode, and the per-step quantise-dequantise pass of every group in one launch.
//
// Compiled with -ffp-contract=off: every operation of the header's definition is ONE rounded fp32 operation (the divisions
// and the square root are the correctly rounded ones, subnormals are kept), and the one fused operation of the decode is
// written out as __builtin_fmaf.  tests/quant_ref.py restates it in numpy; the kernels are held to it bit for bit.
//
// Two access regimes:
//   cols <= 4 : a lane owns a ROW (consecutive lanes, consecutive rows: a wave reads one contiguous run of bytes; float4 /
//               uchar4 / ushort4 accesses at cols = 4 where the arrays' alignment allows);
//   cols  > 4 : lane d owns COLUMN d (as vq_accumulate_kernel): a row is one coalesced read, and a lane's range, 1 / step and
//               step are computed once per 64 rows instead of once per element.
// block_rows is a multiple of 64, so the 64 rows of a wave always lie in one block: the block number is wave-uniform.
// Bandwidth kernels: no LDS beyond the range reduction, no scratch memory.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsr.h"
#include "gsr_kernels.h"
#include "wave_reduce.h"

namespace {

constexpr int Q_THREADS = 256;        // 4 waves
constexpr int Q_WG_ROWS = 256;        // rows of one workgroup of the encode / decode / fake kernels
constexpr int Q_RANGE_ROWS = 1024;    // rows of one workgroup of the one-block range reduction
constexpr int Q_MAX_COLS = 48;

// ---- the monotone integer key of a float's bits: unsigned order = the order -Inf < ... < -0 < +0 < ... < +Inf ----
__device__ __forceinline__ uint32_t q_key(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ uint32_t q_unkey(uint32_t k) { return (k >> 31) ? k ^ 0x80000000u : ~k; }
constexpr uint32_t Q_KMIN_NONE = 0xFFFFFFFFu, Q_KMAX_NONE = 0u;   // keys of NaN bit patterns: no finite value has them

__device__ __forceinline__ void q_see(float x, uint32_t& kmin, uint32_t& kmax) {
    const uint32_t b = __float_as_uint(x);
    if ((b & 0x7F800000u) != 0x7F800000u) {
        const uint32_t k = q_key(b);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
    }
}

// ---- the definition's per-(block, column) constants and its two maps ----
struct QParam {
    float lo, inv, step, Lf;
    uint32_t L;
    bool ok;
};

__device__ __forceinline__ QParam q_param(float lo, float hi, int bits) {
    QParam p;
    p.L = (1u << bits) - 1u;
    p.Lf = (float)p.L;
    const float span = hi - lo;
    p.ok = span > 0.0f && span < __builtin_inff();
    p.lo = lo;
    p.inv = p.Lf / span;
    p.step = span / p.Lf;
    return p;
}

__device__ __forceinline__ uint32_t q_encode(float x, const QParam& p) {
    float t = (x - p.lo) * p.inv;
    t = (t != t) ? 0.0f : fminf(fmaxf(t, 0.0f), p.Lf);
    const uint32_t q = (uint32_t)rintf(t);
    return p.ok ? q : 0u;
}

__device__ __forceinline__ float q_decode(uint32_t q, const QParam& p) {
    q = q < p.L ? q : p.L;
    return p.ok ? __builtin_fmaf((float)q, p.step, p.lo) : p.lo;
}

// (w, x, y, z) normalised, with w >= 0; a row without a positive finite squared norm becomes (1, 0, 0, 0)
__device__ __forceinline__ void q_unit_quat(float (&v)[4]) {
    const float n2 = ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3];
    if (n2 > 0.0f && n2 < __builtin_inff()) {
        const float inv = 1.0f / sqrtf(n2);
        const float s = v[0] < 0.0f ? -inv : inv;
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = v[k] * s;
    } else {
        v[0] = 1.0f; v[1] = 0.0f; v[2] = 0.0f; v[3] = 0.0f;
    }
}

// ---- ranges ----
// One workgroup per unit of `unit_rows` rows.  C = 1..4: thread t takes rows t, t + 256, ... of the unit and keeps C key
// pairs; C = 0: wave w takes rows w, w + 4, ... and lane d column d.  The waves meet in LDS; then either the unit IS a block
// and its floats are written (atomic = 0), or the unit is a slice of the one block and the keys go through integer min / max
// atomics into `ranges` itself, which q_ranges_begin filled with the identities and q_ranges_end turns into floats.
template <int C>
__global__ __launch_bounds__(Q_THREADS) void q_ranges_kernel(long long n, int cols, const float* __restrict__ rows, int unit_rows,
                                                            int atomic, float* __restrict__ ranges) {
    __shared__ uint32_t red[Q_THREADS / 64][2][Q_MAX_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r0 = (long long)blockIdx.x * unit_rows;
    const long long r1 = n - r0 < unit_rows ? n : r0 + unit_rows;
    if (C > 0) {
        constexpr int CC = C > 0 ? C : 1;
        uint32_t kmin[CC], kmax[CC];
#pragma unroll
        for (int c = 0; c < CC; c++) { kmin[c] = Q_KMIN_NONE; kmax[c] = Q_KMAX_NONE; }
        const bool vec = C == 4 && ((uintptr_t)rows & 15) == 0;
        for (long long r = r0 + tid; r < r1; r += Q_THREADS) {
            float x[CC];
            if (vec) {
                const float4 v = *reinterpret_cast<const float4*>(rows + (size_t)r * 4);
                x[0] = v.x; x[CC > 1 ? 1 : 0] = v.y; x[CC > 2 ? 2 : 0] = v.z; x[CC > 3 ? 3 : 0] = v.w;
            } else {
#pragma unroll
                for (int c = 0; c < CC; c++) x[c] = rows[(size_t)r * CC + c];
            }
#pragma unroll
            for (int c = 0; c < CC; c++) q_see(x[c], kmin[c], kmax[c]);
        }
#pragma unroll
        for (int c = 0; c < CC; c++) {   // every lane takes part: the identities are the idle lanes' values
            const uint32_t mx = gsr::wave_max_u32(kmax[c]);
            const uint32_t mn = ~gsr::wave_max_u32(~kmin[c]);
            if (lane == 0) { red[wave][0][c] = mn; red[wave][1][c] = mx; }
        }
    } else {
        uint32_t kmin = Q_KMIN_NONE, kmax = Q_KMAX_NONE;
        if (lane < cols) {
            for (long long r = r0 + wave; r < r1; r += 4 * (Q_THREADS / 64)) {
                float x[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const long long q = r + u * (Q_THREADS / 64);
                    x[u] = q < r1 ? rows[(size_t)q * cols + lane] : __builtin_nanf("");
                }
#pragma unroll
                for (int u = 0; u < 4; u++) q_see(x[u], kmin, kmax);
            }
            red[wave][0][lane] = kmin; red[wave][1][lane] = kmax;
        }
    }
    __syncthreads();
    if (tid >= cols) return;
    uint32_t mn = red[0][0][tid], mx = red[0][1][tid];
#pragma unroll
    for (int w = 1; w < Q_THREADS / 64; w++) {
        mn = red[w][0][tid] < mn ? red[w][0][tid] : mn;
        mx = red[w][1][tid] > mx ? red[w][1][tid] : mx;
    }
    if (atomic) {
        uint32_t* keys = reinterpret_cast<uint32_t*>(ranges);
        if (mn != Q_KMIN_NONE) {
            atomicMin(keys + tid, mn);
            atomicMax(keys + cols + tid, mx);
        }
    } else {
        float* out = ranges + (size_t)blockIdx.x * 2 * cols;
        const bool any = mn != Q_KMIN_NONE;
        out[tid] = any ? __uint_as_float(q_unkey(mn)) : 0.0f;
        out[cols + tid] = any ? __uint_as_float(q_unkey(mx)) : 0.0f;
    }
}

__global__ void q_ranges_begin(int cols, uint32_t* __restrict__ keys) {
    const int t = threadIdx.x;
    if (t < 2 * cols) keys[t] = t < cols ? Q_KMIN_NONE : Q_KMAX_NONE;
}

__global__ void q_ranges_end(int cols, uint32_t* __restrict__ keys) {
    const int t = threadIdx.x;
    if (t >= 2 * cols) return;
    const uint32_t k = keys[t], none = t < cols ? Q_KMIN_NONE : Q_KMAX_NONE;
    keys[t] = k == none ? 0u : q_unkey(k);
}

// ---- encode / decode / fake: one kernel, a workgroup belongs to one group and covers Q_WG_ROWS rows of it ----
enum { OP_ENCODE = 0, OP_DECODE = 1, OP_FAKE = 2 };

struct QuantGroups {
    const float* in[GSR_QUANT_MAX_GROUPS];
    float* out[GSR_QUANT_MAX_GROUPS];
    void* codes[GSR_QUANT_MAX_GROUPS];
    const float* ranges[GSR_QUANT_MAX_GROUPS];
    int cols[GSR_QUANT_MAX_GROUPS], bits[GSR_QUANT_MAX_GROUPS], kind[GSR_QUANT_MAX_GROUPS], block_rows[GSR_QUANT_MAX_GROUPS];
    long long block_start[GSR_QUANT_MAX_GROUPS + 1];   // first workgroup of each group
    long long n;
    int n_groups;
};

// cols = C <= 4: this thread's row.  `in` and `out` may be the same array: a thread reads its row before it writes it.
template <int OP, int C, class CT>
__device__ __forceinline__ void q_row_lane(long long n, int bits, int kind, int block_rows, const float* in, float* out, CT* codes,
                                           const float* __restrict__ ranges, long long row) {
    if (row >= n) return;
    const bool quat = C == 4 && kind == GSR_QUANT_UNIT_QUAT;
    QParam p[C];
    if (quat) {
#pragma unroll
        for (int c = 0; c < C; c++) p[c] = q_param(-1.0f, 1.0f, bits);
    } else {
        const float* rg = ranges + (size_t)(block_rows ? row / block_rows : 0) * 2 * C;
#pragma unroll
        for (int c = 0; c < C; c++) p[c] = q_param(rg[c], rg[C + c], bits);
    }
    uint32_t q[C];
    if (OP != OP_DECODE) {
        float x[C];
        if (C == 4 && ((uintptr_t)in & 15) == 0) {
            const float4 v = *reinterpret_cast<const float4*>(in + (size_t)row * 4);
            x[0] = v.x; x[C > 1 ? 1 : 0] = v.y; x[C > 2 ? 2 : 0] = v.z; x[C > 3 ? 3 : 0] = v.w;
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) x[c] = in[(size_t)row * C + c];
        }
        if constexpr (C == 4) {
            if (quat) q_unit_quat(x);
        }
#pragma unroll
        for (int c = 0; c < C; c++) q[c] = q_encode(x[c], p[c]);
    } else {
        if (C == 4 && ((uintptr_t)codes & (4 * sizeof(CT) - 1)) == 0) {
            if (sizeof(CT) == 1) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(codes + (size_t)row * 4);
#pragma unroll
                for (int c = 0; c < C; c++) q[c] = (w >> (8 * c)) & 0xFFu;
            } else {
                const uint2 w = *reinterpret_cast<const uint2*>(codes + (size_t)row * 4);
#pragma unroll
                for (int c = 0; c < C; c++) q[c] = ((c < 2 ? w.x : w.y) >> (16 * (c & 1))) & 0xFFFFu;
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) q[c] = codes[(size_t)row * C + c];
        }
    }
    if (OP == OP_ENCODE) {
        if (C == 4 && ((uintptr_t)codes & (4 * sizeof(CT) - 1)) == 0) {
            const uint32_t q1 = q[C > 1 ? 1 : 0], q2 = q[C > 2 ? 2 : 0], q3 = q[C > 3 ? 3 : 0];   // every code is <= 2^bits - 1
            if (sizeof(CT) == 1) *reinterpret_cast<uint32_t*>(codes + (size_t)row * 4) = q[0] | (q1 << 8) | (q2 << 16) | (q3 << 24);
            else *reinterpret_cast<uint2*>(codes + (size_t)row * 4) = make_uint2(q[0] | (q1 << 16), q2 | (q3 << 16));
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) codes[(size_t)row * C + c] = (CT)q[c];
        }
    } else {
        float y[C];
#pragma unroll
        for (int c = 0; c < C; c++) y[c] = q_decode(q[c], p[c]);
        if (C == 4 && ((uintptr_t)out & 15) == 0) {
            *reinterpret_cast<float4*>(out + (size_t)row * 4) = make_float4(y[0], y[C > 1 ? 1 : 0], y[C > 2 ? 2 : 0], y[C > 3 ? 3 : 0]);
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) out[(size_t)row * C + c] = y[c];
        }
    }
}

// any cols (used above 4): this wave's 64 rows [row0, row0 + 64), lane d column d; the rows lie in one block
template <int OP, class CT>
__device__ __forceinline__ void q_rows_wave(long long n, int cols, int bits, int block_rows, const float* in, float* out, CT* codes,
                                            const float* __restrict__ ranges, long long row0, int lane) {
    if (row0 >= n || lane >= cols) return;
    const long long row1 = n - row0 < 64 ? n : row0 + 64;
    const float* rg = ranges + (size_t)(block_rows ? row0 / block_rows : 0) * 2 * cols;
    const QParam p = q_param(rg[lane], rg[cols + lane], bits);
    for (long long r = row0; r < row1; r += 4) {
        uint32_t q[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t e = (size_t)(r + u < row1 ? r + u : row1 - 1) * cols + lane;   // a slot past the end repeats the last row
            q[u] = OP != OP_DECODE ? q_encode(in[e], p) : (uint32_t)codes[e];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (r + u >= row1) break;
            const size_t e = (size_t)(r + u) * cols + lane;
            if (OP == OP_ENCODE) codes[e] = (CT)q[u];
            else out[e] = q_decode(q[u], p);
        }
    }
}

template <int OP, class CT>
__device__ __forceinline__ void q_group(const QuantGroups& G, int g, long long blk) {
    const long long n = G.n;
    const int cols = G.cols[g], bits = G.bits[g], kind = G.kind[g], block_rows = G.block_rows[g];
    const float* in = G.in[g];
    float* out = G.out[g];
    CT* codes = reinterpret_cast<CT*>(G.codes[g]);
    const float* ranges = G.ranges[g];
    const long long row = blk * Q_WG_ROWS + threadIdx.x;
    switch (cols) {
        case 1: q_row_lane<OP, 1, CT>(n, bits, kind, block_rows, in, out, codes, ranges, row); break;
        case 2: q_row_lane<OP, 2, CT>(n, bits, kind, block_rows, in, out, codes, ranges, row); break;
        case 3: q_row_lane<OP, 3, CT>(n, bits, kind, block_rows, in, out, codes, ranges, row); break;
        case 4: q_row_lane<OP, 4, CT>(n, bits, kind, block_rows, in, out, codes, ranges, row); break;
        default:
            q_rows_wave<OP, CT>(n, cols, bits, block_rows, in, out, codes, ranges, blk * Q_WG_ROWS + (threadIdx.x >> 6) * 64,
                                threadIdx.x & 63);
    }
}

template <int OP>
__global__ __launch_bounds__(Q_THREADS) void q_op_kernel(QuantGroups G) {
    int g = 0;
#pragma unroll
    for (int k = 1; k < GSR_QUANT_MAX_GROUPS; k++)
        if (k < G.n_groups && (long long)blockIdx.x >= G.block_start[k]) g = k;
    const long long blk = (long long)blockIdx.x - G.block_start[g];
    if (OP == OP_FAKE || G.bits[g] <= 8) q_group<OP, uint8_t>(G, g, blk);   // the fake pass writes no codes: their width is moot
    else q_group<OP, uint16_t>(G, g, blk);
}

template <int OP>
void q_launch(hipStream_t s, int n_groups, long long n, const float* const* in, float* const* out, void* const* codes,
              const float* const* ranges, const int* cols, const int* bits, const int* kind, const int* block_rows) {
    if (n <= 0 || n_groups <= 0) return;
    QuantGroups G;
    const long long blocks = (n + Q_WG_ROWS - 1) / Q_WG_ROWS;
    for (int g = 0; g < GSR_QUANT_MAX_GROUPS; g++) {
        const int k = g < n_groups ? g : 0;
        G.in[g] = in ? in[k] : nullptr; G.out[g] = out ? out[k] : nullptr; G.codes[g] = codes ? codes[k] : nullptr;
        G.ranges[g] = ranges[k]; G.cols[g] = cols[k]; G.bits[g] = bits[k]; G.kind[g] = kind[k]; G.block_rows[g] = block_rows[k];
        G.block_start[g] = (long long)(g < n_groups ? g : n_groups) * blocks;
    }
    G.block_start[GSR_QUANT_MAX_GROUPS] = (long long)n_groups * blocks;
    G.n = n;
    G.n_groups = n_groups;
    hipLaunchKernelGGL(q_op_kernel<OP>, dim3((unsigned)(blocks * n_groups)), dim3(Q_THREADS), 0, s, G);
}

}  // namespace

void gsr_launch_quant_ranges(hipStream_t s, long long n, int cols, const float* rows, int block_rows, float* ranges) {
    const int unit = block_rows ? block_rows : Q_RANGE_ROWS;
    const unsigned blocks = (unsigned)((n + unit - 1) / unit);
    const int atomic = block_rows ? 0 : 1;
    if (atomic) hipLaunchKernelGGL(q_ranges_begin, dim3(1), dim3(128), 0, s, cols, reinterpret_cast<uint32_t*>(ranges));
    if (blocks) {
        switch (cols) {
            case 1: hipLaunchKernelGGL(q_ranges_kernel<1>, dim3(blocks), dim3(Q_THREADS), 0, s, n, cols, rows, unit, atomic, ranges); break;
            case 2: hipLaunchKernelGGL(q_ranges_kernel<2>, dim3(blocks), dim3(Q_THREADS), 0, s, n, cols, rows, unit, atomic, ranges); break;
            case 3: hipLaunchKernelGGL(q_ranges_kernel<3>, dim3(blocks), dim3(Q_THREADS), 0, s, n, cols, rows, unit, atomic, ranges); break;
            case 4: hipLaunchKernelGGL(q_ranges_kernel<4>, dim3(blocks), dim3(Q_THREADS), 0, s, n, cols, rows, unit, atomic, ranges); break;
            default: hipLaunchKernelGGL(q_ranges_kernel<0>, dim3(blocks), dim3(Q_THREADS), 0, s, n, cols, rows, unit, atomic, ranges);
        }
    }
    if (atomic) hipLaunchKernelGGL(q_ranges_end, dim3(1), dim3(128), 0, s, cols, reinterpret_cast<uint32_t*>(ranges));
}

void gsr_launch_quant_encode(hipStream_t s, long long n, int cols, int bits, int kind, const float* rows, int block_rows,
                             const float* ranges, void* codes) {
    q_launch<OP_ENCODE>(s, 1, n, &rows, nullptr, &codes, &ranges, &cols, &bits, &kind, &block_rows);
}

void gsr_launch_quant_decode(hipStream_t s, long long n, int cols, int bits, int kind, const void* codes, int block_rows,
                             const float* ranges, float* rows_out) {
    void* c = const_cast<void*>(codes);
    q_launch<OP_DECODE>(s, 1, n, nullptr, &rows_out, &c, &ranges, &cols, &bits, &kind, &block_rows);
}

void gsr_launch_quant_fake(hipStream_t s, int n_groups, long long n, const float* const* in, float* const* out,
                           const float* const* ranges, const int* cols, const int* bits, const int* kind, const int* block_rows) {
    q_launch<OP_FAKE>(s, n_groups, n, in, out, nullptr, ranges, cols, bits, kind, block_rows);
}
