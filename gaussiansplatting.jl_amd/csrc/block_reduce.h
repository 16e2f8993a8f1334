// Fixed-order workgroup sums and integer block scans of the loss and trainer kernels (depth, geometry, bilateral, mcmc,
// trainer, ssim).  Results are bit-identical run to run, so the ORDER of a helper's additions is its contract: it is stated
// at the helper, and a change of it changes bits.  pergauss.hip (pose_final_kernel) and binning.hip (its scans) keep copies
// of their own: bench.py's counter staleness guard hashes those files, and an edit would retire the recorded counters.
//
// Two spellings that this header replaced differed from it, both without a change of bits:
//  - mcmc_reg_kernel summed a wave with __shfl_down and used lane 0's value.  At step `off`, lane k < off reads lane
//    k + off = k ^ off in both butterflies, its own value on the left of the `+`: by induction the lanes below `off` hold
//    the same bits after every step (and fp addition is commutative besides).  Only lane 0's value was used.
//  - the loss head's finish summed its wave totals as ((0.0f + red[0]) + red[1]) + ..., block_sum starts from red[0]: other
//    bits only for red[0] = -0.0f.  Its L1 sum adds absolute values, never -0.  Its SSIM sum can be -0, and the sign then
//    reaches loss_out only if every wave's total is -0.0f.
#pragma once
#include <hip/hip_runtime.h>
#include "wave_reduce.h"

namespace gsr {

// Sum over the 64 lanes of a wave, every lane gets it: the xor butterfly v += v[lane ^ off], off = 32, 16, 8, 4, 2, 1.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Sum over a workgroup of NWAVES full waves, every thread gets it: wave_sum, then the wave totals in wave order,
// ((red[0] + red[1]) + red[2]) + ...  `red`: NWAVES elements of LDS; the leading barrier lets back-to-back calls reuse it.
template <class T, int NWAVES = 4>
__device__ __forceinline__ T block_sum(T v, T* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = red[0];
#pragma unroll
    for (int w = 1; w < NWAVES; w++) r += red[w];
    return r;
}

// The serial-order final pass of ONE workgroup of 256 threads over n rows of N per-workgroup partials, in double.
// Thread t: s_t[a] = ((0 + row t) + row t+256) + ..., rows ascending; then per value a, by thread 0 alone,
// s[a] = ((0 + s_0[a]) + s_1[a]) + ... + s_255[a].  Only thread 0's s[] is the result.  red: N x 256 doubles of LDS.
template <int N, class Tin>
__device__ __forceinline__ void sum_partials(int n, const Tin* __restrict__ partial, double (*red)[256], double* s) {
#pragma unroll
    for (int a = 0; a < N; a++) s[a] = 0.0;
    for (int i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int a = 0; a < N; a++) s[a] += (double)partial[(size_t)i * N + a];
#pragma unroll
    for (int a = 0; a < N; a++) red[a][threadIdx.x] = s[a];
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int a = 0; a < N; a++) s[a] = 0.0;
    for (int i = 0; i < 256; i++)
#pragma unroll
        for (int a = 0; a < N; a++) s[a] += red[a][i];
}

// wave_inclusive_scan (wave_reduce.h) for 64-bit counts.  Integer sums are exact: no order to state.
__device__ __forceinline__ unsigned long long wave_inclusive_scan(unsigned long long x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    return x;
}

// The body of a ONE-workgroup, 1024-thread kernel: block_sum[0..nb) <- its exclusive prefix sums, in place, *total <- the
// sum of all.  Rounds of 1024 entries; the running carry crosses the rounds through LDS.  T: uint32_t or unsigned long long.
template <class T>
__device__ __forceinline__ void block_scan_carry(int nb, T* __restrict__ block_sum, T* __restrict__ total) {
    __shared__ T wave_sums[16];
    __shared__ T carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int i = b0 + tid;
        const T v = i < nb ? block_sum[i] : (T)0;
        const T x = wave_inclusive_scan(v, lane);
        if (lane == 63) wave_sums[wave] = x;
        __syncthreads();
        T woff = 0;
        for (int w = 0; w < wave; w++) woff += wave_sums[w];
        const T excl = carry_s + woff + x - v;
        if (i < nb) block_sum[i] = excl;
        __syncthreads();
        if (tid == 1023) carry_s = excl + v;
        __syncthreads();
    }
    if (tid == 0) *total = carry_s;
}

}  // namespace gsr
