// Transposed multi-value wave64 reduction for gfx950.
//
// Reduces N per-lane values (N <= 16) across the 64 lanes of a wave with ~3N/2 + 6 VALU
// ops instead of 6N: at every butterfly level two values are *paired* — one half of the
// lanes carries on with the first, the other half with the second — so the number of live
// registers halves per level.  Levels, in order:
//   bit 5  v_permlane32_swap (lanes 32-63 <-> 0-31)          2 ops / pair
//   bit 4  v_permlane16_swap (odd rows <-> even rows)         2 ops / pair
//   bit 3  DPP row_ror:8                                      2 v_cndmask + 1 v_add_dpp / pair
//   bit 0  DPP quad_perm [1,0,3,2]                            2 v_cndmask + 1 v_add_dpp / pair
//   bit 1  DPP quad_perm [2,3,0,1]   (plain add, 1 value left)
//   bit 2  DPP row_shr:4             (plain add; no xor-4 DPP exists, so only lanes with
//                                     bit 2 set end up with both halves)
// Afterwards every lane with (lane & 4) != 0 holds the complete 64-lane sum of one of the N
// inputs; which one is given by wave_reduce_index<N>(lane).  The caller stores with one
// ds_write per wave from the lanes wave_reduce_writer(lane) selects.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

// Inclusive prefix sum over the 64 lanes of a wave (six shuffle-up steps); lane 63 ends up with the wave's total.
// `lane` = threadIdx.x & 63.  Every lane of the wave has to call it.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    return x;
}

__device__ __forceinline__ float dpp_xor1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_xor2(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_ror8(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_shr4(float v) {  // lane i <- lane i-4 within the row, 0 for i < 4
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xF, 0xF, true));
}

// Integer max / sum over the 64 lanes of a wave, the result wave-uniform (in SGPRs): four DPP steps inside the rows of 16 —
// xor 1, xor 2, row_half_mirror, row_mirror: max and + are commutative, so a mirror pairs as well as an xor — with the
// identity 0 for the lanes a row shift leaves out (the compiler folds each into one v_max_u32_dpp / v_add_u32_dpp), then the
// four row totals through v_readlane and three scalar operations.  Integer results: no order to state.
#define GSR_DPP_U32(v, ctrl) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), 0xF, 0xF, true))
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = umax32(v, GSR_DPP_U32(v, 0xB1)); v = umax32(v, GSR_DPP_U32(v, 0x4E));
    v = umax32(v, GSR_DPP_U32(v, 0x141)); v = umax32(v, GSR_DPP_U32(v, 0x140));
    const uint32_t r0 = __builtin_amdgcn_readlane((int)v, 0), r1 = __builtin_amdgcn_readlane((int)v, 16);
    const uint32_t r2 = __builtin_amdgcn_readlane((int)v, 32), r3 = __builtin_amdgcn_readlane((int)v, 48);
    return umax32(umax32(r0, r1), umax32(r2, r3));
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += GSR_DPP_U32(v, 0xB1); v += GSR_DPP_U32(v, 0x4E);
    v += GSR_DPP_U32(v, 0x141); v += GSR_DPP_U32(v, 0x140);
    const uint32_t r0 = __builtin_amdgcn_readlane((int)v, 0), r1 = __builtin_amdgcn_readlane((int)v, 16);
    const uint32_t r2 = __builtin_amdgcn_readlane((int)v, 32), r3 = __builtin_amdgcn_readlane((int)v, 48);
    return (r0 + r1) + (r2 + r3);
}

// sum over the lane pair (i, i^32): lanes 0-31 get a's, lanes 32-63 get b's
__device__ __forceinline__ float pair_swap32(float a, float b) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// sum over (i, i^16): even rows get a's, odd rows get b's
__device__ __forceinline__ float pair_swap16(float a, float b) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

struct LaneBits {
    bool b0, b3, hi, odd_row;
    __device__ __forceinline__ explicit LaneBits(int lane)
        : b0(lane & 1), b3(lane & 8), hi(lane & 32), odd_row(lane & 16) {}
};

// One pairing level over n live values -> (n+1)/2 live values.  KIND: 0 swap32, 1 swap16, 2 ror8, 3 xor1.
template <int KIND>
__device__ __forceinline__ float pair_level(float a, float b, const LaneBits& L) {
    if (KIND == 0) return pair_swap32(a, b);
    if (KIND == 1) return pair_swap16(a, b);
    const bool bit = KIND == 2 ? L.b3 : L.b0;
    const float send = bit ? a : b, keep = bit ? b : a;
    return keep + (KIND == 2 ? dpp_ror8(send) : dpp_xor1(send));
}
template <int KIND>
__device__ __forceinline__ float single_level(float a, const LaneBits& L) {
    if (KIND == 0) return pair_swap32(a, a);
    if (KIND == 1) return pair_swap16(a, a);
    return a + (KIND == 2 ? dpp_ror8(a) : dpp_xor1(a));
}

template <int N, int KIND>
__device__ __forceinline__ void net_level(float (&v)[16], const LaneBits& L) {
    constexpr int H = N / 2;
#pragma unroll
    for (int p = 0; p < H; p++) v[p] = pair_level<KIND>(v[2 * p], v[2 * p + 1], L);
    if (N & 1) v[H] = single_level<KIND>(v[N - 1], L);
}

// In: v[0..N-1] per-lane partials.  Out: return value = the full wave sum of input
// number wave_reduce_index<N>(lane).
template <int N>
__device__ __forceinline__ float wave_reduce_transposed(float (&v)[16], const LaneBits& L) {
    static_assert(N >= 1 && N <= 16, "at most 16 values per network");
    constexpr int N1 = (N + 1) / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2;
    net_level<N, 0>(v, L);
    net_level<N1, 1>(v, L);
    net_level<N2, 2>(v, L);
    net_level<N3, 3>(v, L);
    float r = v[0];
    r = r + dpp_xor2(r);
    r = r + dpp_shr4(r);
    return r;
}

// Lanes whose result is complete and which are pairwise distinct per input (bit 1 clear, bit 2 set).
__device__ __forceinline__ bool wave_reduce_writer(int lane) { return (lane & 6) == 4; }

// ---- row-then-column reduction of the backward's partials (mode :rgb) ----
// The wave is 4 rows of 16 lanes; lanes l, l^16, l^32, l^48 sit in the same pixel COLUMN, and
// the three geometric moments the gradient row needs are P, dx*P, dx^2*P and U1, dx*U1 with dx a
// function of the column only.  So the six per-lane sums {P, U1, c0, c1, U2, c2} are first
// reduced over the 4 rows (two transposed swap levels: 5 swaps instead of 8 for nine values),
// each row of lanes then expands what it holds with its dx weights into at most 3 outputs, and
// the 16-lane tail of the network finishes.  Row r (= lane >> 4) ends up with:
//   r = 0: {P, dx*P, dx^2*P}   r = 1: {c0, U2, -}   r = 2: {U1, dx*U1, c2}   r = 3: {c1, -, -}
// Output j of a row lands on its lanes with (b3, b0) = (0,0): j = 0, (1,0): j = 1, (0,1): j = 2.
struct RowColConsts {  // loop-invariant per lane
    float e1, e3, k2, k4;  // o1 = b0*(dx*e1) + b1*k2;  o2 = b0*(dx*dx*e3) + b1*k4
    int slot;              // index into the 9-float accumulator row this lane's total goes to, or -1
    __device__ __forceinline__ explicit RowColConsts(int lane) {
        const int r = lane >> 4;
        e1 = (r == 0 || r == 2) ? 1.0f : 0.0f;
        e3 = r == 0 ? 1.0f : 0.0f;
        k2 = r == 1 ? 1.0f : 0.0f;
        k4 = r == 2 ? 1.0f : 0.0f;
        // accumulator row layout (composite.hip): [0..2] rgb, [3] P, [4] dx^2*P, [5] dx*U1, [6] U2, [7] dx*P, [8] U1
        const int j = (lane & 1) ? 2 : ((lane & 8) ? 1 : 0);
        const int table[4][3] = {{3, 7, 4}, {0, 6, -1}, {8, 5, 2}, {1, -1, -1}};
        int t = -1;
#pragma unroll
        for (int rr = 0; rr < 4; rr++)
#pragma unroll
            for (int jj = 0; jj < 3; jj++)
                if (rr == r && jj == j) t = table[rr][jj];
        const bool writer = (lane & 6) == 4 && !((lane & 1) && (lane & 8));  // (b3,b0) = (1,1) duplicates j = 2
        slot = writer ? t : -1;
    }
};

// The first level alone: pairs (P,U1), (c0,c1), (U2,c2) over lane^32.
struct RowColHalf { float a0, a1, a2; };
__device__ __forceinline__ RowColHalf wave_reduce_rowcol_rgb_half(float P, float U1, float U2, float c0, float c1, float c2) {
    return {pair_swap32(P, U1), pair_swap32(c0, c1), pair_swap32(U2, c2)};
}
// ... and the levels behind it.
__device__ __forceinline__ float wave_reduce_rowcol_rgb_rest(const RowColHalf& h, float dx, const LaneBits& L, const RowColConsts& K) {
    // pair + single over lane^16
    const float b0 = pair_swap16(h.a0, h.a1), b1 = pair_swap16(h.a2, h.a2);
    // column weights
    const float o0 = b0;
    const float o1 = b0 * (dx * K.e1) + b1 * K.k2;
    const float o2 = b0 * ((dx * dx) * K.e3) + b1 * K.k4;
    // 16 lanes of the row: pair (o0,o1) by b3, o2 alongside; then pair by b0; then the two plain levels
    const float x0 = pair_level<2>(o0, o1, L), x1 = single_level<2>(o2, L);
    float r = pair_level<3>(x0, x1, L);
    r = r + dpp_xor2(r);
    r = r + dpp_shr4(r);
    return r;
}
__device__ __forceinline__ float wave_reduce_rowcol_rgb(float P, float U1, float U2, float c0, float c1, float c2,
                                                        float dx, const LaneBits& L, const RowColConsts& K) {
    return wave_reduce_rowcol_rgb_rest(wave_reduce_rowcol_rgb_half(P, U1, U2, c0, c1, c2), dx, L, K);
}

// a * b rounded to fp32 whatever consumes it: the product carries no `contract` flag, so it cannot fuse into a following add
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// ---- two consecutive :rgb instances, A and B, in ONE network ----
// The unpaired network above carries one value where two fit (pair_swap16(a2, a2), single_level<2>(o2)) and runs its last two
// levels on one value.  Two instances fill those places.  Each does its first level by itself, when its sums are complete
// (wave_reduce_rowcol_rgb_half: A then waits for B in three registers, not six); behind it three swap16 (nine swaps for the
// pair, not ten), one set of dx weights, and a 16-lane tail over 5 -> 3 -> 2 -> 1 values.  Row r (= lane >> 4) ends up with
// (b0, b1, b2) and the outputs
//   r = 0: (P, c0, U2) of A -> {P, dx*P, dx^2*P, c0, U2}      r = 2: (U1, c1, c2) of A -> {U1, dx*U1, -, c1, c2}
//   r = 1: the same of B                                       r = 3: the same of B
// EVERY value passes the levels in the order it does above — swap32, swap16, weight, ror8, xor1, xor2, shr4 — and every level adds
// the same two operands; only which lanes carry which value differs.  The 18 sums are therefore the unpaired network's bit for
// bit (up to the sign of an exact zero: above, o1 and o2 also add the other value times a zero weight).
// A lane with bit 2 set holds, by (b1, b3, b0): (0,0,0) o0 = b0, (0,1,0) o1 = dx*b0, (0,0,1) o3 = b1, (0,1,1) o4 = b2, and
// (1,-,-) o2 = dx^2*b0, which rows 0 and 1 write from their lane (1,0,0).
struct RowColConstsPair {  // loop-invariant per lane
    bool b1;   // lane & 2: the xor2 level is a pair level here
    int slot;  // index into the 9-float accumulator row of instance (odd row ? B : A) this lane's total goes to, or -1
    __device__ __forceinline__ explicit RowColConstsPair(int lane) : b1(lane & 2) {
        const int r = lane >> 4;
        // accumulator row layout (composite.hip): [0..2] rgb, [3] P, [4] dx^2*P, [5] dx*U1, [6] U2, [7] dx*P, [8] U1
        const int j = (lane & 2) ? 2 : ((lane & 1) ? 3 : 0) + ((lane & 8) ? 1 : 0);  // which of o0..o4
        const int table[2][5] = {{3, 7, 4, 0, 6}, {8, 5, -1, 1, 2}};
        int t = -1;
#pragma unroll
        for (int hh = 0; hh < 2; hh++)
#pragma unroll
            for (int jj = 0; jj < 5; jj++)
                if (hh == (r >> 1) && jj == j) t = table[hh][jj];
        const bool writer = (lane & 4) && (!(lane & 2) || !(lane & 9));  // o2 sits on four lanes of a row: (b3, b0) = (0, 0) writes
        slot = writer ? t : -1;
    }
};

// In: the first level and dx of instance A and of instance B.  Out: the wave total that K.slot names, of A on the even lane
// rows and of B on the odd ones.
__device__ __forceinline__ float wave_reduce_rowcol_rgb_pair(const RowColHalf& A, float dxA, const RowColHalf& B, float dxB,
                                                             const LaneBits& L, const RowColConstsPair& K) {
    // even rows get A's, odd rows B's
    const float b0 = pair_swap16(A.a0, B.a0), b1 = pair_swap16(A.a1, B.a1), b2 = pair_swap16(A.a2, B.a2);
    // column weights, of the instance this row holds
    // (rounded products: left contractable, o2 fuses into the add of its ror8 level — above it is the result of an FMA with a
    //  zero addend, which cannot fuse again — and the moments differ from the unpaired network's in the last bit)
    const float dx = L.odd_row ? dxB : dxA;
    const float o1 = mul_rounded(b0, dx), o2 = mul_rounded(b0, mul_rounded(dx, dx));
    // 16 lanes of the row: 5 -> 3 by b3, 3 -> 2 by b0, 2 -> 1 by b1, then the plain level
    const float x0 = pair_level<2>(b0, o1, L), x1 = pair_level<2>(b1, b2, L), x2 = single_level<2>(o2, L);
    const float y0 = pair_level<3>(x0, x1, L), y1 = single_level<3>(x2, L);
    const float send = K.b1 ? y0 : y1, keep = K.b1 ? y1 : y0;
    float r = keep + dpp_xor2(send);
    r = r + dpp_shr4(r);
    return r;
}

// ---- the same for mode :rgbd (seven per-lane sums: P, U1, U2, r, g, b, depth -> ten outputs) ----
// swap32 pairs (P,r) (U1,g) (U2,b) (depth,depth), swap16 pairs (a0,a1) and (a3,a2): six swaps instead of the eight the
// generic ten-value network needs.  Row r (= lane >> 4) ends up with b0 / b1 =
//   r = 0: P / depth (unused)   r = 1: U1 / U2   r = 2: r / depth   r = 3: g / b
// and outputs  r = 0: {P, dx*P, dx^2*P}   r = 1: {U1, dx*U1, U2}   r = 2: {r, depth, -}   r = 3: {g, b, -}.
struct RowColConstsD {
    float e1, e3, k2, k4;
    int slot;
    __device__ __forceinline__ explicit RowColConstsD(int lane) {
        const int r = lane >> 4;
        e1 = r < 2 ? 1.0f : 0.0f;        // o1 = dx * b0 on rows 0, 1
        e3 = r == 0 ? 1.0f : 0.0f;       // o2 = dx^2 * b0 on row 0
        k2 = r >= 2 ? 1.0f : 0.0f;       // o1 = b1 on rows 2, 3
        k4 = r == 1 ? 1.0f : 0.0f;       // o2 = b1 on row 1
        // accumulator row layout (composite.hip, NA = 10): [0..2] rgb, [3] P, [4] dx^2*P, [5] dx*U1, [6] U2, [7] dx*P, [8] U1, [9] depth
        const int j = (lane & 1) ? 2 : ((lane & 8) ? 1 : 0);
        const int table[4][3] = {{3, 7, 4}, {8, 5, 6}, {0, 9, -1}, {1, 2, -1}};
        int t = -1;
#pragma unroll
        for (int rr = 0; rr < 4; rr++)
#pragma unroll
            for (int jj = 0; jj < 3; jj++)
                if (rr == r && jj == j) t = table[rr][jj];
        const bool writer = (lane & 6) == 4 && !((lane & 1) && (lane & 8));
        slot = writer ? t : -1;
    }
};

__device__ __forceinline__ float wave_reduce_rowcol_rgbd(float P, float U1, float U2, float c0, float c1, float c2, float c3,
                                                         float dx, const LaneBits& L, const RowColConstsD& K) {
    const float a0 = pair_swap32(P, c0), a1 = pair_swap32(U1, c1), a2 = pair_swap32(U2, c2), a3 = pair_swap32(c3, c3);
    const float b0 = pair_swap16(a0, a1), b1 = pair_swap16(a3, a2);
    const float o0 = b0;
    const float o1 = b0 * (dx * K.e1) + b1 * K.k2;
    const float o2 = b0 * ((dx * dx) * K.e3) + b1 * K.k4;
    const float x0 = pair_level<2>(o0, o1, L), x1 = single_level<2>(o2, L);
    float r = pair_level<3>(x0, x1, L);
    r = r + dpp_xor2(r);
    r = r + dpp_shr4(r);
    return r;
}

// Which input a lane ends up holding (the same network run on indices).
template <int N>
__device__ __forceinline__ void index_level(int (&idx)[16], bool bit) {
    constexpr int H = N / 2;
#pragma unroll
    for (int p = 0; p < H; p++) idx[p] = bit ? idx[2 * p + 1] : idx[2 * p];
    if (N & 1) idx[H] = idx[N - 1];
}
template <int N>
__device__ __forceinline__ int wave_reduce_index(int lane) {
    constexpr int N1 = (N + 1) / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2;
    int idx[16];
#pragma unroll
    for (int i = 0; i < 16; i++) idx[i] = i;
    index_level<N>(idx, (lane & 32) != 0);
    index_level<N1>(idx, (lane & 16) != 0);
    index_level<N2>(idx, (lane & 8) != 0);
    index_level<N3>(idx, (lane & 1) != 0);
    return idx[0];
}

}  // namespace gsr
