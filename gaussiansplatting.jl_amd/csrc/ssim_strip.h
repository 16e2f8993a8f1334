// The SSIM strip walk: what ssim.hip (the loss head and the generic entry points) and eval.hip (the evaluation head) share.
//
// Strips, not tiles: one wave owns 54 output columns (lane = column, 5 halo lanes on each side) and walks down a strip of
// rows + 5 above and below.  Per input row the horizontal 11x1 goes through a per-wave LDS row (one 8-byte write, ten 8-byte
// reads per lane, no workgroup barrier: the waves of a workgroup are independent); its results enter slot `row % 11` of a ring
// of the last 11 rows held in registers, and the vertical 1x11 of output row r is evaluated over the ring when row r + 5 has
// arrived.  The statistics travel as float2 pairs ((x, y), (x², y²)): packed fp32 instructions, two per issue slot.  Rows are
// requested from memory AHEAD rows before they are filtered.  Accumulation order follows the reference (symmetric pairs
// d = 1..5 with weight GAUSS[5-d], centre tap last, horizontally and vertically; zero padding outside the image).
// DESIGN.md §4, §4.2.
//
// What a kernel writes itself around these pieces: its fetch queue and the row loop, unrolled 11 times so that every ring
// index is static (a `break` in it defeats the unroll and sends the ring to scratch: guard the body instead).  The loads are
// straight-line, from a clamped address, the value untouched until its row is filtered (rows and columns outside the image
// become zeros then): a load under a branch, or a select right behind it, makes the wave wait for the row it has just
// requested, and the rows in flight are gone.
//
// Everything here is in an anonymous namespace: each translation unit gets its own GAUSS table.
#pragma once

#ifndef SSIM_EXACT
#define SSIM_EXACT 1  // every fp32 operation as written (ssim.hip's contracted build sets 0)
#endif

namespace {

constexpr int HALO = 5;
// The strip shape; the series that chose these values is in DESIGN.md §4.2 and profiles/ssim_strips/knobs.txt
constexpr int STRIP_W = 64 - 2 * HALO;  // 54 output columns per wave
constexpr int AHEAD = 3;                // rows requested from memory before the row being filtered
constexpr int RING = 2 * HALO + 1;      // 11 rows of horizontal results live in registers
constexpr int ROW_LDS = 64 + 2 * HALO;  // a wave's row buffer, padded so that the halo lanes read inside it

__constant__ float GAUSS[11] = {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f,
                                0.10936068743467331f,  0.21300552785396576f,   0.26601171493530273f,
                                0.21300552785396576f,  0.10936068743467331f,   0.036000773310661316f,
                                0.0075987582094967365f, 0.001028380123898387f};

typedef float v2f __attribute__((ext_vector_type(2)));  // two statistics per lane: the packed fp32 instructions of gfx950

// element at byte offset `lane_off` of the row that starts `row` elements into `plane`: a load is `scalar base + 32-bit lane
// offset` with no 64-bit lane arithmetic (offsets inside a plane are 32-bit: the entry points refuse images of 2^32 elements
// or more)
template <class T>
__device__ __forceinline__ T& at(T* plane, unsigned row, unsigned lane_off) {
    return *(T*)((char*)(plane + row) + lane_off);
}
template <class T>
__device__ __forceinline__ const T& at(const T* plane, unsigned row, unsigned lane_off) {
    return *(const T*)((const char*)(plane + row) + lane_off);
}

// A lane's column of the strip whose first output column is x0: `const Column col{x0, lane, W};`.  An aggregate, and
// SsimTerms below too: the member initialisers are evaluated in the kernel, where the object is declared, in this order —
// the same code as the statements written out there (a helper function is optimised on its own first, and the kernels'
// instruction order moves with it).
struct Column {
    int x0, lane, W;
    int gx = x0 - HALO + lane, cx = lane + HALO;            // image column, slot in the wave's LDS row
    bool col_in = gx >= 0 && gx < W;                        // the column is inside the image
    bool own = lane >= HALO && lane < 64 - HALO && gx < W;  // this lane's column is an output of this strip
    // gx clamped into the image: the column that is loaded
    __device__ __forceinline__ int gxc() const { return min(max(gx, 0), W - 1); }
};

// Zeros in the two ends of a wave's LDS row(s) that no lane writes (the halo lanes read them); the lanes below HALO call it:
// `if (lane < HALO) clear_halo(lane, buf);`.
template <class... T>
__device__ __forceinline__ void clear_halo(int lane, T*... buf) {
    ((buf[lane] = T{}), ...);
    ((buf[64 + HALO + lane] = T{}), ...);
}

// Orders a wave's own LDS writes before its other lanes' reads (and the reads before the next row's writes).  The LDS
// serves one wave's instructions in order, so this only has to hold the compiler: no instruction, no workgroup barrier.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a·b + c·d.  The contracted build fuses a·b into the add and rounds c·d, which is what the compiler has made of this
// expression in the default build since it exists; left to itself it picks the other product when the operands come out
// of float2 pairs, and the default build's results would move in the last bit (a training run then takes another path).
__device__ __forceinline__ float sum_of_products(float a, float b, float c, float d) {
#if SSIM_EXACT
    return a * b + c * d;
#else
    return __builtin_fmaf(a, b, c * d);
#endif
}

// 11x1 of one input row: the lane's (x, y) goes into slot cx of the wave's LDS row, the neighbours' come out of it.
// m = (Σx, Σy), q = (Σx², Σy²), c = Σxy.
__device__ __forceinline__ void horizontal_stats(v2f* buf, int cx, v2f XY, v2f& hm, v2f& hq, float& hc) {
    buf[cx] = XY;
    wave_sync();
    v2f m = 0, q = 0;
    float c = 0;
#pragma unroll
    for (int d = 1; d <= HALO; d++) {
        const float w = GAUSS[HALO - d];
        const v2f L = buf[cx - d], R = buf[cx + d];
        m += (L + R) * w;
        q += (L * L + R * R) * w;
        c += sum_of_products(L.x, L.y, R.x, R.y) * w;
    }
    wave_sync();
    const float wc = GAUSS[HALO];
    m += XY * wc; q += XY * XY * wc; c += XY.x * XY.y * wc;
    hm = m; hq = q; hc = c;
}

// 1x11 over the ring of horizontal results, input row in slot j just arrived: output row = slot j - 5, symmetric pairs
// d = 1..5, centre tap last (the reference's order, fused_ssim.jl:160-190: what keeps the exact build bit-identical to the
// oracle; scattering each new row into eleven pending outputs is another order).  j is static after the unroll.
template <class T>
__device__ __forceinline__ T ring_vertical(const T (&h)[RING], int j) {
    T a = 0;
#pragma unroll
    for (int d = 1; d <= HALO; d++) a += (h[(j + HALO + 1 + RING - d) % RING] + h[(j + HALO + 1 + d) % RING]) * GAUSS[HALO - d];
    a += h[(j + HALO + 1) % RING] * GAUSS[HALO];
    return a;
}

// The terms of SSIM = (Cv·Dv) / (A·Bv) from the filtered statistics of a pixel: the means of x, y, x², y² and xy
// (fused_ssim.jl:200-217): `const SsimTerms t{mu1, mu2, ex2, ey2, exy, C1, C2};`.  It takes scalars: where a kernel takes
// its float2 results apart (before or under the `own` branch) decides whether the compiler squares the means as a pair.
struct SsimTerms {
    float mu1, mu2, ex2, ey2, exy, C1, C2;
    float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2;
    float sigma1_sq = ex2 - mu1_sq, sigma2_sq = ey2 - mu2_sq, sigma12 = exy - mu1 * mu2;
    float A = mu1_sq + mu2_sq + C1, Bv = sigma1_sq + sigma2_sq + C2;
    float Cv = 2.0f * mu1 * mu2 + C1, Dv = 2.0f * sigma12 + C2;
};

}  // namespace
