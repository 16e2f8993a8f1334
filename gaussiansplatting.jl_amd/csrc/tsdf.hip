// TSDF fusion of rendered depth frames and surface-nets mesh extraction: the step behind the geometry features (the :rgbd /
// :rgbdn frames, the depth and depth-normal losses, the sky dome, the 3-D filter) — one surface of the scene, made on the device.
// DESIGN.md §21.  Compiled with -ffp-contract=off: every fp32 expression below is one rounded operation per operator, in the
// association written, and the numpy restatement (tests/tsdf_ref.py) is held to the same bits.
//
// The volume: nx x ny x nz samples, sample (i, j, k) at world o + h*(i, j, k), linear index l = i + nx*(j + ny*k); per sample
// one float2 {tsdf, weight}, optionally 3 floats of colour.
//
//   integrate : one lane per sample, a workgroup is 256 consecutive x of ONE (j, k) row (blockIdx.y = j, blockIdx.z = k): a
//               wave's loads and stores are contiguous in x, py / pz and the camera are wave-uniform, no index is divided.
//                   p = o + h*(float)idx                       pc[r] = ((R[r]*px + R[r+3]*py) + R[r+6]*pz) + t[r] ;  z = pc[2]
//                   skip unless z > near
//                   u = (fx*pc[0])/z + cx ;  v = (fy*pc[1])/z + cy ;  fu = floorf(u + 0.5f), fv = floorf(v + 0.5f)
//                   skip unless 0 <= fu < W, 0 <= fv < H (in float), alpha >= min_alpha
//                   d = D/alpha ;  sdf = d - z ;  skip unless sdf >= -trunc ;  s = fminf(1, sdf/trunc)
//                   tsdf' = (tsdf*w + s)/(w + 1) ;  w' = w + 1 ;  colour' = (colour*w + clamp(rgb/alpha, 0, 1))/(w + 1)
//               Every comparison is written so that a NaN skips.  A skipped sample's volume entry is neither read nor written.
//
//   count     : one lane per sample column: a wave walks a RUN of `rows` whole x-rows of cells of one k in steps of 63 cells, in
//               ascending cell order (lane 63 only carries the next column over to lane 62), so a run is one contiguous range
//               of the cell order and the runs ascend with it.  A lane loads its column's four samples, contiguous in x across
//               the wave, and gets the other four corners of its cell from lane + 1.  Per cell one word: bit 27 active, bits
//               28..30 the quads of the edges p -> p + e_a (a = 0, 1, 2), bit 31 "p is inside", bits 0..23 the number of
//               active cells before it in its run (ballot and popcount: integers, exact).  Per run one 64-bit word
//               {active cells, quads << 32}.  No LDS, no barrier.
//   scan      : ONE workgroup: block_scan_carry (block_reduce.h) over the packed per-run words; the totals are the two counts.
//   emit      : the same walk over the cell words alone (the volume is read for the active cells only): vertex id = run
//               offset + rank, quad id = run offset + the quad bits before it in the run.  Rows at or past the capacities are
//               not written.
// Integer sums only; no atomics.  The output is the same bits in every run.
#include <algorithm>

#include "gsr_kernels.h"
#include "block_reduce.h"

namespace {

constexpr int TS_THREADS = 256;
constexpr int MESH_RUN_CELLS = 2048;         // cells a wave's run aims at (whole rows: at least one)
constexpr int MESH_STEP = 63;                // cells of one wave step
constexpr uint32_t MESH_RANK_MASK = 0xFFFFFFu;
constexpr uint32_t MESH_ACTIVE = 1u << 27;
constexpr int MESH_QUAD_SHIFT = 28;
constexpr uint32_t MESH_INSIDE = 1u << 31;

template <bool COLOR>
__global__ __launch_bounds__(TS_THREADS) void tsdf_integrate_kernel(GsrTsdfGrid g, GsrTsdfCam c, int W, int H, int C,
                                                                    const float* __restrict__ image, float min_alpha,
                                                                    float near_plane, float trunc, float2* __restrict__ vol,
                                                                    float* __restrict__ color) {
    const int i = blockIdx.x * TS_THREADS + threadIdx.x;
    if (i >= g.nx) return;
    const int j = blockIdx.y, k = blockIdx.z;   // wave-uniform
    const float px = g.o[0] + g.h * (float)i;
    const float py = g.o[1] + g.h * (float)j;
    const float pz = g.o[2] + g.h * (float)k;
    const float x = ((c.R[0] * px + c.R[3] * py) + c.R[6] * pz) + c.t[0];
    const float y = ((c.R[1] * px + c.R[4] * py) + c.R[7] * pz) + c.t[1];
    const float z = ((c.R[2] * px + c.R[5] * py) + c.R[8] * pz) + c.t[2];
    if (!(z > near_plane)) return;
    const float u = (c.fx * x) / z + c.cx;
    const float v = (c.fy * y) / z + c.cy;
    const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
    if (!(fu >= 0.0f && fu < (float)W && fv >= 0.0f && fv < (float)H)) return;
    const size_t pix = ((size_t)(int)fv * (size_t)W + (size_t)(int)fu) * (size_t)C;
    const float D = image[pix + 3], alpha = image[pix + 4];   // (one wait for the two)
    if (!(alpha >= min_alpha)) return;
    const float d = D / alpha;
    const float sdf = d - z;
    if (!(sdf >= -trunc)) return;
    const float s = fminf(1.0f, sdf / trunc);
    const size_t l = (size_t)i + (size_t)g.nx * ((size_t)j + (size_t)g.ny * (size_t)k);
    const float2 tw = vol[l];
    const float w1 = tw.y + 1.0f;
    vol[l] = make_float2((tw.x * tw.y + s) / w1, w1);
    if (COLOR) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float q = fminf(fmaxf(image[pix + ch] / alpha, 0.0f), 1.0f);
            color[3 * l + ch] = (color[3 * l + ch] * tw.y + q) / w1;
        }
    }
}

// How many of the lanes below this one are set in a ballot.
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The quad of the grid edge p -> p + e_A (p = cell (i, j, k), both ends observed and on different sides — the caller knows):
// the four cells around the edge exist (p_b >= 1, p_c >= 1; the upper bounds hold because p is a cell) and are active, i.e.
// the 2 x 3 x 3 samples they span are all observed (each of the four contains the sign-changing edge).
template <int A>
__device__ __forceinline__ bool mesh_quad_at(const GsrTsdfGrid& g, const float2* __restrict__ vol, int i, int j, int k) {
    constexpr int B = (A + 1) % 3, Cc = (A + 2) % 3;
    const int idx[3] = {i, j, k};
    const long long st[3] = {1, (long long)g.nx, (long long)g.nx * g.ny};
    if (idx[B] < 1 || idx[Cc] < 1) return false;
    const long long base = (long long)i + st[1] * j + st[2] * k;
    float wt[18];   // all 18 loads in flight at once: no short-circuit between them
#pragma unroll
    for (int da = 0; da < 2; da++)
#pragma unroll
        for (int db = -1; db <= 1; db++)
#pragma unroll
            for (int dc = -1; dc <= 1; dc++)
                wt[(da * 3 + db + 1) * 3 + dc + 1] = vol[base + da * st[A] + db * st[B] + dc * st[Cc]].y;
    bool all = true;
#pragma unroll
    for (int n = 0; n < 18; n++) all = all & (wt[n] > 0.0f);
    return all;
}

// The four samples of column (i, j..j+1, k..k+1), p -> sample (i, j, k): bit s = inside, bit 4 + s = observed, s = dy + 2 dz.
__device__ __forceinline__ uint32_t mesh_column_code(const float2* __restrict__ p, size_t sy, size_t sz) {
    const float2 t[4] = {p[0], p[sy], p[sz], p[sy + sz]};
    uint32_t code = 0;
#pragma unroll
    for (int s = 0; s < 4; s++) code |= ((t[s].x < 0.0f ? 1u : 0u) << s) | ((t[s].y > 0.0f ? 0x10u : 0u) << s);
    return code;
}

// The flag bits of cell (i, j, k) — MESH_ACTIVE, the three quad bits, MESH_INSIDE of its corner 0 — from the codes of its own
// column and of the next one.
__device__ __forceinline__ uint32_t mesh_cell_flags(const GsrTsdfGrid& g, const float2* __restrict__ vol, int i, int j, int k,
                                                    uint32_t code, uint32_t next) {
    const uint32_t in = (code & 0xFu) | ((next & 0xFu) << 4), obs = (code >> 4) | (next & 0xF0u);   // bit s + 4 dx
    uint32_t w = 0;
    if (obs == 0xFFu && in != 0u && in != 0xFFu) w |= MESH_ACTIVE;
    if (in & 1u) w |= MESH_INSIDE;
    if ((obs & 1u) && (obs & 16u) && ((in ^ (in >> 4)) & 1u) && mesh_quad_at<0>(g, vol, i, j, k)) w |= 1u << MESH_QUAD_SHIFT;
    if ((obs & 1u) && (obs & 2u) && ((in ^ (in >> 1)) & 1u) && mesh_quad_at<1>(g, vol, i, j, k)) w |= 2u << MESH_QUAD_SHIFT;
    if ((obs & 1u) && (obs & 4u) && ((in ^ (in >> 2)) & 1u) && mesh_quad_at<2>(g, vol, i, j, k)) w |= 4u << MESH_QUAD_SHIFT;
    return w;
}

// grid (runs of a slab / 4, nz - 1), one run per wave.  blk[run + nruns * k]: {active cells, quads << 32}.
__global__ __launch_bounds__(TS_THREADS) void mesh_count_kernel(GsrTsdfGrid g, int rows, int nruns, const float2* __restrict__ vol,
                                                                uint32_t* __restrict__ words,
                                                                unsigned long long* __restrict__ blk) {
    const int lane = threadIdx.x & 63;
    const int run = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (run >= nruns) return;   // (the whole wave: there is no barrier)
    const int ncx = g.nx - 1, ncy = g.ny - 1, k = blockIdx.y;
    const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * (size_t)g.ny;
    uint32_t carry_v = 0, carry_q = 0;
    for (int r = 0; r < rows; r++) {
        const int j = run * rows + r;
        if (j >= ncy) break;
        const size_t row = (size_t)ncx * ((size_t)j + (size_t)ncy * (size_t)k);
        const float2* __restrict__ vrow = vol + (sy * (size_t)j + sz * (size_t)k);
        for (int i0 = 0; i0 < ncx; i0 += MESH_STEP) {
            const int i = i0 + lane;
            const uint32_t code = i < g.nx ? mesh_column_code(vrow + i, sy, sz) : 0u;
            const uint32_t next = __shfl_down(code, 1);
            const bool cell = lane < MESH_STEP && i < ncx;
            const uint32_t w = cell ? mesh_cell_flags(g, vol, i, j, k, code, next) : 0u;
            const unsigned long long bv = __ballot((w & MESH_ACTIVE) != 0);
            if (cell) words[row + i] = w | ((carry_v + lanes_below(bv)) & MESH_RANK_MASK);
            carry_v += (uint32_t)__popcll(bv);
            carry_q += (uint32_t)(__popcll(__ballot((w >> MESH_QUAD_SHIFT) & 1u)) + __popcll(__ballot((w >> MESH_QUAD_SHIFT) & 2u)) +
                                  __popcll(__ballot((w >> MESH_QUAD_SHIFT) & 4u)));
        }
    }
    if (lane == 0) blk[(size_t)run + (size_t)nruns * blockIdx.y] = (unsigned long long)carry_v | ((unsigned long long)carry_q << 32);
}

// ONE workgroup of 1024: blk <- its exclusive prefix sums, total[0] <- the sum, counts <- {vertices, quads}.
__global__ __launch_bounds__(1024) void mesh_scan_kernel(int nb, unsigned long long* __restrict__ blk,
                                                         unsigned long long* __restrict__ total, uint32_t* __restrict__ counts) {
    gsr::block_scan_carry(nb, blk, total);
    if (threadIdx.x == 0) {   // (thread 0 wrote *total itself)
        const unsigned long long t = *total;
        counts[0] = (uint32_t)t;
        counts[1] = (uint32_t)(t >> 32);
    }
}

// The vertex id of cell (i, j, k), known to be active: its run's offset plus its rank.
__device__ __forceinline__ int mesh_vertex_id(const uint32_t* __restrict__ words, const unsigned long long* __restrict__ blk,
                                              int ncx, int ncy, int rows, int nruns, int i, int j, int k) {
    const uint32_t w = words[(size_t)i + (size_t)ncx * ((size_t)j + (size_t)ncy * (size_t)k)];
    return (int)((uint32_t)blk[(size_t)(j / rows) + (size_t)nruns * (size_t)k] + (w & MESH_RANK_MASK));
}

template <int A>
__device__ __forceinline__ void mesh_write_quad(const uint32_t* __restrict__ words, const unsigned long long* __restrict__ blk,
                                                int ncx, int ncy, int rows, int nruns, int i, int j, int k, bool inside,
                                                unsigned long long q, long long max_faces, int* __restrict__ faces) {
    constexpr int B = (A + 1) % 3, Cc = (A + 2) % 3;
    int v[4];
#pragma unroll
    for (int n = 0; n < 4; n++) {   // c0 = p - e_b - e_c, c1 = p - e_c, c2 = p, c3 = p - e_b
        int p[3] = {i, j, k};
        if (n == 0 || n == 3) p[B] -= 1;
        if (n == 0 || n == 1) p[Cc] -= 1;
        v[n] = mesh_vertex_id(words, blk, ncx, ncy, rows, nruns, p[0], p[1], p[2]);
    }
    const int a0 = inside ? v[0] : v[3], a1 = inside ? v[1] : v[2], a2 = inside ? v[2] : v[1], a3 = inside ? v[3] : v[0];
    const long long f = 2 * (long long)q;
    if (f < max_faces) {
        faces[3 * f] = a0; faces[3 * f + 1] = a1; faces[3 * f + 2] = a2;
    }
    if (f + 1 < max_faces) {
        faces[3 * f + 3] = a0; faces[3 * f + 4] = a2; faces[3 * f + 5] = a3;
    }
}

// The vertex of the active cell (i, j, k): the mean of the crossing points of its sign-changing edges — the 4 x-edges, then
// y, then z; within an axis the two fixed coordinates count up, the lower axis fastest — and the mean of the 8 corners' colours
// in corner order (corner c = dx + 2 dy + 4 dz).
template <bool COLOR>
__device__ __forceinline__ void mesh_write_vertex(const GsrTsdfGrid& g, const float2* __restrict__ vol,
                                                  const float* __restrict__ color, int i, int j, int k, size_t vid,
                                                  float* __restrict__ vertices, float* __restrict__ vcolors) {
    const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * (size_t)g.ny;
    const size_t base = (size_t)i + sy * (size_t)j + sz * (size_t)k;
    float T[8];
#pragma unroll
    for (int c = 0; c < 8; c++) T[c] = vol[base + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz].x;
    float s[3] = {0.0f, 0.0f, 0.0f};
    int n = 0;
#pragma unroll
    for (int axis = 0; axis < 3; axis++) {
        const int step = 1 << axis;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            // the e-th corner with a zero coordinate along `axis`, the other two counting up
            const int lo = e & 1, hi = e >> 1;
            const int ca = axis == 0 ? 2 * lo + 4 * hi : axis == 1 ? lo + 4 * hi : lo + 2 * hi;
            const float Ta = T[ca], Tb = T[ca + step];
            if ((Ta < 0.0f) != (Tb < 0.0f)) {
                const float t = Ta / (Ta - Tb);
#pragma unroll
                for (int d = 0; d < 3; d++) s[d] = s[d] + (d == axis ? t : (float)((ca >> d) & 1));
                n++;
            }
        }
    }
    const float fn = (float)n;
    const int idx[3] = {i, j, k};
#pragma unroll
    for (int d = 0; d < 3; d++) vertices[3 * vid + d] = g.o[d] + g.h * ((float)idx[d] + s[d] / fn);
    if (COLOR) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            float a = color[3 * base + ch];
#pragma unroll
            for (int c = 1; c < 8; c++) a = a + color[3 * (base + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz) + ch];
            vcolors[3 * vid + ch] = a * 0.125f;
        }
    }
}

// The walk of mesh_count_kernel over the cell words; blk holds the exclusive run offsets now.
template <bool COLOR>
__global__ __launch_bounds__(TS_THREADS) void mesh_emit_kernel(GsrTsdfGrid g, int rows, int nruns, const float2* __restrict__ vol,
                                                               const float* __restrict__ color,
                                                               const uint32_t* __restrict__ words,
                                                               const unsigned long long* __restrict__ blk, long long max_vertices,
                                                               long long max_faces, float* __restrict__ vertices,
                                                               float* __restrict__ vcolors, int* __restrict__ faces) {
    const int lane = threadIdx.x & 63;
    const int run = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (run >= nruns) return;
    const int ncx = g.nx - 1, ncy = g.ny - 1, k = blockIdx.y;
    const unsigned long long off = blk[(size_t)run + (size_t)nruns * blockIdx.y];
    const uint32_t v_off = (uint32_t)off;
    unsigned long long q_carry = off >> 32;
    for (int r = 0; r < rows; r++) {
        const int j = run * rows + r;
        if (j >= ncy) break;
        const size_t row = (size_t)ncx * ((size_t)j + (size_t)ncy * (size_t)k);
        for (int i0 = 0; i0 < ncx; i0 += MESH_STEP) {
            const int i = i0 + lane;
            const uint32_t w = (lane < MESH_STEP && i < ncx) ? words[row + i] : 0u;
            const uint32_t qm = (w >> MESH_QUAD_SHIFT) & 7u;
            const unsigned long long b0 = __ballot(qm & 1u), b1 = __ballot(qm & 2u), b2 = __ballot(qm & 4u);
            unsigned long long q = q_carry + lanes_below(b0) + lanes_below(b1) + lanes_below(b2);
            q_carry += (unsigned long long)(__popcll(b0) + __popcll(b1) + __popcll(b2));
            if (w & MESH_ACTIVE) {
                const size_t vid = (size_t)v_off + (w & MESH_RANK_MASK);
                if ((long long)vid < max_vertices) mesh_write_vertex<COLOR>(g, vol, color, i, j, k, vid, vertices, vcolors);
            }
            const bool inside = (w & MESH_INSIDE) != 0;
            if (qm & 1u) mesh_write_quad<0>(words, blk, ncx, ncy, rows, nruns, i, j, k, inside, q++, max_faces, faces);
            if (qm & 2u) mesh_write_quad<1>(words, blk, ncx, ncy, rows, nruns, i, j, k, inside, q++, max_faces, faces);
            if (qm & 4u) mesh_write_quad<2>(words, blk, ncx, ncy, rows, nruns, i, j, k, inside, q++, max_faces, faces);
        }
    }
}

// rows of cells per run, runs per slab k, runs in all
struct MeshPlan {
    long long ncells;
    int rows, nruns, nblk;
};
inline MeshPlan mesh_plan(int nx, int ny, int nz) {
    MeshPlan p = {0, 1, 0, 0};
    if (nx < 2 || ny < 2 || nz < 2) return p;
    p.ncells = (long long)(nx - 1) * (ny - 1) * (nz - 1);
    p.rows = std::max(1, MESH_RUN_CELLS / (nx - 1));
    p.nruns = (ny - 1 + p.rows - 1) / p.rows;
    p.nblk = p.nruns * (nz - 1);
    return p;
}

}  // namespace

// scratch (8-byte aligned): the per-run words (8 bytes each), the total (8 bytes), one 4-byte word per cell
size_t gsr_mesh_scratch_size(int nx, int ny, int nz) {
    const MeshPlan p = mesh_plan(nx, ny, nz);
    if (p.ncells == 0) return 0;
    return ((size_t)p.nblk + 1) * 8 + (size_t)p.ncells * 4;
}

void gsr_launch_tsdf_integrate(hipStream_t s, const GsrTsdfGrid& g, const GsrTsdfCam& c, int W, int H, int C, const float* image,
                               float min_alpha, float near_plane, float trunc, float* volume, float* color) {
    const dim3 grid((unsigned)((g.nx + TS_THREADS - 1) / TS_THREADS), (unsigned)g.ny, (unsigned)g.nz);
    float2* vol = reinterpret_cast<float2*>(volume);
    if (color)
        hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, dim3(TS_THREADS), 0, s, g, c, W, H, C, image, min_alpha, near_plane,
                           trunc, vol, color);
    else
        hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, dim3(TS_THREADS), 0, s, g, c, W, H, C, image, min_alpha, near_plane,
                           trunc, vol, color);
}

void gsr_launch_mesh_count(hipStream_t s, const GsrTsdfGrid& g, const float* volume, uint32_t* counts, void* scratch) {
    const MeshPlan p = mesh_plan(g.nx, g.ny, g.nz);
    if (p.ncells == 0) {
        (void)hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), s);
        return;
    }
    unsigned long long* blk = reinterpret_cast<unsigned long long*>(scratch);
    uint32_t* words = reinterpret_cast<uint32_t*>(blk + p.nblk + 1);
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)((p.nruns + 3) / 4), (unsigned)(g.nz - 1)), dim3(TS_THREADS), 0, s, g,
                       p.rows, p.nruns, reinterpret_cast<const float2*>(volume), words, blk);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(1024), 0, s, p.nblk, blk, blk + p.nblk, counts);
}

void gsr_launch_mesh_emit(hipStream_t s, const GsrTsdfGrid& g, const float* volume, const float* color, const void* scratch,
                          long long max_vertices, long long max_faces, float* vertices, float* vertex_colors, int32_t* faces) {
    const MeshPlan p = mesh_plan(g.nx, g.ny, g.nz);
    if (p.ncells == 0) return;
    const unsigned long long* blk = reinterpret_cast<const unsigned long long*>(scratch);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(blk + p.nblk + 1);
    const dim3 grid((unsigned)((p.nruns + 3) / 4), (unsigned)(g.nz - 1));
    const float2* vol = reinterpret_cast<const float2*>(volume);
    if (color && vertex_colors)
        hipLaunchKernelGGL(mesh_emit_kernel<true>, grid, dim3(TS_THREADS), 0, s, g, p.rows, p.nruns, vol, color, words, blk, max_vertices,
                           max_faces, vertices, vertex_colors, faces);
    else
        hipLaunchKernelGGL(mesh_emit_kernel<false>, grid, dim3(TS_THREADS), 0, s, g, p.rows, p.nruns, vol, color, words, blk, max_vertices,
                           max_faces, vertices, vertex_colors, faces);
}
