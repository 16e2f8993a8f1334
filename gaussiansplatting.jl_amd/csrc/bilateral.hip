// Bilateral grid appearance correction (src/bilateral_grid.jl): the per-view slice of a (gx,gy,gz,12) grid of 3x4
// affine colour transforms, its pullback, the total-variation prior over all grids and the NU.Adam update of all
// grids with that prior fused in.  Compiled with -ffp-contract=off: the fused Adam tail must give the same bits as
// gsr_bilateral_tv + add + gsr_adam_step, and the region bounds of the pullback must be the same fp32 expression as
// the per-pixel coordinates.
//
// Layouts (column-major, as the reference): image / render (C,W,H); one view's grid (gx,gy,gz,12), x fastest,
// coefficient (d-1)*4 + c; all grids (gx,gy,gz,12,n).
//
// The pullback has no float atomics.  x = wi/(W-1)*(gx-1) is monotone in wi, so the pixels of one
// grid cell (same x0, y0) form a rectangle of the image, and they touch only 2x2 xy corners x gz levels x 12
// coefficients.  A workgroup takes a chunk of one cell's pixels, sums its contributions per level in registers,
// reduces them with fixed-order wave shuffles and a fixed-order cross-wave pass through LDS and stores one partial
// slab; a second kernel sums, per grid entry, the slabs of the <= 4 cells x chunks that touch it in a fixed order.
#include "gsr_kernels.h"
#include "adam_math.h"
#include "block_reduce.h"

#include <algorithm>

namespace {

constexpr float C2G_R = 0.299f, C2G_G = 0.587f, C2G_B = 0.114f;  // BGRID_C2G (bilateral_grid.jl:66)

// `Float32(wi - 1) / (w - 1) * (gx - 1)` (bilateral_grid.jl:133-134); ONE definition for the per-pixel coordinates and
// the cell bounds of the pullback
__device__ __forceinline__ float bg_coord(int i, int n, int g) {
    return n > 1 ? (float)i / (float)(n - 1) * (float)(g - 1) : 0.0f;
}

// first index i in [0, n] with floor(bg_coord(i)) >= cell (the coordinate is monotone in i)
__device__ __forceinline__ int bg_cell_start(int cell, int n, int g) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int)floorf(bg_coord(mid, n, g)) >= cell) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ float finite_or(float v, float alt) { return isfinite(v) ? v : alt; }

// _bgrid_coords (bilateral_grid.jl:122-150), 0-based
struct Coords {
    float s[3];
    float fx, fy, fz;
    int x0, x1, y0, y1, z0, z1;
    bool z_interior;
};
__device__ __forceinline__ Coords bg_coords(const float* __restrict__ px, int wi, int hi, int W, int H, int gx, int gy,
                                            int gz) {
    Coords c;
    c.s[0] = finite_or(px[0], 0.5f);
    c.s[1] = finite_or(px[1], 0.5f);
    c.s[2] = finite_or(px[2], 0.5f);
    const float x = bg_coord(wi, W, gx), y = bg_coord(hi, H, gy);
    const float g = fminf(fmaxf(C2G_R * c.s[0] + C2G_G * c.s[1] + C2G_B * c.s[2], 0.0f), 1.0f);
    const float z = g * (float)(gz - 1);
    c.x0 = (int)floorf(x);
    c.y0 = (int)floorf(y);
    c.z0 = min(max((int)floorf(z), 0), gz - 1);
    c.x1 = min(c.x0 + 1, gx - 1);
    c.y1 = min(c.y0 + 1, gy - 1);
    c.z1 = min(c.z0 + 1, gz - 1);
    c.fx = x - (float)c.x0;
    c.fy = y - (float)c.y0;
    c.fz = z - (float)c.z0;
    c.z_interior = (float)c.z0 != z && (float)c.z1 != z;  // no guidance gradient where z saturates or lands on a cell
    return c;
}

__device__ __forceinline__ size_t gidx(int x, int y, int z, int ci, int gx, int gy, int gz) {
    return (((size_t)ci * gz + z) * gy + y) * gx + x;
}

// ---- forward: one thread per pixel ----
__global__ __launch_bounds__(256) void slice_fwd_kernel(int W, int H, int C, const float* __restrict__ image,
                                                        const float* __restrict__ grid, int gx, int gy, int gz,
                                                        float* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= W * H) return;
    const int hi = p / W, wi = p - hi * W;
    const float* px = image + (size_t)p * C;
    const Coords c = bg_coords(px, wi, hi, W, H, gx, gy, gz);
    const float s4[4] = {c.s[0], c.s[1], c.s[2], 1.0f};
    float res[3];
#pragma unroll
    for (int di = 0; di < 3; di++) {
        float acc = 0.0f;
#pragma unroll
        for (int si = 0; si < 4; si++) {
            const int ci = di * 4 + si;
            const float c00 = grid[gidx(c.x0, c.y0, c.z0, ci, gx, gy, gz)] * (1.0f - c.fx) + grid[gidx(c.x1, c.y0, c.z0, ci, gx, gy, gz)] * c.fx;
            const float c10 = grid[gidx(c.x0, c.y1, c.z0, ci, gx, gy, gz)] * (1.0f - c.fx) + grid[gidx(c.x1, c.y1, c.z0, ci, gx, gy, gz)] * c.fx;
            const float c01 = grid[gidx(c.x0, c.y0, c.z1, ci, gx, gy, gz)] * (1.0f - c.fx) + grid[gidx(c.x1, c.y0, c.z1, ci, gx, gy, gz)] * c.fx;
            const float c11 = grid[gidx(c.x0, c.y1, c.z1, ci, gx, gy, gz)] * (1.0f - c.fx) + grid[gidx(c.x1, c.y1, c.z1, ci, gx, gy, gz)] * c.fx;
            const float v = (c00 * (1.0f - c.fy) + c10 * c.fy) * (1.0f - c.fz) + (c01 * (1.0f - c.fy) + c11 * c.fy) * c.fz;
            acc += v * s4[si];
        }
        res[di] = finite_or(acc, 0.5f);
    }
    float* o = out + (size_t)p * C;
    o[0] = res[0]; o[1] = res[1]; o[2] = res[2];
    for (int ch = 3; ch < C; ch++) o[ch] = px[ch];  // extra channels pass through (the loss head reads the layout)
}

// ---- pullback ----
constexpr int BWD_THREADS = 256, BWD_PPT = 4, BWD_BATCH = BWD_THREADS * BWD_PPT;
constexpr int NCOEF = 12, NSLOT = 4 * NCOEF;  // 2x2 xy corners x 12 coefficients per level

// 48 values per lane -> 3 per lane, summed over the wave, by recursive halving: at each step a lane keeps the half its
// lane bit selects and adds the partner's copy of it.  Fixed partners, fixed order: run-to-run bit-identical.  On exit
// lane l holds the wave sums of the values b5*24 + b4*12 + b3*6 + b2*3 + j (b_k = bit k of l), j = 0..2.
template <int HALF>
__device__ __forceinline__ void halve(float* v, int off, bool upper) {
#pragma unroll
    for (int i = 0; i < HALF; i++) {
        const float keep = upper ? v[i + HALF] : v[i];
        const float send = upper ? v[i] : v[i + HALF];
        v[i] = keep + __shfl_xor(send, off, 64);
    }
}
__device__ __forceinline__ void wave_reduce48(float* v, int lane) {
    halve<24>(v, 32, (lane >> 5) & 1);
    halve<12>(v, 16, (lane >> 4) & 1);
    halve<6>(v, 8, (lane >> 3) & 1);
    halve<3>(v, 4, (lane >> 2) & 1);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        v[j] += __shfl_xor(v[j], 2, 64);
        v[j] += __shfl_xor(v[j], 1, 64);
    }
}

// One workgroup per (cell, chunk): writes ∇image of its pixels and partial[wg][level][corner][coefficient].
// LDS: [gz][4 waves][48] running sums (each slot owned by one lane).
__global__ __launch_bounds__(BWD_THREADS) void slice_bwd_kernel(int W, int H, int C, const float* __restrict__ image,
                                                                const float* __restrict__ grid, int gx, int gy, int gz,
                                                                const float* vout, float* vimage, float* __restrict__ partial,
                                                                int nchunk) {
    extern __shared__ float lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int e = t; e < gz * 4 * NSLOT; e += BWD_THREADS) lds[e] = 0.0f;
    __syncthreads();

    const int wg = blockIdx.x, chunk = wg % nchunk, cell = wg / nchunk;
    const int cx = cell % gx, cy = cell / gx;
    const int col0 = bg_cell_start(cx, W, gx), col1 = bg_cell_start(cx + 1, W, gx);
    const int row0 = bg_cell_start(cy, H, gy), row1 = bg_cell_start(cy + 1, H, gy);
    const int nx = col1 - col0, npix = nx * (row1 - row0);
    const int per = (npix + nchunk - 1) / nchunk;
    const int q0 = min(npix, chunk * per), q1 = min(npix, q0 + per);
    const float dz = (float)(gz - 1);

    for (int b = q0; b < q1; b += BWD_BATCH) {
        float sv[BWD_PPT][3], dv[BWD_PPT][3], fxv[BWD_PPT], fyv[BWD_PPT], fzv[BWD_PPT];
        int z0v[BWD_PPT], z1v[BWD_PPT];
#pragma unroll
        for (int i = 0; i < BWD_PPT; i++) {
            const int q = b + i * BWD_THREADS + t;
            z0v[i] = -1; z1v[i] = -1;  // no level: a lane without a pixel contributes nothing
            sv[i][0] = sv[i][1] = sv[i][2] = 0.0f; dv[i][0] = dv[i][1] = dv[i][2] = 0.0f;
            fxv[i] = fyv[i] = fzv[i] = 0.0f;
            if (q >= q1) continue;
            const int r = q / nx, hi = row0 + r, wi = col0 + (q - r * nx);
            const size_t p = (size_t)hi * W + wi;
            const Coords c = bg_coords(image + p * C, wi, hi, W, H, gx, gy, gz);
            const float* vp = vout + p * C;
            const float d[3] = {finite_or(vp[0], 0.0f), finite_or(vp[1], 0.0f), finite_or(vp[2], 0.0f)};
            const float s4[4] = {c.s[0], c.s[1], c.s[2], 1.0f};
            // ∇image (bilateral_grid.jl:205-241)
            float gs[3] = {0.0f, 0.0f, 0.0f}, gzs = 0.0f;
#pragma unroll
            for (int corner = 0; corner < 8; corner++) {
                const int xc = corner & 1, yc = (corner >> 1) & 1, zc = (corner >> 2) & 1;
                const int xi = xc ? c.x1 : c.x0, yi = yc ? c.y1 : c.y0, zi = zc ? c.z1 : c.z0;
                const float wxy = (xc ? c.fx : 1.0f - c.fx) * (yc ? c.fy : 1.0f - c.fy);
                const float wt = wxy * (zc ? c.fz : 1.0f - c.fz);
                const float dwdz = wxy * (zc ? 1.0f : -1.0f) * dz;
#pragma unroll
                for (int di = 0; di < 3; di++) {
#pragma unroll
                    for (int si = 0; si < 4; si++) {
                        const float v = grid[gidx(xi, yi, zi, di * 4 + si, gx, gy, gz)];
                        const float gb = s4[si] * d[di];
                        if (si < 3) gs[si] += v * wt * d[di];
                        gzs += dwdz * v * gb;
                    }
                }
            }
            gzs = c.z_interior ? gzs : 0.0f;
            // every read of this pixel's cotangent is done: vimage may alias vout
            float* gp = vimage + p * C;
            gp[0] = gs[0] + C2G_R * gzs;
            gp[1] = gs[1] + C2G_G * gzs;
            gp[2] = gs[2] + C2G_B * gzs;
            if (gp != vp)
                for (int ch = 3; ch < C; ch++) gp[ch] = vp[ch];
#pragma unroll
            for (int k = 0; k < 3; k++) { sv[i][k] = c.s[k]; dv[i][k] = d[k]; }
            fxv[i] = c.fx; fyv[i] = c.fy; fzv[i] = c.fz; z0v[i] = c.z0; z1v[i] = c.z1;
        }
        // ∇grid: per level, the 2x2 xy corners x 12 coefficients of this thread's pixels, then over the workgroup
        for (int l = 0; l < gz; l++) {
            float acc[NSLOT];
#pragma unroll
            for (int e = 0; e < NSLOT; e++) acc[e] = 0.0f;
#pragma unroll
            for (int i = 0; i < BWD_PPT; i++) {
                if (z0v[i] != l && z1v[i] != l) continue;
                const float wl = (z0v[i] == l ? 1.0f - fzv[i] : 0.0f) + (z1v[i] == l ? fzv[i] : 0.0f);
                const float w[4] = {(1.0f - fxv[i]) * (1.0f - fyv[i]) * wl, fxv[i] * (1.0f - fyv[i]) * wl,
                                    (1.0f - fxv[i]) * fyv[i] * wl, fxv[i] * fyv[i] * wl};
                const float s4[4] = {sv[i][0], sv[i][1], sv[i][2], 1.0f};
#pragma unroll
                for (int di = 0; di < 3; di++)
#pragma unroll
                    for (int si = 0; si < 4; si++) {
                        const float a = s4[si] * dv[i][di];
#pragma unroll
                        for (int k = 0; k < 4; k++) acc[k * NCOEF + di * 4 + si] += w[k] * a;
                    }
            }
            wave_reduce48(acc, lane);
            if ((lane & 3) == 0) {
                const int base = ((lane >> 5) & 1) * 24 + ((lane >> 4) & 1) * 12 + ((lane >> 3) & 1) * 6 + ((lane >> 2) & 1) * 3;
                float* slot = lds + ((size_t)l * 4 + wave) * NSLOT + base;
#pragma unroll
                for (int j = 0; j < 3; j++) slot[j] += acc[j];
            }
        }
    }
    __syncthreads();
    float* out = partial + (size_t)wg * gz * NSLOT;
    for (int e = t; e < gz * NSLOT; e += BWD_THREADS) {
        const int l = e / NSLOT, k = e - l * NSLOT;
        const float* s = lds + (size_t)l * 4 * NSLOT + k;
        out[e] = ((s[0] + s[NSLOT]) + s[2 * NSLOT]) + s[3 * NSLOT];
    }
}

// ∇grid[x,y,z,ci] = the slabs of the cells (rx, ry) in {x-1, x} x {y-1, y} whose corner slot maps onto (x, y), chunk
// by chunk, in a fixed order.  One thread per grid entry; overwrites.
__global__ __launch_bounds__(256) void slice_bwd_sum_kernel(int gx, int gy, int gz, int nchunk,
                                                            const float* __restrict__ partial, float* __restrict__ vgrid) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int total = gx * gy * gz * NCOEF;
    if (e >= total) return;
    const int x = e % gx, y = (e / gx) % gy, z = (e / (gx * gy)) % gz, ci = e / (gx * gy * gz);
    float sum = 0.0f;
    for (int ry = max(y - 1, 0); ry <= y; ry++)
        for (int dy = 0; dy < 2; dy++) {
            if (min(ry + dy, gy - 1) != y) continue;
            for (int rx = max(x - 1, 0); rx <= x; rx++)
                for (int dx = 0; dx < 2; dx++) {
                    if (min(rx + dx, gx - 1) != x) continue;
                    const size_t cell = (size_t)ry * gx + rx;
                    const float* p = partial + (cell * nchunk * gz + z) * NSLOT + (dy * 2 + dx) * NCOEF + ci;
                    for (int j = 0; j < nchunk; j++) sum += p[(size_t)j * gz * NSLOT];
                }
        }
    vgrid[e] = sum;
}

// ---- total variation (bilateral_grid.jl:106-119) and the fused Adam tail ----
// One workgroup per (image, coefficient) slab of gx*gy*gz floats, staged in LDS: the TV gradient reads neighbours of
// the values BEFORE the update, so the Adam tail can update the slab in place.  partial[slab][3]: the slab's sums of
// squared forward differences along x, y, z.
template <bool ADAM>
__global__ __launch_bounds__(256) void tv_slab_kernel(int gx, int gy, int gz, float* grids, gsr::BilateralTv tv,
                                                      float* __restrict__ grad_out, float* __restrict__ mu,
                                                      float* __restrict__ nu, const float* __restrict__ vgrid, int view,
                                                      gsr::AdamHyper h, float* __restrict__ partial) {
    extern __shared__ float slab[];
    __shared__ float red[4];
    const int G = gx * gy * gz, t = threadIdx.x;
    const size_t sid = blockIdx.x;
    float* const base = grids + sid * G;
    for (int e = t; e < G; e += 256) slab[e] = base[e];
    __syncthreads();
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    const int gxy = gx * gy;
    const bool in_view = ADAM && (int)(sid / NCOEF) == view;
    for (int e = t; e < G; e += 256) {
        const int x = e % gx, y = (e / gx) % gy, z = e / gxy;
        const float c = slab[e];
        float tx = 0.0f, ty = 0.0f, tz = 0.0f;
        if (x > 0) tx += c - slab[e - 1];
        if (y > 0) ty += c - slab[e - gx];
        if (z > 0) tz += c - slab[e - gxy];
        if (x < gx - 1) { const float d = slab[e + 1] - c; sx += d * d; tx -= d; }
        if (y < gy - 1) { const float d = slab[e + gx] - c; sy += d * d; ty -= d; }
        if (z < gz - 1) { const float d = slab[e + gxy] - c; sz += d * d; tz -= d; }
        if (!ADAM && !grad_out) continue;
        const float g = tv.weight * ((tx * tv.rx + ty * tv.ry) + tz * tv.rz);
        if (!ADAM) {
            grad_out[sid * G + e] = g;
        } else {
            const float gg = in_view ? g + vgrid[(sid % NCOEF) * G + e] : g;
            const size_t k = sid * G + e;
            float m = mu[k], v = nu[k];
            base[e] = gsr::adam_update(c, gg, m, v, h);
            mu[k] = m; nu[k] = v;
        }
    }
    sx = gsr::block_sum(sx, red);
    sy = gsr::block_sum(sy, red);
    sz = gsr::block_sum(sz, red);
    if (t == 0) {
        partial[sid * 3 + 0] = sx;
        partial[sid * 3 + 1] = sy;
        partial[sid * 3 + 2] = sz;
    }
}

// the slabs' partial sums in a fixed order -> the TV loss
__global__ __launch_bounds__(256) void tv_final_kernel(int n_slabs, const float* __restrict__ partial,
                                                       gsr::BilateralTv tv, float* loss_out) {
    __shared__ float red[4];
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int i = threadIdx.x; i < n_slabs; i += 256)
#pragma unroll
        for (int a = 0; a < 3; a++) s[a] += partial[(size_t)i * 3 + a];
#pragma unroll
    for (int a = 0; a < 3; a++) s[a] = gsr::block_sum(s[a], red);
    if (threadIdx.x == 0) *loss_out = tv.weight * (((s[0] / tv.nx + s[1] / tv.ny) + s[2] / tv.nz) / tv.n12);
}

}  // namespace

int gsr_bilateral_chunks(int W, int H, int gx, int gy) {
    // upper bound of the pixels of one grid cell: the parallelism of the pullback, not its correctness
    const long long nx = gx > 1 ? std::min<long long>(W, (W - 1) / (gx - 1) + 2) : W;
    const long long ny = gy > 1 ? std::min<long long>(H, (H - 1) / (gy - 1) + 2) : H;
    const long long c = (nx * ny + BWD_BATCH - 1) / BWD_BATCH;
    return (int)std::max<long long>(1, c);
}

size_t gsr_bilateral_partial_bytes(int W, int H, int gx, int gy, int gz) {
    return (size_t)gx * gy * gsr_bilateral_chunks(W, H, gx, gy) * gz * NSLOT * sizeof(float);
}

void gsr_launch_bilateral_fwd(hipStream_t s, int W, int H, int C, const float* image, const float* grid, int gx, int gy,
                              int gz, float* out) {
    const long long P = (long long)W * H;
    hipLaunchKernelGGL(slice_fwd_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, W, H, C, image, grid, gx, gy,
                       gz, out);
}

void gsr_launch_bilateral_bwd(hipStream_t s, int W, int H, int C, const float* image, const float* grid, int gx, int gy,
                              int gz, const float* vout, float* vimage, float* vgrid, float* partial) {
    const int nchunk = gsr_bilateral_chunks(W, H, gx, gy);
    const unsigned wgs = (unsigned)((long long)gx * gy * nchunk);
    hipLaunchKernelGGL(slice_bwd_kernel, dim3(wgs), dim3(BWD_THREADS), (size_t)gz * 4 * NSLOT * sizeof(float), s, W, H,
                       C, image, grid, gx, gy, gz, vout, vimage, partial, nchunk);
    const int total = gx * gy * gz * NCOEF;
    hipLaunchKernelGGL(slice_bwd_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, gx, gy, gz, nchunk,
                       partial, vgrid);
}

void gsr_launch_bilateral_tv(hipStream_t s, int n, int gx, int gy, int gz, const float* grids, const gsr::BilateralTv& tv,
                             float* loss_out, float* grad_out, float* partial) {
    const int slabs = n * NCOEF;
    const size_t lds = (size_t)gx * gy * gz * sizeof(float);
    hipLaunchKernelGGL(tv_slab_kernel<false>, dim3((unsigned)slabs), dim3(256), lds, s, gx, gy, gz,
                       const_cast<float*>(grids), tv, grad_out, (float*)nullptr, (float*)nullptr, (const float*)nullptr, -1,
                       gsr::AdamHyper{}, partial);
    hipLaunchKernelGGL(tv_final_kernel, dim3(1), dim3(256), 0, s, slabs, partial, tv, loss_out);
}

void gsr_launch_bilateral_adam_tail(hipStream_t s, int n, int gx, int gy, int gz, float* grids, float* mu, float* nu,
                                    const float* vgrid, int view, const gsr::BilateralTv& tv, const gsr::AdamHyper& h,
                                    float* tv_loss_out, float* partial) {
    const int slabs = n * NCOEF;
    const size_t lds = (size_t)gx * gy * gz * sizeof(float);
    hipLaunchKernelGGL(tv_slab_kernel<true>, dim3((unsigned)slabs), dim3(256), lds, s, gx, gy, gz, grids, tv,
                       (float*)nullptr, mu, nu, vgrid, view, h, partial);
    hipLaunchKernelGGL(tv_final_kernel, dim3(1), dim3(256), 0, s, slabs, partial, tv, tv_loss_out);
}
