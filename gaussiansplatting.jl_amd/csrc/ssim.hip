// Fused SSIM forward / backward and the photometric loss head.
// Reference behaviour: src/fused_ssim.jl:34-371 (kernels), :373-424 (host wrappers),
// src/training.jl:656,684-694 (L = (1-λ)·L1 + λ·(1 - mean SSIM)); SURVEY.md A.12.
//
// The kernels walk strips (ssim_strip.h: a wave owns 54 output columns and walks down a strip of rows through a per-wave LDS
// row and a ring of 11 rows in registers; the evaluation head, eval.hip, walks the same way).  One channel plane per wave:
// grid.z enumerates (channel, batch) planes for the generic entry points, the loss head puts the three channel waves of a
// strip into one workgroup (they read the same lines of the channel-interleaved image).  The strip height is chosen per
// launch (ssim_strip_h).  DESIGN.md §4, §4.2.
//
// This file is compiled TWICE into the library (csrc/Makefile):
//   SSIM_EXACT = 1, -ffp-contract=off: every fp32 operation as written, IEEE divisions — the maps are
//       bit-reproducible against the CPU oracle (the oracle's twin; gsr_ssim_precision(1) selects it);
//   SSIM_EXACT = 0 (the default path), -ffp-contract=fast: the same expressions with the multiply-adds fused
//       and the six divisions of the SSIM formula replaced by two hardware reciprocals — what any GPU compiler
//       makes of the reference's source ("contraction order unspecified, LLVM may fuse FMAs");
//       parity at the stated fp32 tolerance instead of bit for bit; −46 % VALU instructions per pixel.
#include "gsr_kernels.h"
#include "block_reduce.h"
#include "ssim_strip.h"

#if SSIM_EXACT
#define SSIM_NAME(x) x##_exact
#else
#define SSIM_NAME(x) x##_fast
#endif

namespace {

constexpr int MIN_WAVES = 4;    // waves per SIMD the register allocation has to leave room for
constexpr int LOSS_STRIPS = 1;  // loss head: strips per workgroup (x 3 channel waves); planar entry points: 4 waves

// A source hands out a plane (64-bit, once per wave), a row's offset inside it (wave-uniform: scalar arithmetic) and a lane's
// byte offset inside the row, for at().
// (W,H,CH,B) planar arrays, x fastest (fused_ssim.jl:27-31)
struct PlanarSrc {
    const float* img;
    const float* ref;
    int W, H;
    __device__ __forceinline__ const float* xplane(int plane) const { return img + (size_t)W * H * plane; }
    __device__ __forceinline__ const float* yplane(int plane) const { return ref + (size_t)W * H * plane; }
    __device__ __forceinline__ unsigned xrow(int gy) const { return (unsigned)W * (unsigned)gy; }
    __device__ __forceinline__ unsigned xlane(int gx) const { return 4u * (unsigned)gx; }
};
// rasterizer output (C,W,H) channel-fastest vs target (W,H,3): folds
// `features[1:3,:,:]` + `permutedims` (training.jl:656,684-685) into the loads
struct RasterSrc {
    const float* image;
    const float* target;
    int W, H, C;
    __device__ __forceinline__ const float* xplane(int plane) const { return image + plane; }
    __device__ __forceinline__ const float* yplane(int plane) const { return target + (size_t)W * H * plane; }
    __device__ __forceinline__ unsigned xrow(int gy) const { return (unsigned)(C * W) * (unsigned)gy; }
    __device__ __forceinline__ unsigned xlane(int gx) const { return 4u * (unsigned)(C * gx); }
};

// A wave's strip.  Workgroups are dealt round-robin to the 8 XCDs (one L2 each).  Neighbouring strips share 10 of 64
// columns and 10 input rows, so XCD x gets the x-th contiguous eighth of the strip groups (raster order) instead of every
// 8th group.  Grid: (8 * ceil(groups / 8), 1, planes) with groups = ceil(strips / SPB); a workgroup is NPL * SPB independent
// waves (NPL channel planes of SPB strips: nothing to synchronise between them).
struct Strip {
    int x0, y0, rows;  // first output column, first output row, output rows (< strip_h in the last strip row)
};
template <int NPL, int SPB>
__device__ __forceinline__ bool strip_of_wave(int W, int H, int strip_h, int wv, Strip& st) {
    const int nsx = (W + STRIP_W - 1) / STRIP_W, nsy = (H + strip_h - 1) / strip_h;
    const int n = nsx * nsy, groups = (n + SPB - 1) / SPB, per = (groups + 7) / 8;
    const int g = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    const int s = g * SPB + wv / NPL;
    if ((int)(blockIdx.x >> 3) >= per || g >= groups || s >= n) return false;
    st.x0 = (s % nsx) * STRIP_W;
    st.y0 = (s / nsx) * strip_h;
    st.rows = min(strip_h, H - st.y0);
    return true;
}

// fused_ssim.jl:34-238.  LOSS: additionally reduce Σ|x-y| and Σssim into one partial pair per wave.
template <class Src, bool LOSS, int NPL, int SPB>
__global__ __launch_bounds__(64 * NPL * SPB, MIN_WAVES) void ssim_fwd_kernel(Src src, int W, int H, int strip_h, float C1, float C2, int train,
                                                                 float* __restrict__ ssim_map, float* __restrict__ d0,
                                                                 float* __restrict__ d1, float* __restrict__ d2,
                                                                 float* __restrict__ partial) {
    constexpr int NW = NPL * SPB;
    __shared__ v2f rowbuf[NW][ROW_LDS];  // (x, y) of the wave's current row
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    Strip st;
    if (!strip_of_wave<NPL, SPB>(W, H, strip_h, wv, st)) {  // padding wave of the XCD-aware grid: contributes a zero pair
        if (LOSS && lane == 0) { partial[2 * ((size_t)blockIdx.x * NW + wv)] = 0.0f; partial[2 * ((size_t)blockIdx.x * NW + wv) + 1] = 0.0f; }
        return;
    }
    const int plane = blockIdx.z * NPL + wv % NPL;
    v2f* buf = rowbuf[wv];
    if (lane < HALO) clear_halo(lane, buf);
    const Column col{st.x0, lane, W};
    const int nrows = st.rows + 2 * HALO;  // input rows: rr = 0 is image row y0 - 5
    const unsigned xo = src.xlane(col.gxc()), yo = 4u * (unsigned)col.gxc();
    const float* xp = src.xplane(plane);
    const float* yp = src.yplane(plane);
    const size_t po = (size_t)W * H * plane;  // this wave's plane of the planar outputs
    auto fetch = [&](int rr) {  // straight-line, from a clamped address, untouched until the row is filtered (ssim_strip.h)
        const int gyc = min(max(st.y0 - HALO + rr, 0), H - 1);
        return v2f{at(xp, src.xrow(gyc), xo), at(yp, (unsigned)W * (unsigned)gyc, yo)};
    };
    v2f nxt[AHEAD];  // rows in flight: a wave that waits for each row's load lives in memory latency
#pragma unroll
    for (int i = 0; i < AHEAD; i++) nxt[i] = fetch(i);
    v2f hm[RING], hq[RING];  // horizontal results of the last 11 rows: (Σx, Σy), (Σx², Σy²)
    float hc[RING];          // ... Σxy
    float l1 = 0.0f, sv = 0.0f;
    for (int base = 0; base < nrows; base += RING) {
#pragma unroll
        for (int j = 0; j < RING; j++) {
            const int rr = base + j;
            if (rr < nrows) {
                const int gy = st.y0 - HALO + rr;
                const v2f XY = col.col_in && gy >= 0 && gy < H ? nxt[0] : v2f{0.0f, 0.0f};  // outside the image: zeros
#pragma unroll
                for (int i = 0; i + 1 < AHEAD; i++) nxt[i] = nxt[i + 1];
                nxt[AHEAD - 1] = fetch(rr + AHEAD);
                horizontal_stats(buf, col.cx, XY, hm[j], hq[j], hc[j]);
                if (LOSS && col.own && rr >= HALO && rr < nrows - HALO) l1 += fabsf(XY.x - XY.y);
                if (rr >= 2 * HALO) {  // output row rr - 10 of the strip is complete
                    const v2f om = ring_vertical(hm, j), oq = ring_vertical(hq, j);
                    const float o[5] = {om.x, om.y, oq.x, oq.y, ring_vertical(hc, j)};  // scalars before the branch
                    if (col.own) {
                        const int py = st.y0 + rr - 2 * HALO;
                        const SsimTerms t{o[0], o[1], o[2], o[3], o[4], C1, C2};
                        const float mu1 = t.mu1, mu2 = t.mu2, A = t.A, Bv = t.Bv, Cv = t.Cv, Dv = t.Dv;
                        const unsigned orow = (unsigned)W * (unsigned)py;
#if SSIM_EXACT
                        const float val = (Cv * Dv) / (A * Bv);
                        if (!LOSS) at(ssim_map + po, orow, yo) = val;
                        if (train) {
                            at(d0 + po, orow, yo) = ((mu2 * 2.0f * Dv) / (A * Bv) - (mu2 * 2.0f * Cv) / (A * Bv) -
                                      (mu1 * 2.0f * Cv * Dv) / (A * A * Bv) + (mu1 * 2.0f * Cv * Dv) / (A * Bv * Bv));
                            at(d1 + po, orow, yo) = (-Cv * Dv) / (A * Bv * Bv);
                            at(d2 + po, orow, yo) = (2.0f * Cv) / (A * Bv);
                        }
#else
                        // the same four quotients (fused_ssim.jl:219-233) over two reciprocals: 1/(AB) = rA·rB, 1/(A²B) = rA·rAB, 1/(AB²) = rB·rAB
                        const float rA = __builtin_amdgcn_rcpf(A), rB = __builtin_amdgcn_rcpf(Bv), rAB = rA * rB;
                        const float val = (Cv * Dv) * rAB;
                        if (!LOSS) at(ssim_map + po, orow, yo) = val;
                        if (train) {
                            at(d0 + po, orow, yo) = 2.0f * (mu2 * (Dv - Cv) * rAB + mu1 * val * (rB - rA));
                            at(d1 + po, orow, yo) = -val * rB;
                            at(d2 + po, orow, yo) = 2.0f * Cv * rAB;
                        }
#endif
                        if (LOSS) sv += val;
                    }
                }
            }
        }
    }
    if (LOSS) {
        // one partial pair per wave; thousands of waves hammering two words with atomics
        // serialise at ~12 ns each (MI355X_MICROARCH.md "fanin")
        const float a = gsr::wave_sum(l1), b = gsr::wave_sum(sv);
        if (lane == 0) {
            const size_t pair = (size_t)blockIdx.x * NW + wv;
            partial[2 * pair] = a;
            partial[2 * pair + 1] = b;
        }
    }
}

// The scalar loss (training.jl:656,684-694) from the per-wave partial sums the forward kernel left: the work of
// ONE workgroup, done by an extra workgroup of the backward launch (a launch of its own was 4 us during which the
// whole GPU waited).  Fixed summation order: bit-reproducible.
template <int NT>
__device__ __forceinline__ void loss_finish_body(const float* __restrict__ partial, int n_pairs, float lambda,
                                                 float inv_count, float* __restrict__ loss_out) {
    __shared__ float red[NT / 64];
    float a = 0.0f, b = 0.0f;
    for (int i = threadIdx.x; i < n_pairs; i += NT) {
        const float2 p = reinterpret_cast<const float2*>(partial)[i];
        a += p.x; b += p.y;
    }
    a = gsr::block_sum<float, NT / 64>(a, red);
    b = gsr::block_sum<float, NT / 64>(b, red);
    if (threadIdx.x == 0) {
        const float l1 = a * inv_count;
        const float s = 1.0f - b * inv_count;
        loss_out[0] = (1.0f - lambda) * l1 + lambda * s;
    }
}

// fused_ssim.jl:241-371.  LOSS: dL_dmap is the constant -λ/(3P) (pullback of
// λ·(1-mean(map))), the L1 pullback is added, output goes to the (C,W,H) rasterizer layout.
// Same strip walk as the forward with three maps instead of five statistics.
template <class Src, bool LOSS, int NPL, int SPB>
__global__ __launch_bounds__(64 * NPL * SPB, MIN_WAVES) void ssim_bwd_kernel(Src src, int W, int H, int strip_h, const float* __restrict__ dL_dmap,
                                                                 float chain_const, float l1_scale,
                                                                 const float* __restrict__ d0, const float* __restrict__ d1,
                                                                 const float* __restrict__ d2, float* __restrict__ out,
                                                                 int outC, const float* __restrict__ partial, int n_partial,
                                                                 float lambda, float inv_count, float* __restrict__ loss_out) {
    constexpr int NW = NPL * SPB;
    __shared__ v2f rowbuf01[NW][ROW_LDS];  // chained (d0, d1) of the wave's current row
    __shared__ float rowbuf2[NW][ROW_LDS];  // ... d2
    if (LOSS && blockIdx.x == gridDim.x - 1) {  // the extra workgroup of the loss head's launch
        loss_finish_body<64 * NW>(partial, n_partial, lambda, inv_count, loss_out);
        return;
    }
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    Strip st;
    if (!strip_of_wave<NPL, SPB>(W, H, strip_h, wv, st)) return;
    const int ch = wv % NPL, plane = blockIdx.z * NPL + ch;
    const size_t P = (size_t)W * H;
    v2f* b01 = rowbuf01[wv];
    float* b2 = rowbuf2[wv];
    if (lane < HALO) clear_halo(lane, b01, b2);
    const Column col{st.x0, lane, W};
    const int cx = col.cx, nrows = st.rows + 2 * HALO;
    const unsigned xo = src.xlane(col.gxc()), yo = 4u * (unsigned)col.gxc();
    const float* xp = src.xplane(plane);
    const float* yp = src.yplane(plane);
    const size_t po = P * plane;  // this wave's plane of the planar maps
    struct Row { v2f a01; float a2, chain, p1, p2; };  // derivative maps, dL/dmap of input row rr; x, y of the output row rr - 10
    auto fetch = [&](int rr) {  // straight-line loads from clamped addresses, values untouched until consumed, as in the forward
        const int gy = st.y0 - HALO + rr;
        const int gyc = min(max(gy, 0), H - 1), gyo = min(max(gy - HALO, 0), H - 1);
        const unsigned ro = (unsigned)W * (unsigned)gyc;
        Row r;
        r.a01 = v2f{at(d0 + po, ro, yo), at(d1 + po, ro, yo)};
        r.a2 = at(d2 + po, ro, yo);
        r.chain = LOSS ? chain_const : at(dL_dmap + po, ro, yo);
        r.p1 = at(xp, src.xrow(gyo), xo);
        r.p2 = at(yp, (unsigned)W * (unsigned)gyo, yo);
        return r;
    };
    Row nr[AHEAD];
#pragma unroll
    for (int i = 0; i < AHEAD; i++) nr[i] = fetch(i);
    v2f h01[RING];
    float h2[RING];
    for (int base = 0; base < nrows; base += RING) {
#pragma unroll
        for (int j = 0; j < RING; j++) {
            const int rr = base + j;
            if (rr < nrows) {
                const int gy = st.y0 - HALO + rr;
                const bool in = col.col_in && gy >= 0 && gy < H;  // outside the image: zeros
                Row r = nr[0];
                r.chain = in ? r.chain : 0.0f;
                r.a01 = (in ? r.a01 : v2f{0.0f, 0.0f}) * r.chain;
                r.a2 = (in ? r.a2 : 0.0f) * r.chain;
#pragma unroll
                for (int i = 0; i + 1 < AHEAD; i++) nr[i] = nr[i + 1];
                nr[AHEAD - 1] = fetch(rr + AHEAD);
                b01[cx] = r.a01; b2[cx] = r.a2;
                wave_sync();
                v2f s01 = 0;
                float s2 = 0;
#pragma unroll
                for (int d = 1; d <= HALO; d++) {
                    const float w = GAUSS[HALO - d];
                    s01 += (b01[cx - d] + b01[cx + d]) * w;
                    s2 += (b2[cx - d] + b2[cx + d]) * w;
                }
                wave_sync();
                h01[j] = s01 + r.a01 * GAUSS[HALO];
                h2[j] = s2 + r.a2 * GAUSS[HALO];
                if (rr >= 2 * HALO) {
                    const v2f v01 = ring_vertical(h01, j);
                    const float s[3] = {v01.x, v01.y, ring_vertical(h2, j)};
                    if (col.own) {
                        const int py = st.y0 + rr - 2 * HALO;
                        const float p1 = r.p1, p2 = r.p2;
                        float g = s[0] + 2.0f * p1 * s[1] + p2 * s[2];
                        if (LOSS) {
                            const float df = p1 - p2;
                            g = g + l1_scale * (df > 0.0f ? 1.0f : (df < 0.0f ? -1.0f : 0.0f));
                            float* o = &at(out + ch, (unsigned)(outC * W) * (unsigned)py, 4u * (unsigned)(outC * col.gxc()));
                            o[0] = g;
                            // the loss head only sees features[1:3]: the other channels of vpixels (C > 3) get their zeros
                            // here, from the last colour channel's wave (a launch of its own for them was 17 us in :rgbd mode)
                            if (ch == NPL - 1)
                                for (int c = 1; c <= outC - NPL; c++) o[c] = 0.0f;
                        } else {
                            at(out + po, (unsigned)W * (unsigned)py, yo) = g;
                        }
                    }
                }
            }
        }
    }
}

}  // namespace

// Strip height of a launch.  A wave's cost is 10 halo rows plus its output rows (a halo row costs about 0.4 of an output row:
// it has no vertical pass), the kernels are VALU-bound once there is a wave to hide another's loads, and a 1080p image is
// only a few waves per SIMD: what counts is the number of waves the fullest SIMD gets, times a wave's cost.  Pick the height
// that minimises it; at least three waves per SIMD, so that loads and the LDS round trip of one hide behind the others.
static int ssim_strip_h(int W, int H, int planes) {
    static const int n_simd = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        return 4 * cus;
    }();
    const long cols = (long)((W + STRIP_W - 1) / STRIP_W) * planes;
    int best = 8;
    long best_cost = -1;
    for (int h = 8; h <= 64; h++) {
        const long waves = cols * ((H + h - 1) / h);
        const long per_simd = (waves + n_simd - 1) / n_simd;
        const long cost = (per_simd < 3 ? 3 : per_simd) * (h + 4);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = h; }
    }
    return best;
}

template <int SPB>
static dim3 ssim_grid(int W, int H, int strip_h, int planes) {
    const int n = ((W + STRIP_W - 1) / STRIP_W) * ((H + strip_h - 1) / strip_h);
    const int groups = (n + SPB - 1) / SPB;
    return dim3(8 * ((groups + 7) / 8), 1, planes);
}

// pairs of `partial` the loss head's forward writes: one per wave of its launch
size_t SSIM_NAME(gsr_loss_partial_pairs)(int W, int H) {
    return (size_t)ssim_grid<LOSS_STRIPS>(W, H, ssim_strip_h(W, H, 3), 1).x * 3 * LOSS_STRIPS;
}

void SSIM_NAME(gsr_launch_ssim_fwd)(hipStream_t s, int W, int H, int CH, int B, const float* img, const float* ref, float C1,
                         float C2, int train, float* ssim_map, float* d0, float* d1, float* d2) {
    PlanarSrc src{img, ref, W, H};
    const int sh = ssim_strip_h(W, H, CH * B);
    hipLaunchKernelGGL((ssim_fwd_kernel<PlanarSrc, false, 1, 4>), ssim_grid<4>(W, H, sh, CH * B), dim3(256), 0, s, src, W, H, sh,
                       C1, C2, train, ssim_map, d0, d1, d2, (float*)nullptr);
}

void SSIM_NAME(gsr_launch_ssim_bwd)(hipStream_t s, int W, int H, int CH, int B, const float* img, const float* ref,
                         const float* dL_dmap, const float* d0, const float* d1, const float* d2, float* dL_dimg) {
    PlanarSrc src{img, ref, W, H};
    const int sh = ssim_strip_h(W, H, CH * B);
    hipLaunchKernelGGL((ssim_bwd_kernel<PlanarSrc, false, 1, 4>), ssim_grid<4>(W, H, sh, CH * B), dim3(256), 0, s, src, W, H, sh,
                       dL_dmap, 0.0f, 0.0f, d0, d1, d2, dL_dimg, 0, (const float*)nullptr, 0, 0.0f, 0.0f, (float*)nullptr);
}

void SSIM_NAME(gsr_launch_loss_fwd)(hipStream_t s, int W, int H, int C, const float* image, const float* target, float C1,
                         float C2, float* d0, float* d1, float* d2, float* partial) {
    RasterSrc src{image, target, W, H, C};
    const int sh = ssim_strip_h(W, H, 3);
    hipLaunchKernelGGL((ssim_fwd_kernel<RasterSrc, true, 3, LOSS_STRIPS>), ssim_grid<LOSS_STRIPS>(W, H, sh, 1),
                       dim3(64 * 3 * LOSS_STRIPS), 0, s, src, W, H, sh, C1, C2, 1, (float*)nullptr, d0, d1, d2, partial);
}

void SSIM_NAME(gsr_launch_loss_bwd)(hipStream_t s, int W, int H, int C, const float* image, const float* target, float lambda,
                         const float* d0, const float* d1, const float* d2, const float* partial, float* loss_out,
                         float* vpixels) {
    RasterSrc src{image, target, W, H, C};
    const float count = 3.0f * (float)W * (float)H;
    const float inv_count = 1.0f / count;
    const int sh = ssim_strip_h(W, H, 3);
    dim3 g = ssim_grid<LOSS_STRIPS>(W, H, sh, 1);
    const int n_partial = (int)(g.x * 3 * LOSS_STRIPS);  // one pair per wave of the forward launch
    g.x += 1;                                            // + the workgroup that finishes the scalar loss
    hipLaunchKernelGGL((ssim_bwd_kernel<RasterSrc, true, 3, LOSS_STRIPS>), g, dim3(64 * 3 * LOSS_STRIPS), 0, s, src, W, H, sh,
                       (const float*)nullptr, -lambda * inv_count, (1.0f - lambda) * inv_count, d0, d1, d2, vpixels,
                       C, partial, n_partial, lambda, inv_count, loss_out);
}
