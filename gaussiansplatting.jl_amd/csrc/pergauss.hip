// The backward of a view, per Gaussian: the fused ∇project! + ∇spherical_harmonics! (with the trainer tail as its FUSED
// epilogue), the fixed-order sum of its pose partials, and the densification statistics read from its ∇means_2d.
//
// Reference behaviour: src/rasterization/projection.jl:132-257, 289-393, spherical_harmonics.jl:20-38, 76-181,
// render.jl:302-320, 335-366, 383-413, src/strategy.jl:118-136.
//
// This translation unit is compiled with -ffp-contract=off, like preprocess.hip: the forward chain it recomputes
// (splat_math.h) gives the forward's floats bit for bit, and the gradients are bit-reproducible against the CPU oracle.
// The kernel is HBM-bound, the extra VALU ops are free.
#include "gsr_kernels.h"
#include "gsr_dispatch.h"
#include "tile_mask.h"
#include "wave_reduce.h"
#include "adam_math.h"
#include "splat_math.h"
#include "sh_rows.h"

namespace {
using namespace gsr::splat;
using gsr::dispatch_bool;
using gsr::dispatch_degree;
using gsr::store_sh_rows;
using gsr::tail_sh_group;

constexpr uint32_t DENSE_RECT = GSR_DENSE_RECT;  // rects up to which a Gaussian's rows are one per EMITTED tile (preprocess.hip)

__device__ __forceinline__ M33 add33(const M33& a, const M33& b) {
    M33 o;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) o.m[i][j] = a.m[i][j] + b.m[i][j];
    return o;
}
__device__ __forceinline__ M22 mul22(const M22& a, const M22& b) {
    M22 o;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) o.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j];
    return o;
}

// ∇unnorm_quat2rot (render.jl:335-366): vR = the rotation matrix cotangent, qn = the normalised quaternion (w, x, y, z),
// inv_norm = 1 / |q|.  One expression tree for the float64 chain and for the reference's fp32 chain.
template <class T>
__device__ __forceinline__ void unnorm_quat2rot_bwd(const T (&vR)[3][3], const T (&qn)[4], T inv_norm, float vq_out[4]) {
    const T w = qn[0], x = qn[1], y = qn[2], z = qn[3];
#define V(i_, j_) vR[(i_) - 1][(j_) - 1]
    T vqn[4];
    vqn[0] = T(2) * (x * (V(3, 2) - V(2, 3)) + y * (V(1, 3) - V(3, 1)) + z * (V(2, 1) - V(1, 2)));
    vqn[1] = T(2) * (T(-2) * x * (V(2, 2) + V(3, 3)) + y * (V(2, 1) + V(1, 2)) + z * (V(3, 1) + V(1, 3)) + w * (V(3, 2) - V(2, 3)));
    vqn[2] = T(2) * (x * (V(2, 1) + V(1, 2)) - T(2) * y * (V(1, 1) + V(3, 3)) + z * (V(3, 2) + V(2, 3)) + w * (V(1, 3) - V(3, 1)));
    vqn[3] = T(2) * (x * (V(3, 1) + V(1, 3)) + y * (V(3, 2) + V(2, 3)) - T(2) * z * (V(1, 1) + V(2, 2)) + w * (V(2, 1) - V(1, 2)));
#undef V
    const T dq = vqn[0] * qn[0] + vqn[1] * qn[1] + vqn[2] * qn[2] + vqn[3] * qn[3];
#pragma unroll
    for (int k = 0; k < 4; k++) vq_out[k] = (float)((vqn[k] - dq * qn[k]) * inv_norm);
}

// ---------------------------------------------------------------------------------
// ∇scales / ∇rotations IN FLOAT64 (round 5).  The reference's chain  vconic -> ∇inverse (render.jl:383-385) ->
// ∇perspective_projection (projection.jl:289-353) -> ∇covar_world_to_cam -> ∇quat_scale_to_cov (render.jl:302-320) ->
// ∇unnorm_quat2rot (render.jl:335-366) multiplies 2x2 and 3x3 matrices whose eigenvalues differ by the SQUARE of a splat's
// aspect ratio.  For the flat, needle-projecting splats a trained scene is full of (scale ratios of 100 and more) fp32 loses
// the thin eigen-direction in every one of those products: the last bit of vconic — any summation order's — moves ∇rotations
// by 1e-3 relative, in the reference's kernels, in the CPU oracle and here alike, although the map itself is well conditioned
// (kappa ~ 3-10: the float64 replay of the oracle, oracle/gsr_oracle.c ORC_REAL_DOUBLE, is insensitive to those bits).  This
// kernel is HBM-bound; ~250 double-precision FMAs per visible Gaussian cost nothing (7 us of 140 at config 3).  So the part
// of the pullback that ends in ∇scales / ∇rotations runs in float64 FROM THE RAW INPUTS (the forward's fp32 conic cannot
// hold the thin eigenvalue either): the same formulas, vSigma = T' vS2 T folded with T = J R so that no 3x3 product of
// ill-scaled factors is ever rounded.  ∇means (well scaled) keeps the fp32 expression trees of the reference.
//   va, vb, vc: the summed conic cotangent (vb on both off-diagonal entries, as the reference places it); vRg: the normal
//   channel's contribution to the rotation matrix cotangent (projection.jl:227-235), zero outside :rgbdn.
// ---------------------------------------------------------------------------------
//   AA: rho, vrho = the forward's compensation and its cotangent; ∇add_blur (render.jl:398-413) is added to vS2 below.
template <bool AA>
__device__ __forceinline__ void scales_rots_bwd_f64(const GsrCam& cam, const M33& Rf, const float tf[3], const float pf[3],
                                                    const float4 q4, const float sf[3], float va, float vb, float vc,
                                                    const M33& vRg, float rho, float vrho, float vs_out[3], float vq_out[4]) {
    double R[3][3], mc[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) R[r][c] = (double)Rf.m[r][c];
        mc[r] = (R[r][0] * (double)pf[0] + R[r][1] * (double)pf[1] + R[r][2] * (double)pf[2]) + (double)tf[r];
    }
    // projection.jl:259-287 (persp_common of splat_math.h, in double)
    const double rz = 1.0 / mc[2], rz2 = rz * rz;
    const int res[2] = {cam.width, cam.height};
    double J02[2], J00[2];  // J = [J00[0] 0 J02[0]; 0 J00[1] J02[1]]
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const double fk = (double)cam.focal[k], rk = (double)res[k];
        const double stf = 0.3 * ((0.5 * rk) / fk), pp = (double)cam.principal[k] * rk;
        const double lim = (rk - pp) / fk + stf, lim_neg = pp / fk + stf;
        const double c = fmin(lim, fmax(-lim_neg, mc[k] * rz));
        J00[k] = fk * rz;
        J02[k] = -fk * (mc[2] * c) * rz2;
    }
    // render.jl:322-333 (quat2rot) and M = Rg diag(s)
    const double qw = (double)q4.x, qx = (double)q4.y, qy = (double)q4.z, qz = (double)q4.w;
    const double inv_norm = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    const double w = qw * inv_norm, x = qx * inv_norm, y = qy * inv_norm, z = qz * inv_norm;
    double Rg[3][3];
    Rg[0][0] = 1.0 - 2.0 * (y * y + z * z); Rg[1][0] = 2.0 * (x * y + w * z); Rg[2][0] = 2.0 * (x * z - w * y);
    Rg[0][1] = 2.0 * (x * y - w * z); Rg[1][1] = 1.0 - 2.0 * (x * x + z * z); Rg[2][1] = 2.0 * (y * z + w * x);
    Rg[0][2] = 2.0 * (x * z + w * y); Rg[1][2] = 2.0 * (y * z - w * x); Rg[2][2] = 1.0 - 2.0 * (x * x + y * y);
    const double s[3] = {(double)sf[0], (double)sf[1], (double)sf[2]};
    // T = J R (2x3), TM = T Rg diag(s) (2x3)
    double T[2][3], TM[2][3];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) T[a][c] = J00[a] * R[a][c] + J02[a] * R[2][c];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) TM[a][c] = (T[a][0] * Rg[0][c] + T[a][1] * Rg[1][c] + T[a][2] * Rg[2][c]) * s[c];
    // Sigma_2D = TM TM' + blur (projection.jl:96-100), conic = its inverse
    const double S00 = TM[0][0] * TM[0][0] + TM[0][1] * TM[0][1] + TM[0][2] * TM[0][2] + (double)cam.blur_eps;
    const double S01 = TM[0][0] * TM[1][0] + TM[0][1] * TM[1][1] + TM[0][2] * TM[1][2];
    const double S11 = TM[1][0] * TM[1][0] + TM[1][1] * TM[1][1] + TM[1][2] * TM[1][2] + (double)cam.blur_eps;
    const double det_inv = 1.0 / (S00 * S11 - S01 * S01);
    const double Ca = S11 * det_inv, Cb = -S01 * det_inv, Cc = S00 * det_inv;
    // vS2 = -C vC C (render.jl:383-385), symmetric
    const double a_ = (double)va, b_ = (double)vb, c_ = (double)vc;
    const double P00 = Ca * a_ + Cb * b_, P01 = Ca * b_ + Cb * c_, P10 = Cb * a_ + Cc * b_, P11 = Cb * b_ + Cc * c_;
    double V00 = -(P00 * Ca + P01 * Cb), V01 = -(P00 * Cb + P01 * Cc), V11 = -(P10 * Cb + P11 * Cc);
    if constexpr (AA) {
        // ∇add_blur (render.jl:398-413) on the conic: vS2 += vs ((1 - rho²) C - eps det(C) I), the pullback of
        // rho = sqrt(det S / det(S + eps I)) (adj(S) = adj(S + eps I) - eps I in 2 x 2), with the reference's 1e-6 under vs
        const double r_ = (double)rho, vsq = 0.5 * (double)vrho / (r_ + 1e-6), ct = 1.0 - r_ * r_;
        const double ed = (double)cam.blur_eps * (Ca * Cc - Cb * Cb);
        V00 += vsq * (ct * Ca - ed); V01 += vsq * ct * Cb; V11 += vsq * (ct * Cc - ed);
    }
    // vM = (vSigma + vSigma') M with vSigma = T' vS2 T:  vM = 2 T' (vS2 TM)
    double X[2][3], vM[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++) { X[0][c] = V00 * TM[0][c] + V01 * TM[1][c]; X[1][c] = V01 * TM[0][c] + V11 * TM[1][c]; }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) vM[r][c] = 2.0 * (T[0][r] * X[0][c] + T[1][r] * X[1][c]);
    double vRq[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        vs_out[c] = (float)(Rg[0][c] * vM[0][c] + Rg[1][c] * vM[1][c] + Rg[2][c] * vM[2][c]);
#pragma unroll
        for (int r = 0; r < 3; r++) vRq[r][c] = vM[r][c] * s[c] + (double)vRg.m[r][c];
    }
    const double qn[4] = {w, x, y, z};
    unnorm_quat2rot_bwd<double>(vRq, qn, inv_norm, vq_out);
}

// One gradient row (GSR_ROW_F4(channels) float4, written by composite_bwd) onto the 13 sums of pergauss_bwd_kernel (acc
// layout: at sum_gradient_rows); f3 is read for channels > 5 only.  The four-in-flight form of the row sum adds through it.
__device__ __forceinline__ void add_row(float acc[16], const float4& f0, const float4& f1, const float4& f2, const float4& f3,
                                        int channels) {
    acc[0] += f0.x; acc[1] += f0.y; acc[2] += f0.z; acc[3] += f0.w;
    acc[4] += f1.x; acc[5] += f1.y; acc[6] += f1.z; acc[7] += f1.w;
    acc[8] += f2.x; acc[9] += f2.y;
    if (channels > 5) { acc[10] += f2.z; acc[11] += f2.w; acc[12] += f3.x; }
}
// coefficient of band k >= 1, channel c, of an SH row that starts at band 1 (∇SH of pergauss_bwd_kernel)
__device__ __forceinline__ float sh_coeff(const float* sh, int k, int c) { return sh[3 * (k - 1) + c]; }

// pos_world_to_cam (projection.jl:75)
__device__ __forceinline__ void to_camera(const M33& R, const float t[3], const float p[3], float mc[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) mc[r] = (R.m[r][0] * p[0] + R.m[r][1] * p[1] + R.m[r][2] * p[2]) + t[r];
}

// The forward chain both per-Gaussian kernels start from (projection.jl:76-95): the Gaussian's rotation Rg with the
// normalised quaternion qn and 1 / |q|, M = Rg diag(s), Sigma = M M', its camera-space image Sc = R Sigma R', and the
// perspective terms at the camera-space mean mc.  project_bwd recomputes it through this function; preprocess_kernel keeps
// the same expression trees written out inside its (inline) projection.  A caller reads the members it needs, the others
// are dead code there.
struct ForwardChain {
    M33 Rg, M, Sigma, Sc;
    float qn[4], inv_norm;
    Persp pr;
};
__device__ __forceinline__ ForwardChain forward_chain(const M33& R, const float mc[3], const float4 q4, const float s[3],
                                                      const GsrCam& cam) {
    ForwardChain c;
    c.Rg = quat2rot(q4, c.qn, c.inv_norm);
    c.Sigma = cov3d(c.Rg, s, c.M);
    c.Sc = mul33(mul33(R, c.Sigma), tr33(R));
    c.pr = persp_common(mc, cam);
    return c;
}

// ---------------------------------------------------------------------------------
// The stages of pergauss_bwd_kernel (below), in the order the kernel runs them.
// ---------------------------------------------------------------------------------
// Sum this Gaussian's per-instance gradient rows (written by composite_bwd).
// acc: [0..2] v rgb, [3] v opacity, [4..6] v conic, [7] v depth, [8..9] v mean2d, [10..12] v normal
//   in: visible, the record (rect, slot offset, emitted mask, footprint floats), geom.bpre, the rows.  out: acc[0..12]
//   (zeros for a culled Gaussian).  The sums run in ascending slot order (per lane; the wave-cooperative form: lane-strided
//   partial sums, then wave_reduce_transposed<13>) — fixed orders, bit-reproducible gradients.  No template flag.
__device__ __forceinline__ void sum_gradient_rows(int i, bool visible, const GsrGeoRec& rec, const GsrGeom& geom, const GsrCam& cam,
                                                  const GsrInst& inst, int channels, float acc[16]) {
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = 0.0f;
    uint32_t area = 0, goff = 0;
    if (visible) {
        const uint32_t lo = __float_as_uint(rec.q3.x), hi = __float_as_uint(rec.q3.y);
        area = ((hi & 0xFFFFu) - (lo & 0xFFFFu)) * ((hi >> 16) - (lo >> 16));
        goff = geom.bpre[i >> 8] + __float_as_uint(rec.q2.w);
    }
    constexpr uint32_t BIG = 48;  // larger footprints are summed by the whole wave
    // Rects beyond DENSE_RECT tiles: slots of tiles the exact footprint test culled at binning were never written by
    // composite_bwd (no instance exists): they are skipped by repeating the SAME test, on the
    // same record floats, compiled with the flags of the count / scatter kernels (preprocess.hip: -ffp-contract=off).
    uint32_t rx0 = 0, ry0 = 0, rw = 1;
    float tau = 0.0f;
    if (visible) {
        const uint32_t lo = __float_as_uint(rec.q3.x), hi = __float_as_uint(rec.q3.y);
        rx0 = lo & 0xFFFFu; ry0 = lo >> 16; rw = (hi & 0xFFFFu) - rx0;
        tau = footprint_tau(rec.q1.y);
    }
    if (area <= BIG) {
        // Which of the rect's tiles hold an instance (pure ALU), then the row loads in batches of ROWS_IN_FLIGHT:
        // a thread that waits for each 64-byte row before asking for the next one spends its life in memory
        // latency (3 waves per SIMD cannot hide it).  The sums run in ascending slot order whatever the batching
        // (fixed order -> bit-reproducible gradients).
        unsigned long long emask = 0ull;
        if (area <= DENSE_RECT) {
            // small rect: its emitted tiles own consecutive slots (preprocess left their mask in the record)
            // (the record of a culled Gaussian was never written: stale bits)
            const uint32_t cnt = visible ? (uint32_t)__popc(__float_as_uint(rec.q3.w)) : 0u;
            emask = cnt ? (~0ull >> (64u - cnt)) : 0ull;
        } else {
            uint32_t tx = rx0, ty = ry0;
            for (uint32_t k = 0; k < area; k++) {
                const bool emitted = !cam.exact_cull || tile_may_touch(rec.q0.x, rec.q0.y, rec.q0.z, rec.q0.w, rec.q1.x,
                                                                       tau, (int)tx * GSR_TILE, (int)ty * GSR_TILE);
                if (++tx == rx0 + rw) { tx = rx0; ty++; }
                emask |= emitted ? (1ull << k) : 0ull;
            }
        }
        while (emask) {
            // up to four rows in flight (explicitly unrolled: arrays indexed by the batch slot end up in scratch)
            const uint32_t k0 = (uint32_t)__builtin_ctzll(emask); emask &= emask - 1ull;
            const bool h1 = emask != 0ull; const uint32_t k1 = h1 ? (uint32_t)__builtin_ctzll(emask) : k0; emask &= emask - 1ull;
            const bool h2 = emask != 0ull; const uint32_t k2 = h2 ? (uint32_t)__builtin_ctzll(emask) : k0; emask &= emask - 1ull;
            const bool h3 = emask != 0ull; const uint32_t k3 = h3 ? (uint32_t)__builtin_ctzll(emask) : k0; emask &= emask - 1ull;
            const float4* r0 = inst.rows + (size_t)GSR_ROW_F4(channels) * (goff + k0);
            const float4* r1 = inst.rows + (size_t)GSR_ROW_F4(channels) * (goff + k1);
            const float4* r2 = inst.rows + (size_t)GSR_ROW_F4(channels) * (goff + k2);
            const float4* r3 = inst.rows + (size_t)GSR_ROW_F4(channels) * (goff + k3);
            const float4 a0 = r0[0], a1 = r0[1], a2 = r0[2];
            const float4 b0 = r1[0], b1 = r1[1], b2 = r1[2];
            const float4 c0 = r2[0], c1 = r2[1], c2 = r2[2];
            const float4 d0 = r3[0], d1 = r3[1], d2 = r3[2];
            float4 a3 = a2, b3 = a2, c3 = a2, d3 = a2;
            if (channels > 5) { a3 = r0[3]; b3 = r1[3]; c3 = r2[3]; d3 = r3[3]; }
            add_row(acc, a0, a1, a2, a3, channels);
            if (h1) add_row(acc, b0, b1, b2, b3, channels);  // (a duplicate load stands in for a missing row; it is not added)
            if (h2) add_row(acc, c0, c1, c2, c3, channels);
            if (h3) add_row(acc, d0, d1, d2, d3, channels);
        }
    }
    {
        __shared__ float bounce[4][16];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const gsr::LaneBits lb(lane);
        const int slot = gsr::wave_reduce_index<13>(lane);
        unsigned long long big = __ballot(area > BIG);
        while (big) {
            const int src = __builtin_ctzll(big);
            big &= big - 1;
            const uint32_t a = __shfl(area, src), o = __shfl(goff, src);
            const uint32_t sx0 = __shfl(rx0, src), sy0 = __shfl(ry0, src), sw = __shfl(rw, src);
            const float smx = __shfl(rec.q0.x, src), smy = __shfl(rec.q0.y, src), sa = __shfl(rec.q0.z, src),
                        sb = __shfl(rec.q0.w, src), sc = __shfl(rec.q1.x, src), stau = __shfl(tau, src);
            float part[16];
#pragma unroll
            for (int k = 0; k < 16; k++) part[k] = 0.0f;
            for (uint32_t k = lane; k < a; k += 64) {
                const uint32_t tx = sx0 + k % sw, ty = sy0 + k / sw;
                if (cam.exact_cull && !tile_may_touch(smx, smy, sa, sb, sc, stau, (int)tx * GSR_TILE, (int)ty * GSR_TILE))
                    continue;
                const float4* row = inst.rows + (size_t)GSR_ROW_F4(channels) * (o + k);
                const float4 f0 = row[0], f1 = row[1], f2 = row[2];
                part[0] += f0.x; part[1] += f0.y; part[2] += f0.z; part[3] += f0.w;
                part[4] += f1.x; part[5] += f1.y; part[6] += f1.z; part[7] += f1.w;
                part[8] += f2.x; part[9] += f2.y;
                if (channels > 5) {
                    const float4 f3 = row[3];
                    part[10] += f2.z; part[11] += f2.w; part[12] += f3.x;
                }
            }
            const float total = gsr::wave_reduce_transposed<13>(part, lb);
            if (gsr::wave_reduce_writer(lane)) bounce[wave][slot] = total;
            __builtin_amdgcn_wave_barrier();
            if (lane == src) {
#pragma unroll
                for (int k = 0; k < 13; k++) acc[k] = bounce[wave][k];
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// ∇project (projection.jl:170-256) of a visible Gaussian, from the forward chain recomputed on its raw inputs.
//   in: the pose R, t; p, q4, s; the record's conic (q0.z, q0.w, q1.x); a1 = (v conic a, b, c, v depth), vm2 = v mean2d.
//   out: the struct below — vmean (the projection's share of ∇means), vSigma (fp32 chain only), and the forward values the
//   next stages read (mc, Rg: normal channel; M, qn, inv_norm: fp32 chain); with_pose: the thresholded pose terms of this
//   Gaussian in poseR (∇R, column-major) / poset (projection.jl:243-256), else left as they are.  No template flag.
struct ProjectBwd {
    float mc[3];
    M33 Rg, M;
    float qn[4], inv_norm;
    float vmean[3];
    M33 vSigma;
};
//   AA: rho, vrho = the forward's compensation (GSR_BUF_COMPENSATIONS, re-read as the reference re-reads compensations[i]) and
//   its cotangent; ∇add_blur is added to the 2-D covariance cotangent before anything reads it.  Depends on AA.
template <bool AA>
__device__ __forceinline__ ProjectBwd project_bwd(const GsrCam& cam, const M33& R, const float t[3], const float p[3],
                                                  const float4 q4, const float s[3], const GsrGeoRec& rec, const float4 a1,
                                                  const float2 vm2, float rho, float vrho, int channels, bool with_pose,
                                                  float poseR[9], float poset[3]) {
    ProjectBwd o;
    const float4 g0 = rec.q0, g1 = rec.q1;
    M22 Ci, vCi;
    Ci.m[0][0] = g0.z; Ci.m[1][0] = g0.w; Ci.m[0][1] = g0.w; Ci.m[1][1] = g1.x;
    vCi.m[0][0] = a1.x; vCi.m[1][0] = a1.y; vCi.m[0][1] = a1.y; vCi.m[1][1] = a1.z;
    M22 nC;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) nC.m[a][b] = -Ci.m[a][b];
    M22 vS2 = mul22(mul22(nC, vCi), Ci);  // ∇inverse (render.jl:383-385)
    if constexpr (AA) {
        // ∇add_blur (render.jl:398-413).  The reference hands it the conic where its parameter is named Σ_2D_blur; the
        // formula is the right one for the conic: vs ((1 - rho²) C - eps det(C) I).  rho == 0: finite (the 1e-6), times vrho = 0.
        const float dc = Ci.m[0][0] * Ci.m[1][1] - Ci.m[0][1] * Ci.m[1][0];
        const float vsq = 0.5f * vrho / (rho + 1e-6f);
        const float ct = 1.0f - rho * rho;
        vS2.m[0][0] = vS2.m[0][0] + vsq * (ct * Ci.m[0][0] - cam.blur_eps * dc);
        vS2.m[1][0] = vS2.m[1][0] + vsq * ct * Ci.m[1][0];
        vS2.m[0][1] = vS2.m[0][1] + vsq * ct * Ci.m[0][1];
        vS2.m[1][1] = vS2.m[1][1] + vsq * (ct * Ci.m[1][1] - cam.blur_eps * dc);
    }
    to_camera(R, t, p, o.mc);
    const float* mc = o.mc;
    const ForwardChain fc = forward_chain(R, mc, q4, s, cam);
    o.Rg = fc.Rg; o.M = fc.M; o.inv_norm = fc.inv_norm;
#pragma unroll
    for (int k = 0; k < 4; k++) o.qn[k] = fc.qn[k];
    const M33& Sigma = fc.Sigma;
    const M33& Sc = fc.Sc;
    const Persp& pr = fc.pr;
    const float rz = pr.rz, rz2 = rz * rz, rz3 = rz2 * rz;
    const float* f = cam.focal;
    // ∇perspective_projection (projection.jl:289-353)
    float JtV[3][2];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) JtV[a][b] = pr.J[0][a] * vS2.m[0][b] + pr.J[1][a] * vS2.m[1][b];
    M33 vSc;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) vSc.m[a][b] = JtV[a][0] * pr.J[0][b] + JtV[a][1] * pr.J[1][b];
    float A[2][3], B[2][3], vJ[2][3];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            A[a][b] = vS2.m[a][0] * pr.J[0][b] + vS2.m[a][1] * pr.J[1][b];
            B[a][b] = vS2.m[0][a] * pr.J[0][b] + vS2.m[1][a] * pr.J[1][b];
        }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            float u = A[a][0] * Sc.m[b][0] + A[a][1] * Sc.m[b][1] + A[a][2] * Sc.m[b][2];
            float v = B[a][0] * Sc.m[0][b] + B[a][1] * Sc.m[1][b] + B[a][2] * Sc.m[2][b];
            vJ[a][b] = u + v;
        }
    float vx = f[0] * rz * vm2.x;
    float vy = f[1] * rz * vm2.y;
    float vz = -rz2 * (f[0] * mc[0] * vm2.x + f[1] * mc[1] * vm2.y);
    float rx = mc[0] * rz, ry = mc[1] * rz;
    if (-pr.lim_neg[0] <= rx && rx <= pr.lim[0]) vx += -f[0] * rz2 * vJ[0][2];
    else vz += -f[0] * rz3 * vJ[0][2] * pr.txy[0];
    if (-pr.lim_neg[1] <= ry && ry <= pr.lim[1]) vy += -f[1] * rz2 * vJ[1][2];
    else vz += -f[1] * rz3 * vJ[1][2] * pr.txy[1];
    vz += -f[0] * rz2 * vJ[0][0] - f[1] * rz2 * vJ[1][1] + 2.0f * f[0] * pr.txy[0] * rz3 * vJ[0][2] +
          2.0f * f[1] * pr.txy[1] * rz3 * vJ[1][2];
    float vmc[3] = {vx, vy, vz};
    if (channels > 3) vmc[2] = vmc[2] + a1.w;  // vdepth (projection.jl:218-222)
    // ∇pos_world_to_cam, ∇covar_world_to_cam
#pragma unroll
    for (int c = 0; c < 3; c++) o.vmean[c] = R.m[0][c] * vmc[0] + R.m[1][c] * vmc[1] + R.m[2][c] * vmc[2];
    o.vSigma = mul33(mul33(tr33(R), vSc), R);
    if (with_pose) {
        M33 vR0;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) vR0.m[r][c] = vmc[r] * p[c];
        M33 u = mul33(mul33(vSc, R), tr33(Sigma));
        M33 v = mul33(mul33(tr33(vSc), R), Sigma);
        M33 vR2 = add33(add33(vR0, u), v);
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) poseR[c * 3 + r] = fabsf(vR2.m[r][c]) > 1e-7f ? vR2.m[r][c] : 0.0f;
            poset[r] = fabsf(vmc[r]) > 1e-7f ? vmc[r] : 0.0f;
        }
    }
    return o;
}

// The normal channel's pullback (projection.jl:227-235): the cotangent of the Gaussian's rotation matrix from acc[10..12].
//   out: vRg (zeros unless channels > 5).  No template flag.
__device__ __forceinline__ void normal_bwd(int channels, const float acc[16], const M33& R, const M33& Rg, const float s[3],
                                           const float mc[3], M33& vRg) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) vRg.m[a][b] = 0.0f;
    if (channels > 5) {
        const float4 a2 = make_float4(acc[10], acc[11], acc[12], 0.0f);
        float nn[3]; int k; float sg;
        gaussian_normal(R, Rg, s, mc, nn, k, sg);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            float g = R.m[0][r] * a2.x + R.m[1][r] * a2.y + R.m[2][r] * a2.z;
            float v = sg * g;
            vRg.m[r][0] = k == 0 ? v : 0.0f;
            vRg.m[r][1] = k == 1 ? v : 0.0f;
            vRg.m[r][2] = k == 2 ? v : 0.0f;
        }
    }
}

// ∇spherical_harmonics! with respect to the direction (spherical_harmonics.jl:76-181).
//   in: sh = the coefficients of band 1 on (3 floats per band; band 0 has no directional gradient), p, the camera centre,
//   vc = the colour cotangent with the clamp mask applied.  out: b = the SH basis at the view direction (the coefficient
//   gradient is the outer product b x vc, stored by store_or_apply_sh), vmsh = the SH stage's share of ∇means.  Depends on DEG.
//   JAC: sh = the nine floats of d rgb / d dir that the row-independent job of composite_bwd's launch stored for this Gaussian
//   (splat_math.h: sh_dir_jacobian, the expression evaluated here otherwise — the same bits), read instead of the SH bands.
template <int DEG, bool JAC = false>
__device__ __forceinline__ void sh_bwd(const float* sh, const float p[3], const GsrCam& cam, const float vc[3], float b[16],
                                       float vmsh[3]) {
    float d0[3], dir[3];
    view_dir(p, cam.center, d0, dir);
    sh_basis<DEG>(dir, b);
    float dcx[3] = {0, 0, 0}, dcy[3] = {0, 0, 0}, dcz[3] = {0, 0, 0};
    if constexpr (JAC) {
        // (sh = the Gaussian's nine floats, as the row-independent job of composite_bwd's launch stored them)
        if (DEG > 0) {
#pragma unroll
            for (int c = 0; c < 3; c++) { dcx[c] = sh[c]; dcy[c] = sh[3 + c]; dcz[c] = sh[6 + c]; }
        }
    } else {
    // (the text of splat_math.h's sh_dir_jacobian, kept here: through the function the compiler folds the negated constants of
    //  band 3 another way — the same floats, but not this kernel's instructions)
    if (DEG > 0) {
        const float x = dir[0], y = dir[1], z = dir[2];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            dcx[c] = -SH1 * sh_coeff(sh, 3, c); dcy[c] = -SH1 * sh_coeff(sh, 1, c); dcz[c] = SH1 * sh_coeff(sh, 2, c);
        }
        if (DEG > 1) {
            float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                dcx[c] = dcx[c] + SH2C1 * y * sh_coeff(sh, 4, c) + SH2C3 * 2.0f * -x * sh_coeff(sh, 6, c) +
                         SH2C4 * z * sh_coeff(sh, 7, c) + SH2C5 * 2.0f * x * sh_coeff(sh, 8, c);
                dcy[c] = dcy[c] + SH2C1 * x * sh_coeff(sh, 4, c) + SH2C2 * z * sh_coeff(sh, 5, c) +
                         SH2C3 * 2.0f * -y * sh_coeff(sh, 6, c) + SH2C5 * 2.0f * -y * sh_coeff(sh, 8, c);
                dcz[c] = dcz[c] + SH2C2 * y * sh_coeff(sh, 5, c) + SH2C3 * 4.0f * z * sh_coeff(sh, 6, c) +
                         SH2C4 * x * sh_coeff(sh, 7, c);
            }
            if (DEG > 2) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    dcx[c] = dcx[c] + SH3C1 * sh_coeff(sh, 9, c) * 3.0f * 2.0f * xy + SH3C2 * sh_coeff(sh, 10, c) * yz +
                             SH3C3 * sh_coeff(sh, 11, c) * -2.0f * xy + SH3C4 * sh_coeff(sh, 12, c) * -3.0f * 2.0f * xz +
                             SH3C5 * sh_coeff(sh, 13, c) * (-3.0f * x2 + 4.0f * z2 - y2) +
                             SH3C6 * sh_coeff(sh, 14, c) * 2.0f * xz + SH3C7 * sh_coeff(sh, 15, c) * 3.0f * (x2 - y2);
                    dcy[c] = dcy[c] + SH3C1 * sh_coeff(sh, 9, c) * 3.0f * (x2 - y2) + SH3C2 * sh_coeff(sh, 10, c) * xz +
                             SH3C3 * sh_coeff(sh, 11, c) * (-3.0f * y2 + 4.0f * z2 - x2) +
                             SH3C4 * sh_coeff(sh, 12, c) * -3.0f * 2.0f * yz + SH3C5 * sh_coeff(sh, 13, c) * -2.0f * xy +
                             SH3C6 * sh_coeff(sh, 14, c) * -2.0f * yz + SH3C7 * sh_coeff(sh, 15, c) * -3.0f * 2.0f * xy;
                    dcz[c] = dcz[c] + SH3C2 * sh_coeff(sh, 10, c) * xy + SH3C3 * sh_coeff(sh, 11, c) * 4.0f * 2.0f * yz +
                             SH3C4 * sh_coeff(sh, 12, c) * 3.0f * (2.0f * z2 - x2 - y2) +
                             SH3C5 * sh_coeff(sh, 13, c) * 4.0f * 2.0f * xz + SH3C6 * sh_coeff(sh, 14, c) * (x2 - y2);
                }
            }
        }
    }
    }
    float vdir[3];
    vdir[0] = dcx[0] * vc[0] + dcx[1] * vc[1] + dcx[2] * vc[2];
    vdir[1] = dcy[0] * vc[0] + dcy[1] * vc[1] + dcy[2] * vc[2];
    vdir[2] = dcz[0] * vc[0] + dcz[1] * vc[1] + dcz[2] * vc[2];
    // ∇normalize (spherical_harmonics.jl:174-181)
    float s2 = d0[0] * d0[0] + d0[1] * d0[1] + d0[2] * d0[2];
    float inv_s = 1.0f / sqrtf(s2 * s2 * s2);
    vmsh[0] = ((s2 - d0[0] * d0[0]) * vdir[0] - d0[1] * d0[0] * vdir[1] - d0[2] * d0[0] * vdir[2]) * inv_s;
    vmsh[1] = (-d0[0] * d0[1] * vdir[0] + (s2 - d0[1] * d0[1]) * vdir[1] - d0[2] * d0[1] * vdir[2]) * inv_s;
    vmsh[2] = (-d0[0] * d0[2] * vdir[0] - d0[1] * d0[2] * vdir[1] + (s2 - d0[2] * d0[2]) * vdir[2]) * inv_s;
}

// The SH part of the gradient is the outer product basis x colour cotangent: its factors wait in LDS and the whole
// workgroup writes (FUSED: updates) the workgroup's contiguous slice element-major, as full cache lines.
//   in: per thread, the factors f_b (basis), f_vc (colour cotangent), f_nb (bands carrying a gradient; 0: culled), and for
//   FUSED the Gaussian's own gradients f_vmean, f_vopac, f_vs, f_vq.  out: !FUSED: vshs (unless vcolors: the factored
//   form left the kernel already); FUSED: the trainer tail applied to TS (adam_math.h).  Depends on FUSED.
//   JAC (!FUSED, no vcolors): the rows of culled Gaussians are not this launch's — the row-independent job wrote their zeros.
template <bool FUSED, bool JAC = false>
__device__ __forceinline__ void store_or_apply_sh(int i, int n, int K, float* __restrict__ vshs, const float* vcolors,
                                                  const gsr::TailState& TS, const float f_b[16], const float f_vc[3],
                                                  int f_nb, const float f_vmean[3], float f_vopac, const float f_vs[3],
                                                  const float f_vq[4]) {
    __shared__ float tail_b[256][17];  // SH basis of each Gaussian of the workgroup (odd stride: no bank conflicts)
    __shared__ float tail_vc[256][3];  // its colour cotangent (clamp mask applied)
    __shared__ int tail_nb[256];       // SH bands carrying a gradient (0: culled Gaussian)
    const int i0 = blockIdx.x * 256;
    const int cnt = min(256, n - i0);
    const int K3 = 3 * K;
    if (FUSED || !vcolors) {
#pragma unroll
        for (int k = 0; k < 16; k++) tail_b[threadIdx.x][k] = f_b[k];
#pragma unroll
        for (int c = 0; c < 3; c++) tail_vc[threadIdx.x][c] = f_vc[c];
        tail_nb[threadIdx.x] = f_nb;
    }
    if constexpr (!FUSED) {
        if (!vcolors) {
            __syncthreads();
            auto value = [&](int il, int j) {
                const int k = j / 3, c = j - 3 * k;
                return k < tail_nb[il] ? tail_b[il][k] * tail_vc[il][c] : 0.0f;
            };
            if constexpr (JAC) gsr::store_sh_rows_where(vshs, i0, cnt, K3, value, [&](int il) { return tail_nb[il] != 0; });
            else store_sh_rows(vshs, i0, cnt, K3, value);
        }
    }
    if constexpr (FUSED) {
        if (i < n) gsr::tail_gauss_apply(TS, i, f_vmean, f_vopac, f_vs, f_vq);
        __syncthreads();
        // (g(il, k, c): the SH-coefficient gradient of Gaussian il of the workgroup, band k, channel c)
        auto grad = [&](int il, int k, int c) { return k < tail_nb[il] ? tail_b[il][k] * tail_vc[il][c] : 0.0f; };
        auto sh_group = [&](float* __restrict__ th, float* __restrict__ mu, float* __restrict__ nu, int R, int k0,
                            const gsr::AdamHyper& hy) { tail_sh_group(TS, i0, cnt, K3, th, mu, nu, R, k0, hy, grad); };
        sh_group(TS.dc, TS.dc_mu, TS.dc_nu, 3, 0, TS.h_dc);
        if (K > 1) sh_group(TS.rest, TS.rest_mu, TS.rest_nu, 3 * (K - 1), 1, TS.h_rest);
    }
}

// ---------------------------------------------------------------------------------
// fused ∇project! (projection.jl:170-256) + ∇spherical_harmonics!
// (spherical_harmonics.jl:32-37,76-181).  Every output element is written exactly
// once (zeros for culled Gaussians and for SH bands above the active degree), so the
// 59·N-float gradient arena needs no memset.
//
// FUSED: the single-GPU trainer step.  The 59 gradient floats of a Gaussian never reach HBM: the
// trainer tail (pullback of the sigmoid / exp prologue + the six NU.Adam updates + the activated
// copies of the next forward; trainer.hip, training.jl:768-779) is applied in the epilogue.  The
// per-Gaussian groups are updated by the owning thread; the SH groups (48 of the 59 floats) by the
// whole workgroup, element-major over the workgroup's contiguous slice of features_dc /
// features_rest so that θ, μ, ν stream as full cache lines — the per-Gaussian factors of the SH
// gradient (basis x colour cotangent) wait in LDS.  `means` / `rots` ARE the raw points / rotations,
// `scales` the activated copy; the SH coefficients are read from features_rest (the hcat copy `shs`
// is only written).  Same expression trees as the unfused chain (adam_math.h): identical bits.
// ---------------------------------------------------------------------------------
// F32CHAIN (gsr_config.grad_precision = GSR_GRAD_FP32_REFERENCE): ∇scales / ∇rotations through the reference's own fp32
// expression trees instead of the float64 chain — reference-parity runs; a template parameter, not a branch, so
// that the default kernels are round 5's register for register.
// AA (GSR_FLAG_ANTIALIASED): the row sum acc[3] is the cotangent of the EFFECTIVE opacity o * rho the forward put into the
// record.  ∇opacity = acc[3] * rho is with respect to the caller's o; v rho = acc[3] * o goes through ∇add_blur into the 2-D
// covariance cotangent of both chains (project_bwd, scales_rots_bwd_f64).  `comp` = the forward's compensations, `opac` = the
// caller's opacities (FUSED: TS.opac_act): 8 more bytes per Gaussian.  A template parameter for the same reason.
// JAC (!FUSED, !F32CHAIN, no vcolors; gsr_launch_pergauss_bwd): the launch behind a composite_bwd launch that carried the
// row-independent job (bwd_row_job.h).  `shs` is then the job's Jacobian buffer, nine floats per Gaussian (the SH bands are not
// read at all: 36 bytes instead of up to 180 per visible Gaussian), and the gradient rows of a culled Gaussian are left alone:
// the job wrote their zeros.  ∇means_2d is still written for every Gaussian here.  A template parameter for the same reason.
template <int DEG, bool FUSED, bool F32CHAIN = false, bool AA = false, bool JAC = false>
__global__ __launch_bounds__(256, 1) void pergauss_bwd_kernel(int n, int K, int channels, const float* __restrict__ means,
                                                           const float* __restrict__ scales,
                                                           const float4* __restrict__ rots,
                                                           const float* __restrict__ shs, GsrCam cam, GsrGeom geom,
                                                           GsrInst inst, float2* __restrict__ vmean2d_out,
                                                           float* __restrict__ vmeans,
                                                           float* __restrict__ vshs, float* __restrict__ vopac,
                                                           float* __restrict__ vscales, float4* __restrict__ vrots,
                                                           float* __restrict__ pose_part,
                                                           float* __restrict__ vcolors, gsr::TailState TS,
                                                           const float* __restrict__ opac,
                                                           const float* __restrict__ comp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    float poseR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, poset[3] = {0, 0, 0};
    // The radius, the geometry record and the Gaussian's own inputs are all requested at once (the record and the
    // inputs of a culled Gaussian are fetched for nothing: 104 bytes x 14 %); fetched one after the other — radius ->
    // record -> rows -> inputs -> SH — they would be five dependent round trips at 3 waves per SIMD.
    GsrGeoRec rec;
    rec.q0 = rec.q1 = rec.q2 = rec.q3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float p_in[3] = {0, 0, 0}, s_in[3] = {0, 0, 0};
    float4 q_in = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    int radius_in = 0;
    float o_in = 0.0f, rho_in = 0.0f;  // AA (comp[i] of a culled Gaussian is stale: read, never used)
    if (i < n) {
        radius_in = geom.radii[i];
        rec = geom.rec[i];
        // (FUSED: these arrays are updated in place by the epilogue — read through the same non-restrict pointers)
        const float* mp = FUSED ? TS.points : means;
        const float* sp = FUSED ? TS.scales_act : scales;
        const float4* qp = FUSED ? reinterpret_cast<const float4*>(TS.rots) : rots;
        p_in[0] = mp[3 * i]; p_in[1] = mp[3 * i + 1]; p_in[2] = mp[3 * i + 2];
        s_in[0] = sp[3 * i]; s_in[1] = sp[3 * i + 1]; s_in[2] = sp[3 * i + 2];
        q_in = qp[i];
        if constexpr (AA) {
            o_in = FUSED ? TS.opac_act[i] : opac[i];
            rho_in = comp[i];
        }
    }
    const bool visible = radius_in > 0;
    // 1. the summed gradient row
    float acc[16];
    sum_gradient_rows(i, visible, rec, geom, cam, inst, channels, acc);

    // FUSED: the gradients of this Gaussian stay here (zeros for a culled one)
    float f_vmean[3] = {0, 0, 0}, f_vs[3] = {0, 0, 0}, f_vq[4] = {0, 0, 0, 0}, f_vopac = 0.0f;
    float f_vc[3] = {0, 0, 0}, f_b[16];
    int f_nb = 0;  // SH bands carrying a gradient: 0 for a culled Gaussian
#pragma unroll
    for (int k = 0; k < 16; k++) f_b[k] = 0.0f;
    if (i < n) {
        if (!visible) {
            vmean2d_out[i] = make_float2(0.0f, 0.0f);
            if constexpr (!FUSED && !JAC) {
#pragma unroll
                for (int c = 0; c < 3; c++) { vmeans[3 * i + c] = 0.0f; vscales[3 * i + c] = 0.0f; }
                vrots[i] = make_float4(0, 0, 0, 0);
                vopac[i] = 0.0f;
                if (vcolors) { vcolors[3 * i] = 0.0f; vcolors[3 * i + 1] = 0.0f; vcolors[3 * i + 2] = 0.0f; }
                // (else: f_nb = 0 — the cooperative store below writes this Gaussian's zeros)
            }
        } else {
            const float4 a0 = make_float4(acc[0], acc[1], acc[2], acc[3]);
            const float4 a1 = make_float4(acc[4], acc[5], acc[6], acc[7]);
            const float2 vm2 = make_float2(acc[8], acc[9]);
            vmean2d_out[i] = vm2;  // gstate.∇means_2d, read by densification (strategy.jl:85-86)
            const float vo = AA ? a0.w * rho_in : a0.w, vrho = AA ? a0.w * o_in : 0.0f;
            if constexpr (FUSED) f_vopac = vo; else vopac[i] = vo;
            M33 R; float t[3];
            load_pose(cam, R, t);
            const float p[3] = {p_in[0], p_in[1], p_in[2]};
            const float4 q4 = q_in;
            const float s[3] = {s_in[0], s_in[1], s_in[2]};
            // 2. ∇project
            const ProjectBwd pb = project_bwd<AA>(cam, R, t, p, q4, s, rec, a1, vm2, rho_in, vrho, channels, pose_part != nullptr,
                                                  poseR, poset);
            // 3. the normal channel
            M33 vRg;
            normal_bwd(channels, acc, R, pb.Rg, s, pb.mc, vRg);
            // 4. ∇scales / ∇rotations
            // ∇quat_scale_to_cov (render.jl:302-320) + ∇unnorm_quat2rot (render.jl:335-366): in float64 from the raw inputs
            // (scales_rots_bwd_f64 above — the fp32 chain loses a needle's thin eigen-direction).  F32CHAIN keeps the
            // reference's fp32 expression trees (gsr_config.grad_precision = GSR_GRAD_FP32_REFERENCE).
            float vs[3], vq[4];
            if constexpr (!F32CHAIN) {
                scales_rots_bwd_f64<AA>(cam, R, t, p, q4, s, a1.x, a1.y, a1.z, vRg, rho_in, vrho, vs, vq);
            } else {
                // (inline, and pose partials below: as functions either takes instantiations of this kernel over their register
                //  ceilings — profiles/pergauss_stages/codegen_compare.txt)
                M33 S;
#pragma unroll
                for (int a = 0; a < 3; a++)
#pragma unroll
                    for (int b = 0; b < 3; b++) S.m[a][b] = 0.0f;
                S.m[0][0] = s[0]; S.m[1][1] = s[1]; S.m[2][2] = s[2];
                M33 vM = mul33(add33(pb.vSigma, tr33(pb.vSigma)), pb.M);
                M33 vRq = add33(mul33(vM, S), vRg);
#pragma unroll
                for (int c = 0; c < 3; c++)
                    vs[c] = pb.Rg.m[0][c] * vM.m[0][c] + pb.Rg.m[1][c] * vM.m[1][c] + pb.Rg.m[2][c] * vM.m[2][c];
                unnorm_quat2rot_bwd<float>(vRq.m, pb.qn, pb.inv_norm, vq);
            }
            if constexpr (FUSED) {
#pragma unroll
                for (int k = 0; k < 4; k++) f_vq[k] = vq[k];
#pragma unroll
                for (int c = 0; c < 3; c++) f_vs[c] = vs[c];
            } else {
                vrots[i] = make_float4(vq[0], vq[1], vq[2], vq[3]);
#pragma unroll
                for (int c = 0; c < 3; c++) vscales[3 * i + c] = vs[c];
            }

            // 5. ∇SH
            // coefficients of band k >= 1 (band 0 has no directional gradient)
            const float* sh = JAC ? shs + (size_t)9 * i : FUSED ? TS.rest + (size_t)3 * (K - 1) * i : shs + (size_t)3 * K * i + 3;
            const uint32_t clamp_bits = __float_as_uint(rec.q2.y);
            float vc[3] = {a0.x * (1.0f - (float)(clamp_bits & 1u)), a0.y * (1.0f - (float)((clamp_bits >> 1) & 1u)),
                           a0.z * (1.0f - (float)((clamp_bits >> 2) & 1u))};
            float b[16], vmsh[3];
            sh_bwd<DEG, JAC>(sh, p, cam, vc, b, vmsh);
            constexpr int NB = (DEG + 1) * (DEG + 1);
            if (!FUSED && vcolors) {
                // factored form for the multi-view exchange: ∇shs of a view is the outer product
                // basis(dir) x vc, so 3 floats per Gaussian travel instead of 3K (sh_grad_views_kernel
                // rebuilds Σ_views on every rank)
                vcolors[3 * i] = vc[0]; vcolors[3 * i + 1] = vc[1]; vcolors[3 * i + 2] = vc[2];
            } else {
                // ∇shs = basis x vc is stored (FUSED: applied) by the whole workgroup below (coalesced float4 rows instead
                // of 48 dword stores 192 bytes apart per lane)
                f_nb = NB;
#pragma unroll
                for (int c = 0; c < 3; c++) f_vc[c] = vc[c];
#pragma unroll
                for (int k = 0; k < NB; k++) f_b[k] = b[k];
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if constexpr (FUSED) f_vmean[c] = pb.vmean[c] + vmsh[c]; else vmeans[3 * i + c] = pb.vmean[c] + vmsh[c];
            }
        }
    }
    // 6. the epilogues: ∇shs stored (FUSED: the trainer tail applied) by the whole workgroup, then the pose partials
    store_or_apply_sh<FUSED, JAC>(i, n, K, vshs, vcolors, TS, f_b, f_vc, f_nb, f_vmean, f_vopac, f_vs, f_vq);
    if (pose_part) {  // projection.jl:243-256: thresholded per Gaussian, then summed
        // wave sum -> workgroup sum in LDS -> the workgroup's 12 partials (∇R column-major, ∇t) to ITS slot of pose_part, zeros
        // included (the scratch needs no clearing); pose_final_kernel adds the slots in a fixed order — float atomics onto the 12
        // shared destinations would add in arrival order, and three workgroups already give run-to-run different last bits
        __shared__ float pose_red[4][12];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            float v = k < 9 ? poseR[k] : poset[k - 9];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if ((threadIdx.x & 63) == 0) pose_red[threadIdx.x >> 6][k] = v;
        }
        __syncthreads();
        if (threadIdx.x < 12) {
            const int k = threadIdx.x;
            pose_part[(size_t)blockIdx.x * 12 + k] = pose_red[0][k] + pose_red[1][k] + pose_red[2][k] + pose_red[3][k];
        }
    }
}

// ∇R (9 floats, column-major) and ∇t (3) from the per-workgroup partials of pergauss_bwd_kernel (12 floats per workgroup), summed
// in double in an order that depends on n_part alone: ONE workgroup, thread t takes the partials t, t + 256, ... in ascending
// order, then the 256 thread sums are added in thread order.  Writes (not accumulates into) vR / vt.
__global__ __launch_bounds__(256) void pose_final_kernel(int n_part, const float* __restrict__ part, float* __restrict__ vR,
                                                         float* __restrict__ vt) {
    __shared__ double red[12][256];
    double s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = 0.0;
    for (int i = threadIdx.x; i < n_part; i += 256)
#pragma unroll
        for (int k = 0; k < 12; k++) s[k] += (double)part[(size_t)i * 12 + k];
#pragma unroll
    for (int k = 0; k < 12; k++) red[k][threadIdx.x] = s[k];
    __syncthreads();
    if (threadIdx.x >= 12) return;
    const int k = threadIdx.x;
    double t = 0.0;
    for (int i = 0; i < 256; i++) t += red[k][i];
    if (k < 9) vR[k] = (float)t; else vt[k - 9] = (float)t;
}

// _update_stats! (src/strategy.jl:118-136): densification statistics from the side outputs of
// the last forward/backward pair (radii, ∇means_2d).
__global__ __launch_bounds__(256) void update_stats_kernel(int n, const int32_t* __restrict__ radii,
                                                           const float2* __restrict__ vmean2d, float res_x,
                                                           float res_y, int32_t* __restrict__ max_radii,
                                                           float* __restrict__ accum, float* __restrict__ denom) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = radii[i];
    if (!(r > 0)) return;
    max_radii[i] = max(max_radii[i], r);
    const float2 g = vmean2d[i];
    const float gx = g.x * res_x * 0.5f, gy = g.y * res_y * 0.5f;
    accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.0f;
}

}  // namespace

void gsr_launch_update_stats(hipStream_t s, int n, const int32_t* radii, const float2* vmean2d, int width, int height,
                             int32_t* max_radii, float* accum, float* denom) {
    if (n <= 0) return;
    hipLaunchKernelGGL(update_stats_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, radii, vmean2d, (float)width,
                       (float)height, max_radii, accum, denom);
}

void gsr_launch_pergauss_bwd(hipStream_t s, int n, int K, int degree, int channels, const float* means,
                             const float* scales, const float* rots, const float* shs, GsrCam cam, GsrGeom geom,
                             GsrInst inst, float2* vmean2d, float* vmeans, float* vshs, float* vopac,
                             float* vscales, float* vrots, float* vR, float* vt, float* pose_part, float* vcolors,
                             bool fp32_chain, const float* opac, const float* comp, const float* sh_jac) {
    if (n <= 0) return;
    dim3 grid((n + 255) / 256), block(256);
    const float4* r4 = reinterpret_cast<const float4*>(rots);
    float4* vr4 = reinterpret_cast<float4*>(vrots);
    const gsr::TailState none{};
    dispatch_degree(degree, [&](auto d) {
        constexpr int DEG = d;
        dispatch_bool(fp32_chain, [&](auto f) {
            constexpr bool F32 = f;
            dispatch_bool(comp != nullptr, [&](auto a) {
                constexpr bool AA = a;
                // sh_jac: the composite_bwd launch before this one carried the row-independent job (default precision, ∇shs
                // in full): the Jacobian buffer takes the place of `shs`
                if constexpr (!F32) {
                    if (sh_jac && !vcolors) {
                        hipLaunchKernelGGL((pergauss_bwd_kernel<DEG, false, false, AA, true>), grid, block, 0, s, n, K, channels, means,
                                           scales, r4, sh_jac, cam, geom, inst, vmean2d, vmeans, vshs, vopac, vscales, vr4,
                                           vR ? pose_part : nullptr, vcolors, none, opac, comp);
                        return;
                    }
                }
                hipLaunchKernelGGL((pergauss_bwd_kernel<DEG, false, F32, AA>), grid, block, 0, s, n, K, channels, means, scales,
                                   r4, shs, cam, geom, inst, vmean2d, vmeans, vshs, vopac, vscales, vr4,
                                   vR ? pose_part : nullptr, vcolors, none, opac, comp);
            });
        });
    });
    if (vR) hipLaunchKernelGGL(pose_final_kernel, dim3(1), dim3(256), 0, s, (int)grid.x, pose_part, vR, vt);
}

void gsr_launch_pergauss_bwd_tail(hipStream_t s, int n, int K, int degree, int channels, GsrCam cam, GsrGeom geom,
                                  GsrInst inst, float2* vmean2d, const gsr::TailState& S, bool fp32_chain, const float* comp) {
    if (n <= 0) return;
    dim3 grid((n + 255) / 256), block(256);
    const float4* r4 = reinterpret_cast<const float4*>(S.rots);
    float* const no_f = nullptr;
    dispatch_degree(degree, [&](auto d) {
        constexpr int DEG = d;
        dispatch_bool(fp32_chain, [&](auto f) {
            constexpr bool F32 = f;
            dispatch_bool(comp != nullptr, [&](auto a) {
                constexpr bool AA = a;
                hipLaunchKernelGGL((pergauss_bwd_kernel<DEG, true, F32, AA>), grid, block, 0, s, n, K, channels, S.points,
                                   S.scales_act, r4, (const float*)nullptr, cam, geom, inst, vmean2d, no_f, no_f, no_f, no_f,
                                   (float4*)nullptr, no_f, no_f, S, (const float*)nullptr, comp);
            });
        });
    });
}
