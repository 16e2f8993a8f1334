// Small-matrix and SH helpers of the per-Gaussian kernels, device-only: what preprocess.hip (the forward of a view),
// pergauss.hip (its backward) and sh_views.hip (the multi-view SH sums) all evaluate, in ONE definition each, so that the
// backward recomputes the forward's floats bit for bit.  A helper only one of them uses lives in that file.
//
// Reference behaviour: src/rasterization/render.jl:288-333 (quat2rot, the 3-D covariance), projection.jl:14-27 (the normal),
// 259-287 (the perspective terms), spherical_harmonics.jl:41-74 (the view direction and the basis).
//
// Every translation unit that includes this is compiled with -ffp-contract=off: each fp32 expression is evaluated as
// written (no FMA), which is what makes the floats the same on both sides and against the CPU oracle.
//
// bench.py's hashes of the kernel sources, which mark profiles/pmc_traffic.json stale, cover pergauss.hip and not this
// file: after a change here, run tools/measure_pmc.sh again.
#pragma once
#include "gsr_kernels.h"

namespace gsr::splat {

constexpr float SH0 = 0.28209479177387814f;
constexpr float SH1 = 0.4886025119029199f;
constexpr float SH2C1 = 1.0925484305920792f;
constexpr float SH2C2 = -1.0925484305920792f;
constexpr float SH2C3 = 0.31539156525252005f;
constexpr float SH2C4 = -1.0925484305920792f;
constexpr float SH2C5 = 0.5462742152960396f;
constexpr float SH3C1 = -0.5900435899266435f;
constexpr float SH3C2 = 2.890611442640554f;
constexpr float SH3C3 = -0.4570457994644658f;
constexpr float SH3C4 = 0.3731763325901154f;
constexpr float SH3C5 = -0.4570457994644658f;
constexpr float SH3C6 = 1.445305721320277f;
constexpr float SH3C7 = -0.5900435899266435f;

struct M33 { float m[3][3]; };
struct M22 { float m[2][2]; };

__device__ __forceinline__ M33 mul33(const M33& a, const M33& b) {
    M33 o;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) o.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return o;
}
__device__ __forceinline__ M33 tr33(const M33& a) {
    M33 o;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) o.m[i][j] = a.m[j][i];
    return o;
}

// world->camera rotation as row-major M33, honouring the device override (pose optimisation)
__device__ __forceinline__ void load_pose(const GsrCam& cam, M33& R, float t[3]) {
    // element-wise selects (a branch over two whole-array initialisations makes the optimiser
    // keep the pose in scratch memory)
    const bool dev = cam.R_dev != nullptr;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float host = cam.R[r * 3 + c];
            R.m[r][c] = dev ? cam.R_dev[c * 3 + r] : host;
        }
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = cam.t_dev ? cam.t_dev[k] : cam.t[k];
}

// render.jl:322-333
__device__ __forceinline__ M33 quat2rot(const float4 q4, float qn[4], float& inv_norm) {
    float n2 = q4.x * q4.x + q4.y * q4.y + q4.z * q4.z + q4.w * q4.w;
    inv_norm = 1.0f / sqrtf(n2);
    float w = q4.x * inv_norm, x = q4.y * inv_norm, y = q4.z * inv_norm, z = q4.w * inv_norm;
    qn[0] = w; qn[1] = x; qn[2] = y; qn[3] = z;
    float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    M33 R;
    R.m[0][0] = 1.0f - 2.0f * (y2 + z2); R.m[1][0] = 2.0f * (xy + wz); R.m[2][0] = 2.0f * (xz - wy);
    R.m[0][1] = 2.0f * (xy - wz); R.m[1][1] = 1.0f - 2.0f * (x2 + z2); R.m[2][1] = 2.0f * (yz + wx);
    R.m[0][2] = 2.0f * (xz + wy); R.m[1][2] = 2.0f * (yz - wx); R.m[2][2] = 1.0f - 2.0f * (x2 + y2);
    return R;
}

// render.jl:291-294
__device__ __forceinline__ M33 cov3d(const M33& Rg, const float s[3], M33& M) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M.m[r][c] = Rg.m[r][c] * s[c];
    return mul33(M, tr33(M));
}

struct Persp {
    float lim[2], lim_neg[2], txy[2], rz;
    float J[2][3];
};
// shared part of projection.jl:259-287 / 289-353
__device__ __forceinline__ Persp persp_common(const float mc[3], const GsrCam& cam) {
    Persp p;
    const int res[2] = {cam.width, cam.height};
    p.rz = 1.0f / mc[2];
    float rz2 = p.rz * p.rz;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        float tan_fov = (0.5f * (float)res[k]) / cam.focal[k];
        float stf = 0.3f * tan_fov;
        float pp = cam.principal[k] * (float)res[k];
        p.lim[k] = ((float)res[k] - pp) / cam.focal[k] + stf;
        p.lim_neg[k] = pp / cam.focal[k] + stf;
        float v = mc[k] * p.rz;
        float c = fmaxf(-p.lim_neg[k], v);
        c = fminf(p.lim[k], c);
        p.txy[k] = mc[2] * c;
    }
    p.J[0][0] = cam.focal[0] * p.rz; p.J[1][0] = 0.0f;
    p.J[0][1] = 0.0f;                p.J[1][1] = cam.focal[1] * p.rz;
    p.J[0][2] = -cam.focal[0] * p.txy[0] * rz2;
    p.J[1][2] = -cam.focal[1] * p.txy[1] * rz2;
    return p;
}


template <int DEG>
__device__ __forceinline__ void sh_basis(const float d[3], float b[16]) {
    float x = d[0], y = d[1], z = d[2];
    b[0] = SH0;
    if (DEG > 0) {
        b[1] = -SH1 * y; b[2] = SH1 * z; b[3] = -SH1 * x;
    }
    if (DEG > 1) {
        float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z;
        b[4] = SH2C1 * xy; b[5] = SH2C2 * yz; b[6] = SH2C3 * (2.0f * z2 - x2 - y2);
        b[7] = SH2C4 * xz; b[8] = SH2C5 * (x2 - y2);
        if (DEG > 2) {
            b[9] = SH3C1 * y * (3.0f * x2 - y2);
            b[10] = SH3C2 * xy * z;
            b[11] = SH3C3 * y * (4.0f * z2 - x2 - y2);
            b[12] = SH3C4 * z * (2.0f * z2 - 3.0f * x2 - 3.0f * y2);
            b[13] = SH3C5 * x * (4.0f * z2 - x2 - y2);
            b[14] = SH3C6 * z * (x2 - y2);
            b[15] = SH3C7 * x * (x2 - 3.0f * y2);
        }
    }
}

// projection.jl:14-27
__device__ __forceinline__ void gaussian_normal(const M33& Rw, const M33& Rg, const float s[3], const float mc[3],
                                                float n[3], int& k, float& sign) {
    k = (s[0] <= s[1] && s[0] <= s[2]) ? 0 : (s[1] <= s[2]) ? 1 : 2;
    // (arithmetic select: a ?: chain over Rg.m[r][k] is turned back into a dynamically indexed
    // load by the optimiser, which puts Rg in scratch)
    const float m0 = k == 0 ? 1.0f : 0.0f, m1 = k == 1 ? 1.0f : 0.0f, m2 = k == 2 ? 1.0f : 0.0f;
    float ax[3];
#pragma unroll
    for (int r = 0; r < 3; r++) ax[r] = m0 * Rg.m[r][0] + m1 * Rg.m[r][1] + m2 * Rg.m[r][2];
    float nc[3];
#pragma unroll
    for (int r = 0; r < 3; r++) nc[r] = Rw.m[r][0] * ax[0] + Rw.m[r][1] * ax[1] + Rw.m[r][2] * ax[2];
    float d = nc[0] * mc[0] + nc[1] * mc[1] + nc[2] * mc[2];
    sign = d > 0.0f ? -1.0f : 1.0f;
#pragma unroll
    for (int r = 0; r < 3; r++) n[r] = sign * nc[r];
}

// The view direction of the SH stages (spherical_harmonics.jl:41-48): d0 = p - center, dir = d0 / |d0|.  The one definition
// for preprocess, the per-Gaussian backward (which also pulls back through the normalisation: it keeps d0) and the two
// multi-view SH kernels.
__device__ __forceinline__ void view_dir(const float p[3], const float* center, float d0[3], float dir[3]) {
    d0[0] = p[0] - center[0]; d0[1] = p[1] - center[1]; d0[2] = p[2] - center[2];
    const float inv = 1.0f / sqrtf(d0[0] * d0[0] + d0[1] * d0[1] + d0[2] * d0[2]);
    dir[0] = d0[0] * inv; dir[1] = d0[1] * inv; dir[2] = d0[2] * inv;
}

// The direction Jacobian of the SH colour before the clamp (spherical_harmonics.jl:76-172): dcx[c], dcy[c], dcz[c] =
// d rgb_c / d dir_x, _y, _z.  sh = the coefficients of band 1 on (3 floats per band; band 0 has no directional gradient).
// It depends on nothing the compositing backward produces: the per-Gaussian backward evaluates it in place, or reads the nine
// floats the row-independent job of composite_bwd's launch left for it (bwd_row_job.h) — one definition, the same bits.
template <int DEG>
__device__ __forceinline__ void sh_dir_jacobian(const float* sh, const float dir[3], float dcx[3], float dcy[3], float dcz[3]) {
    auto coeff = [&](int k, int c) { return sh[3 * (k - 1) + c]; };  // band k >= 1, channel c
#pragma unroll
    for (int c = 0; c < 3; c++) { dcx[c] = 0.0f; dcy[c] = 0.0f; dcz[c] = 0.0f; }
    if (DEG > 0) {
        const float x = dir[0], y = dir[1], z = dir[2];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            dcx[c] = -SH1 * coeff(3, c); dcy[c] = -SH1 * coeff(1, c); dcz[c] = SH1 * coeff(2, c);
        }
        if (DEG > 1) {
            float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                dcx[c] = dcx[c] + SH2C1 * y * coeff(4, c) + SH2C3 * 2.0f * -x * coeff(6, c) +
                         SH2C4 * z * coeff(7, c) + SH2C5 * 2.0f * x * coeff(8, c);
                dcy[c] = dcy[c] + SH2C1 * x * coeff(4, c) + SH2C2 * z * coeff(5, c) +
                         SH2C3 * 2.0f * -y * coeff(6, c) + SH2C5 * 2.0f * -y * coeff(8, c);
                dcz[c] = dcz[c] + SH2C2 * y * coeff(5, c) + SH2C3 * 4.0f * z * coeff(6, c) +
                         SH2C4 * x * coeff(7, c);
            }
            if (DEG > 2) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    dcx[c] = dcx[c] + SH3C1 * coeff(9, c) * 3.0f * 2.0f * xy + SH3C2 * coeff(10, c) * yz +
                             SH3C3 * coeff(11, c) * -2.0f * xy + SH3C4 * coeff(12, c) * -3.0f * 2.0f * xz +
                             SH3C5 * coeff(13, c) * (-3.0f * x2 + 4.0f * z2 - y2) +
                             SH3C6 * coeff(14, c) * 2.0f * xz + SH3C7 * coeff(15, c) * 3.0f * (x2 - y2);
                    dcy[c] = dcy[c] + SH3C1 * coeff(9, c) * 3.0f * (x2 - y2) + SH3C2 * coeff(10, c) * xz +
                             SH3C3 * coeff(11, c) * (-3.0f * y2 + 4.0f * z2 - x2) +
                             SH3C4 * coeff(12, c) * -3.0f * 2.0f * yz + SH3C5 * coeff(13, c) * -2.0f * xy +
                             SH3C6 * coeff(14, c) * -2.0f * yz + SH3C7 * coeff(15, c) * -3.0f * 2.0f * xy;
                    dcz[c] = dcz[c] + SH3C2 * coeff(10, c) * xy + SH3C3 * coeff(11, c) * 4.0f * 2.0f * yz +
                             SH3C4 * coeff(12, c) * 3.0f * (2.0f * z2 - x2 - y2) +
                             SH3C5 * coeff(13, c) * 4.0f * 2.0f * xz + SH3C6 * coeff(14, c) * (x2 - y2);
                }
            }
        }
    }
}

}  // namespace gsr::splat
