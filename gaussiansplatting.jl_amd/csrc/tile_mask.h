// Opacity-aware footprint test shared by the binning kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Conservative footprint masks of an instance inside its 16x16 tile.
//   bits 0..15  row mask: bit r is set unless NO pixel of row r of the tile can pass the kernels' blend test
//               bits(sigma) < X (blend_threshold_bits below: alpha >= 1/255, render.jl:95);
//   bits 16..19 quadrant mask: bit 16 + 2*qy + qx for the 8x8 quadrant (qx, qy): some row of the quadrant's eight can pass
//               the test inside the quadrant's eight columns.
// The composite kernels use them only to skip work; every surviving (pixel, splat) pair still
// runs the exact test, so the slack below never changes a result.
//
// A row is tested once per half (dx = mx - px: left half [mx - X0 - 7, mx - X0], right half [mx - X0 - 15, mx - X0 - 8]):
// sigma is a convex parabola in dx, so its minimum over a column range sits at the vertex -(b/a)·dy clamped to the range,
// and the half is flagged when that minimum is at most the threshold,
//     s = sigma(x*, dy) - ts < 0,    x* = med3(-(b/a)·dy, lo, hi),    ts = S + 2e-3 + 4e-6·M,    S = float(X - 1):
// S is the largest sigma that passes the test, and M = ha·Xm² + |b|·Xm·Ym + hc·Ym² (Xm, Ym: the largest |dx|, |dy| of the
// tile's pixel centres) bounds every term of either evaluation of sigma — fp32 leaves a few ulps (6e-8) of it in the kernels'
// sigma and in s.  An error d of the vertex (the hardware reciprocal's ulp) moves the minimum by a·d²/2: second order.
// No sqrt, no compare, no select and no branch per row: mul / fma / v_med3_f32, and the sign bit of s shifted into the
// half's 16-bit mask by one v_alignbit_b32 (rows walked 15 -> 0; a row the parabola misses shifts in a 0).
__device__ __forceinline__ uint32_t instance_row_mask(const float4 g0, const float4 g1, uint32_t X, int X0, int Y0) {
    const float mx = g0.x, my = g0.y, a = g0.z, b = g0.w, c = g1.x;
    const float ha = 0.5f * a, hc = 0.5f * c;
    const float l_hi = mx - (float)X0, l_lo = mx - (float)(X0 + 7);         // the kernels' own dx at the halves' end columns
    const float r_hi = mx - (float)(X0 + 8), r_lo = mx - (float)(X0 + 15);
    const float dy0 = my - (float)Y0;
    const float xm = fmaxf(fabsf(l_hi), fabsf(r_lo)), ym = fmaxf(fabsf(dy0), fabsf(dy0 - 15.0f));
    const float M = ha * (xm * xm) + fabsf(b) * (xm * ym) + hc * (ym * ym);
    const float ts = __uint_as_float(X - 1u) + 2e-3f + 4e-6f * M;
    const float nboa = -b * __builtin_amdgcn_rcpf(a);
    uint32_t ml = 0, mr = 0;
#pragma unroll
    for (int r = 15; r >= 0; r--) {
        const float dy = dy0 - (float)r;
        const float v = nboa * dy, bdy = b * dy;
        const float k = __fmaf_rn(dy, hc * dy, -ts);
        const float xl = __builtin_amdgcn_fmed3f(v, l_lo, l_hi), xr = __builtin_amdgcn_fmed3f(v, r_lo, r_hi);
        const float sl = __fmaf_rn(xl, __fmaf_rn(ha, xl, bdy), k), sr = __fmaf_rn(xr, __fmaf_rn(ha, xr, bdy), k);
        ml = __builtin_amdgcn_alignbit(ml, __float_as_uint(sl), 31);  // (ml << 1) | sign(sl)
        mr = __builtin_amdgcn_alignbit(mr, __float_as_uint(sr), 31);
    }
    uint32_t m = (ml | mr) | ((ml & 0xFFu) ? 1u << 16 : 0u) | ((mr & 0xFFu) ? 1u << 17 : 0u) |
                 ((ml & 0xFF00u) ? 1u << 18 : 0u) | ((mr & 0xFF00u) ? 1u << 19 : 0u);
    if (!(a > 0.0f)) m = 0xFFFFFu;  // degenerate conic: no culling
    if (X == 0u) m = 0u;            // not even sigma = +0 passes (opacity < 1/255): never blended
    return m;
}


// Cheap per-tile version for the count / scatter loops: does the ellipse {sigma <= tau}
// reach the box of the tile's pixel centres?  sigma is a convex quadratic, so its minimum
// over the box is 0 if the mean lies inside and otherwise sits on one of the four edges
// (a clamped 1-D parabola each).  Conservative (the box also contains the points between
// pixel centres); tau = ln(255*opacity) + slack is hoisted per Gaussian by the caller.
// The blend test of a (pixel, splat) pair — sigma >= 0 && min(0.99, o·exp(-sigma)) >= 1/255 (render.jl:92-95) — as ONE
// unsigned compare per pair: the predicate is monotone in sigma, non-negative floats order like their bit patterns and any
// negative sigma has the sign bit set, so with  S = the largest sigma for which the reference's own expression passes,
//     bits(sigma) < X,   X = bits(S) + 1   (0 when not even sigma = +0 passes: opacity below 1/255, NaN)
// is the whole test.  S is found ONCE PER GAUSSIAN (preprocess; carried in the geometry record) by bisection over bit
// patterns around ln(255·o), evaluating the reference's expression with a correctly rounded exp (through fp64): the decision
// for every pair is then exactly "fl(o · fl(exp(-sigma))) >= fl(1/255)", not an approximation of it by a rounded logarithm
// or a 1-ulp exp (either flips pairs within an ulp of the boundary against the oracle: 1 scene in 400, then 3 in 1600 of
// tools/fuzz_parity.py had one gradient beyond tolerance).
__device__ __forceinline__ uint32_t blend_threshold_bits(float o) {
    const float amin = 1.0f / 255.0f;
    // (exp through fp64: the correctly rounded fp32 value — the CPU oracle's libm expf is that in 99.6 % of its results)
    auto pass = [&](uint32_t b) { return fminf(0.99f, __fmul_rn(o, (float)exp(-(double)__uint_as_float(b)))) >= amin; };
    if (!pass(0u)) return 0u;
    const float tau = fmaxf(logf(255.0f * o), 0.0f);
    const float w = 4e-7f * fmaxf(tau, 1.0f);  // > the shift a 1-ulp exp and a 1-ulp log can cause, absolute
    uint32_t lo = __float_as_uint(fmaxf(tau - w, 0.0f)), hi = __float_as_uint(tau + w);
    if (!pass(lo)) lo = 0u;
    for (int k = 0; k < 24 && pass(hi); k++) { lo = hi; hi = __float_as_uint(__uint_as_float(hi) + w * (float)(2 << k)); }
    if (pass(hi)) return hi + 1u;  // (unreachable: sigma = tau + 6.7 passes for no opacity <= 1)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (pass(mid)) lo = mid; else hi = mid;
    }
    return lo + 1u;
}

__device__ __forceinline__ float footprint_tau(float opacity) { return __logf(255.0f * opacity) + 2e-3f; }

__device__ __forceinline__ bool tile_may_touch(float mx, float my, float a, float b, float c, float tau, int X0,
                                               int Y0) {
    if (!(tau >= 0.0f)) return false;
    if (!(a > 0.0f) || !(c > 0.0f)) return true;
    const float x_lo = mx - (float)(X0 + 15), x_hi = mx - (float)X0;  // dx = mx - px
    const float y_lo = my - (float)(Y0 + 15), y_hi = my - (float)Y0;
    if (x_lo <= 0.0f && x_hi >= 0.0f && y_lo <= 0.0f && y_hi >= 0.0f) return true;
    const float inv_a = 1.0f / a, inv_c = 1.0f / c;
    float best = 3.0e38f;
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const float dx = e ? x_hi : x_lo;  // vertical edges: minimise over dy
        float dy = fminf(y_hi, fmaxf(y_lo, -b * dx * inv_c));
        best = fminf(best, b * dx * dy + 0.5f * (a * dx * dx + c * dy * dy));
        const float ey = e ? y_hi : y_lo;  // horizontal edges: minimise over dx
        float ex = fminf(x_hi, fmaxf(x_lo, -b * ey * inv_a));
        best = fminf(best, b * ex * ey + 0.5f * (a * ex * ex + c * ey * ey));
    }
    return best <= tau + 1e-3f * (1.0f + fabsf(best));
}
