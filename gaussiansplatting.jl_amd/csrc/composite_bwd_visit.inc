// One staged instance visited by one wave: the four pixel groups of its lanes, back to front.  Text of the instance loops of
// composite_bwd_body.inc (the tile walk: composite_bwd_kernel, composite_bwd_kernel_rgb_bg0) and of PASS 2 of
// composite_bwd_long_kernel (the segment walk), included inside `while (wl) { ... }` with these names in scope:
//   C, VC, BG0, ACC, FY_REBUILD, PPL, ROWS, ST, BB       compile-time (the segment walk: VC = C, ACC = FY_REBUILD = false)
//   j, contributor      the instance's LDS slot and its 0-based list position (wave-uniform)
//   l0, l1, l2, l3      the staged batch (bwd_stage_entry);  fx, wave;  fy, T, A, bgT, vp, last_contributor (composite_bwd_state.inc)
//   my, touched         the wave's accumulator slab and the mask of its rows that hold sums
// It leaves the decoded entry (composite_bwd_decode.inc), the lane's partial sums P, U1, U2, col[VC], and jrow / my_row (the
// instance's slab row) to the reduction that follows — composite_bwd_reduce.inc, or the tile walk's PAIR block — and `continue`s
// past it when no pixel of the wave blends the instance.  (Text, not a function: see composite_bwd_body.inc.)  bench.py's hashes
// of the kernel sources, which mark profiles/pmc_traffic.json stale, cover composite.hip and not this file: after a change here,
// run tools/measure_pmc.sh again.
#include "composite_bwd_decode.inc"
    // A lane accumulates only  P = Σ G·vα,  U1 = Σ G·vα·dy,  U2 = Σ G·vα·dy²  and the
    // feature sums.  The conic / mean2d gradients (render.jl:262-272) are linear in
    // {dx²·P, dx·U1, U2, dx·P, U1}: those five are what the wave reduces, and the
    // per-instance flush applies the wave-uniform factors (-o/2, conic) once per row.
    float P = 0.0f, U1 = 0.0f, U2 = 0.0f, col[VC];
#pragma unroll
    for (int c = 0; c < VC; c++) col[c] = 0.0f;
    unsigned long long any_active = 0ull;
    const uint32_t rowbits = entry_rowbits >> (ROWS * wave);
    // The footprint bits of the four pixel groups (readfirstlane of the already-uniform bits: tells the compiler that the
    // group skip below, and everything that merges behind it — the ballot accumulator —, is scalar; without it the test and
    // `any_active` were VALU).  All four HERE, in the block that reads the mask: there the readfirstlane folds into an
    // s_and; written at the skip itself, the ones of groups 2 and 3 sat in later blocks and stayed instructions — the
    // mask copied to a VGPR and read back, 3 VALU instructions per instance (composite_bwd 669 -> 648 us, DESIGN.md §4.1).
    int group_bits[PPL];
#pragma unroll
    for (int q = 0; q < PPL; q++) group_bits[q] = __builtin_amdgcn_readfirstlane((int)((rowbits >> (4 * q)) & 0xFu));
#pragma unroll
    for (int q = 0; q < PPL; q++) {
        if (group_bits[q] == 0) continue;  // pixel rows 4q..4q+3 of this wave: untouched by the footprint -> wave-uniform skip
        const float fyq = FY_REBUILD ? fy[0] + (float)(4 * q) : fy[FY_REBUILD ? 0 : q];
        const float dy = a.y - fyq, dy2 = __fmul_rn(dy, dy);
        const float sigma = sigma_of(sx, b.x, dy, dy2);
        // the blend test is one unsigned compare of sigma against the instance's threshold; exp and alpha are only
        // computed for the lanes that pass (they run under EXEC = active)
        const bool c_live = contributor < last_contributor[q];
        const bool c_touch = __float_as_uint(sigma) < thr_bits;
        const bool active = c_live && c_touch;
        // ballots of the bare compares are their SGPR masks; the AND/OR runs on the scalar unit
        any_active |= wave_ballot(c_live) & wave_ballot(c_touch);
        if (active) {
            const float G = bwd_exp_neg<ACC>(sigma);
            const float alpha = alpha_of(o, G);
            // T /= (1-α) and -T_final/(1-α) (render.jl:237,259) share one hardware reciprocal
            const float rinv = bwd_rcp<ACC>(1.0f - alpha);
            T[q] = T[q] * rinv;
            const float fac = alpha * T[q];
            float cv = f[0] * vp[q][0];
#pragma unroll
            for (int c = 1; c < VC; c++) cv += f[c] * vp[q][c];
            const float d = cv - A[q];                 // (color - accum_rec)·v
            const float valpha = BG0 ? d * T[q] : d * T[q] + bgT[BG0 ? 0 : q] * rinv;
            A[q] = A[q] + alpha * d;                   // α·cv + (1-α)·A for the next (nearer) splat
            const float t = G * valpha;
            P += t;
            U1 += t * dy;
            U2 += t * dy2;
#pragma unroll
            for (int c = 0; c < VC; c++) col[c] += fac * vp[q][c];
        }
    }
    if (any_active == 0ull) continue;  // wave-uniform: none of this wave's pixels is touched
    // row of this splat in the wave's accumulator slab: j is wave-uniform, the multiply belongs on the scalar
    // unit (left to itself the compiler folds `j * ST + slot` into a quarter-rate v_mad_u64_u32 per store)
    int jrow;
    asm("s_mul_i32 %0, %1, %2" : "=s"(jrow) : "s"(j), "n"(ST));
    float* const my_row = my + jrow;
#pragma unroll
    for (int w = 0; w < BB / 64; w++)
        if ((j >> 6) == w) touched[w] |= 1ull << (j & 63);
