// The state a lane's four pixels (px, py0 + 4q) start a backward walk from.  Text of composite_bwd_body.inc (the tile walk) and of
// composite_bwd_long_kernel (the segment walk, both passes), included after the declarations
//   float fy[FY_REBUILD ? 1 : PPL], T[PPL], A[PPL], bgT[BG0 ? 1 : PPL], vp[PPL][VC];  int last_contributor[PPL];
// with C, VC, BG0, FY_REBUILD, PPL, px, py0 and the kernel's arguments W, H, bg, vpixels, n_contrib, final_T in scope.  Fills them
// and leaves `deepest`, the deepest list position any of the four pixels blended.  (Text, not a function: as a function the
// guarded loads of a pixel are merged, which changes every kernel that includes it — profiles/bwd_shared_visit/codegen_compare.txt.)
// bench.py's hashes of the kernel sources, which mark profiles/pmc_traffic.json stale, cover composite.hip and not this file:
// after a change here, run tools/measure_pmc.sh again.
    int deepest = 0;
#pragma unroll
    for (int q = 0; q < PPL; q++) {
        const int py = py0 + 4 * q;
        const bool inside = px < W && py < H;
        const size_t pi = (size_t)px + (size_t)W * py;
        if (!FY_REBUILD || q == 0) fy[FY_REBUILD ? 0 : q] = (float)py;
        const float T_final = inside ? final_T[pi] : 0.0f;
        T[q] = T_final;
        last_contributor[q] = inside ? (int)n_contrib[pi] : 0;
        float bg_dot = 0.0f;
#pragma unroll
        for (int c = 0; c < VC; c++) {
            vp[q][c] = inside ? vpixels[(size_t)C * pi + c] : 0.0f;
            bg_dot += bg.v[c] * vp[q][c];
        }
        if (!BG0) bgT[BG0 ? 0 : q] = -T_final * bg_dot;
        // The reference carries accum_rec[c], last_color[c], last_alpha per channel and forms
        //   vα = Σ_c (color[c] - accum_rec[c])·v[c]            (render.jl:245-252).
        // Only the dot product with the pixel cotangent is ever used, so the state is folded to
        // one scalar A = accum_rec·v with the same recurrence  A' = α·(color·v) + (1-α)·A.
        A[q] = 0.0f;
        deepest = max(deepest, last_contributor[q]);
    }
