// The body of composite_bwd_kernel<C, BG0, VC, ACC> and of composite_bwd_kernel_rgb_bg0 (composite.hip): included inside each, with
// C, BG0, VC, ACC and the kernels' arguments in scope.  (Text, not a function: as a __device__ function template the same lines
// compile with one VGPR more in the six VC == C > 3 instantiations.)  bench.py's hashes of the kernel sources, which mark
// profiles/pmc_traffic.json stale, cover composite.hip and not this file: after a change here, run tools/measure_pmc.sh again.
    static_assert(VC == C || VC == 3, "all channels, or colour only");
    constexpr int NA = AccRow<VC>::N, ST = AccRow<VC>::STRIDE;
    // one wave64 per tile, four pixels per lane, 64 splats staged per batch.  (The wave index, the per-wave slab and mask
    // and the batch loop over 64-entry ballots stay written out for a general NW: folding NW = 1 into them changes the
    // register allocation of every instantiation, one to two VGPRs, and :rgb's would cross from six to seven waves.)
    constexpr int PPL = 4, BB = 64, NT = 64, NW = NT / 64, ROWS = 4 * PPL;
    __shared__ float4 l0[BB], l1[BB], l2[BB];
    __shared__ float4 l3[C > 3 ? BB : 1];
    // One accumulator slab per wave: a wave stores its reduced partials with plain ds_write
    // (no LDS atomics: hipcc wraps those in a per-lane "atomic optimizer" loop), and a
    // per-wave bit mask records which rows it touched so nothing has to be zero-filled.
    __shared__ float lacc[NW][BB * ST];
    __shared__ unsigned long long lmask[NW][BB / 64];
    __shared__ int tile_last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t strip_bits = ((1u << ROWS) - 1u) << (ROWS * wave);  // this wave's pixel rows
    const gsr::LaneBits lane_bits(lane);
    const int red_slot = gsr::wave_reduce_index<NA>(lane);  // which partial this lane ends up holding
    const bool red_writer = gsr::wave_reduce_writer(lane);
    const gsr::RowColConsts rowcol(lane);
    const gsr::RowColConstsD rowcol_d(lane);
    // :rgb's zero-background kernel reduces its instances two at a time (wave_reduce.h: nine swaps and one 16-lane tail for
    // twelve sums); the four registers the waiting instance takes are the ones BG0 frees
    constexpr bool PAIR = C == 3 && BG0 && !ACC;
    const gsr::RowColConstsPair rowcol_pair(lane);
    const int tile = (int)tile_order[blockIdx.x];  // 1-D grid in launch order, longest lists first
    const int tile_x = tile % grid_x, tile_y = tile / grid_x;
    const int px = tile_x * GSR_TILE + (lane & 15);
    const int py0 = tile_y * GSR_TILE + ROWS * wave + (lane >> 4);
    const float fx = (float)px;
    const uint32_t start = tile_start[tile], end = tile_start[tile + 1];
    if (end == start) return;
    if (end - start > tiers.split_len) return;  // composite_bwd_long_kernel owns this tile

    // per-pixel state (rows py0, py0 + 4, py0 + 8, py0 + 12)
    // (:rgbdn: the rows' y coordinates are rebuilt from the first one — fy0 + 4q, exact in fp32, so dy and sigma keep their
    //  bits — instead of living in PPL registers: one more add per visited group, three registers less)
    constexpr bool FY_REBUILD = C > 5;
    float fy[FY_REBUILD ? 1 : PPL], T[PPL], A[PPL], bgT[BG0 ? 1 : PPL], vp[PPL][VC];
    int last_contributor[PPL];
    int wave_last = 0;  // deepest list position any pixel of this wave blended
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
        wave_last = max(wave_last, last_contributor[q]);
    }

    // Splats behind every pixel's last contributor are skipped by each lane in the reference
    // (render.jl:223); start the back-to-front walk at the deepest one any pixel blended.
    if (tid == 0) tile_last_s = 0;
    __syncthreads();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wave_last = max(wave_last, __shfl_xor(wave_last, off));
    if (lane == 0) atomicMax(&tile_last_s, wave_last);
    __syncthreads();
    const int tile_last = tile_last_s;  // process list positions tile_last-1 ... 0

    for (int base = 0; base < tile_last; base += BB) {
        const int cnt = min(BB, tile_last - base);
        __syncthreads();  // previous batch fully flushed
        if (tid < cnt) {
            const uint32_t idx = start + (uint32_t)(tile_last - 1 - base - tid);
            l0[tid] = stream.s0[idx];
            l1[tid] = stream.s1[idx];
            // staged as (third colour, footprint mask, depth, gradient-row slot): what the walk reads per splat is then
            // one aligned 64-bit LDS read in :rgb mode
            const float4 t2 = stream.s2[idx];
            l2[tid] = make_float4(t2.x, t2.w, t2.z, t2.y);
            if (C > 3) l3[tid] = stream.s3[idx];
        }
        __syncthreads();

        unsigned long long touched[BB / 64];
#pragma unroll
        for (int w = 0; w < BB / 64; w++) touched[w] = 0ull;
        float* const my = lacc[wave];
        // PAIR: the first instance of a pair waits here — the first level of its sums, its dx and its slab row — for the next
        // instance that blends a pixel; instances that blend none never enter a pair
        bool pending = false;
        int jrow_a = 0;
        gsr::RowColHalf half_a = {0.0f, 0.0f, 0.0f};
        float dx_a = 0.0f;
        for (int c0 = 0; c0 < cnt; c0 += 64) {
          const int jj = c0 + lane;
          const bool cand = jj < cnt && (__float_as_uint(l2[jj].y) & strip_bits) != 0u &&
                            (tile_last - 1 - base - jj) < wave_last;
          unsigned long long wl = wave_ballot(cand);  // splats whose footprint can touch this wave's rows
          while (wl) {
            const int j = c0 + __builtin_ctzll(wl);
            wl &= wl - 1;
            const int contributor = tile_last - 1 - base - j;  // 0-based position in the tile list
            const float4 a = l0[j], b = l1[j];
            float4 c2;  // (x: third colour, w: footprint mask, z: depth) as the stream has them
            const float4 t2 = l2[j];  // staged as (third colour, footprint mask, depth | :rgb blend threshold, slot)
            c2 = make_float4(t2.x, 0.0f, t2.z, t2.y);
            float4 t3 = t2;
            if (C > 3) t3 = l3[j];  // (normal xyz, blend threshold)
            const uint32_t thr_bits = __float_as_uint(C == 3 ? t2.z : t3.w);
            const float o = b.y;
            const float dx = a.x - fx;
            const SigmaX sx = sigma_x(a.z, a.w, dx);
            float f[C];
            unpack_features<C>(b, c2, t3, f);
            // A lane accumulates only  P = Σ G·vα,  U1 = Σ G·vα·dy,  U2 = Σ G·vα·dy²  and the
            // feature sums.  The conic / mean2d gradients (render.jl:262-272) are linear in
            // {dx²·P, dx·U1, U2, dx·P, U1}: those five are what the wave reduces, and the
            // per-instance flush applies the wave-uniform factors (-o/2, conic) once per row.
            float P = 0.0f, U1 = 0.0f, U2 = 0.0f, col[VC];
#pragma unroll
            for (int c = 0; c < VC; c++) col[c] = 0.0f;
            unsigned long long any_active = 0ull;
            const uint32_t rowbits = __builtin_amdgcn_readfirstlane(__float_as_uint(c2.w)) >> (ROWS * wave);
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
            if (PAIR) {
                // the first level of the network now, on the instance's own sums: what waits is its three results
                const gsr::RowColHalf half = gsr::wave_reduce_rowcol_rgb_half(P, U1, U2, col[0], col[1], col[VC > 2 ? 2 : 0]);
                if (!pending) {
                    pending = true;
                    jrow_a = jrow;
                    half_a = half;
                    dx_a = dx;
                    continue;
                }
                pending = false;
                const float total = gsr::wave_reduce_rowcol_rgb_pair(half_a, dx_a, half, dx, lane_bits, rowcol_pair);
                // even lane rows hold the sums of the parked instance, odd ones of this one
                if (rowcol_pair.slot >= 0) my[(lane_bits.odd_row ? jrow : jrow_a) + rowcol_pair.slot] = total;
            } else if (VC == 3) {
                // :rgb — reduce {P, U1, U2, rgb} over the 4 lanes of each pixel column first, apply the
                // column's dx weights, then finish over the 16 columns (wave_reduce.h: 5 swaps, not 8)
                const float total = gsr::wave_reduce_rowcol_rgb(P, U1, U2, col[0], col[1], col[2], dx, lane_bits, rowcol);
                if (rowcol.slot >= 0) my_row[rowcol.slot] = total;
            } else if (C == 5) {
                // :rgbd (the reference's default training mode): the same row-then-column scheme with the depth sum
                // riding along — six swaps instead of the generic network's eight; feature 4 (constant 1) is not a parameter
                const float total = gsr::wave_reduce_rowcol_rgbd(P, U1, U2, col[0], col[1], col[2], col[VC > 3 ? 3 : 0], dx, lane_bits, rowcol_d);
                if (rowcol_d.slot >= 0) my_row[rowcol_d.slot] = total;
            } else {
                float part[16];
#pragma unroll
                for (int k = 0; k < 16; k++) part[k] = 0.0f;
                const float dxp = dx * P;
                part[0] = col[0]; part[1] = col[1]; part[2] = col[2];
                part[3] = P;         // Σ G·vα          -> v opacity
                part[4] = dx * dxp;  // Σ dx²·G·vα      -> v conic.x  (× -o/2 in the flush)
                part[5] = dx * U1;   // Σ dx·dy·G·vα    -> v conic.y
                part[6] = U2;        // Σ dy²·G·vα      -> v conic.z
                part[7] = dxp;       // Σ dx·G·vα   }   -> v mean2d = -o·(conic · these)
                part[8] = U1;        // Σ dy·G·vα   }
                if (VC > 3) part[9] = col[VC > 3 ? 3 : 0];  // depth feature; channel 4 (constant 1) is not a parameter
                if (VC > 5) { part[10] = col[VC > 5 ? 5 : 0]; part[11] = col[VC > 5 ? 6 : 0]; part[12] = col[VC > 5 ? 7 : 0]; }
                // transposed wave64 reduction: ~3·NA/2 + 6 VALU ops, then ONE ds_write for all NA sums
                const float total = gsr::wave_reduce_transposed<NA>(part, lane_bits);
                // (storing the sums straight into the global row measured 3 % slower than the LDS slab + the
                // coalesced row stores of the flush)
                if (red_writer) my_row[red_slot] = total;
            }
          }
        }
        if (PAIR && pending) {  // an odd count: the batch's last instance is reduced alone
            const float total = gsr::wave_reduce_rowcol_rgb_rest(half_a, dx_a, lane_bits, rowcol);
            if (rowcol.slot >= 0) my[jrow_a + rowcol.slot] = total;
        }
        if (lane == 0) {
#pragma unroll
            for (int w = 0; w < BB / 64; w++) lmask[wave][w] = touched[w];
        }
        __syncthreads();
        if (tid < cnt) {
            float r[NA];
#pragma unroll
            for (int k = 0; k < NA; k++) r[k] = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; w++) {
                if ((lmask[w][tid >> 6] >> (tid & 63)) & 1ull) {
#pragma unroll
                    for (int k = 0; k < NA; k++) r[k] += lacc[w][tid * ST + k];
                }
            }
            bwd_store_row<C, VC>(inst.rows, l0[tid], l1[tid], l2[tid].w, r);
        }
    }
    bwd_zero_rows<C>(inst.rows, stream, start + (uint32_t)tile_last + tid, end);
