// The tile walk: the body of composite_bwd_kernel<C, BG0, VC, ACC> and of composite_bwd_kernel_rgb_bg0 (composite.hip), included
// inside each, with C, BG0, VC, ACC and the kernels' arguments in scope.  (Text, not a function: as a __device__ function template
// the same lines compile with one VGPR more in the six VC == C > 3 instantiations.)  What it shares with the segment walk
// (composite_bwd_long_kernel) is text of its own, included here and there: the per-pixel state (composite_bwd_state.inc), the
// visit of one instance (composite_bwd_visit.inc, which includes composite_bwd_decode.inc) and the one-at-a-time reduction
// (composite_bwd_reduce.inc); the paired reduction (PAIR) is this walk's alone.  bench.py's hashes of the kernel sources, which
// mark profiles/pmc_traffic.json stale, cover composite.hip and none of these texts: after a change here, run
// tools/measure_pmc.sh again.
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
    // deepest list position any pixel of this wave blended
#include "composite_bwd_state.inc"
    int wave_last = deepest;

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
        if (tid < cnt) bwd_stage_entry<C>(stream, start + (uint32_t)(tile_last - 1 - base - tid), tid, l0, l1, l2, l3);
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
#include "composite_bwd_visit.inc"
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
            } else {
#include "composite_bwd_reduce.inc"
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
