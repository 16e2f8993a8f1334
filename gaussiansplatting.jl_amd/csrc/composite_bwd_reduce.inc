// The reduction of one visited instance over the wave's 64 lanes, one instance at a time, and the store of its sums into the
// wave's slab row.  Text that follows composite_bwd_visit.inc: in composite_bwd_body.inc (the tile walk) wherever the
// instances are not reduced in pairs, and in PASS 2 of composite_bwd_long_kernel (the segment walk) always.  Names in scope:
//   C, VC, NA           compile-time;   dx, P, U1, U2, col, my_row   from the visit
//   lane_bits, rowcol, rowcol_d, red_slot, red_writer                the lane's constants of the networks (wave_reduce.h)
// (Text, not a function: as a function it reorders the instructions of all twelve composite_bwd_kernel instantiations —
// profiles/bwd_shared_visit/codegen_compare.txt.)  bench.py's hashes of the kernel sources, which mark
// profiles/pmc_traffic.json stale, cover composite.hip and not this file: after a change here, run tools/measure_pmc.sh again.
    if (VC == 3) {
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
        part[3] = P;           // Σ G·vα          -> v opacity
        part[4] = dx * dxp;    // Σ dx²·G·vα      -> v conic.x  (× -o/2 in the flush)
        part[5] = dx * U1;     // Σ dx·dy·G·vα    -> v conic.y
        part[6] = U2;          // Σ dy²·G·vα      -> v conic.z
        part[7] = dxp;         // Σ dx·G·vα   }   -> v mean2d = -o·(conic · these)
        part[8] = U1;          // Σ dy·G·vα   }
        if (VC > 3) part[9] = col[VC > 3 ? 3 : 0];  // depth feature; channel 4 (constant 1) is not a parameter
        if (VC > 5) { part[10] = col[VC > 5 ? 5 : 0]; part[11] = col[VC > 5 ? 6 : 0]; part[12] = col[VC > 5 ? 7 : 0]; }
        // transposed wave64 reduction: ~3·NA/2 + 6 VALU ops, then ONE ds_write for all NA sums
        const float total = gsr::wave_reduce_transposed<NA>(part, lane_bits);
        // (storing the sums straight into the global row measured 3 % slower than the LDS slab + the
        // coalesced row stores of the flush)
        if (red_writer) my_row[red_slot] = total;
    }
