// The body of composite_fwd_strip_kernel and of composite_fwd_strip_scored_kernel (composite.hip), included in both: as text, not
// as a function, so that the unscored kernel compiles to the code it had before the scored twin existed.  The including kernel
// defines `constexpr bool SCORED` (scored_form) and `GsrScores scores`.
    __shared__ LdsSplats<C, 64> e;
    // 1-D grid, workgroup id -> (launch slot, strip).  Workgroups are dealt round-robin to the 8
    // XCDs (each with its own L2): the 4 strips of a tile get ids that are equal mod 8, so a tile's
    // splat stream is fetched into ONE L2; slots follow tile_order (longest lists first).
    const int id = blockIdx.x, k = id >> 3;
    const int quad = k & 3;  // 8x8 quadrant (qx = quad & 1, qy = quad >> 1) of the tile
    const int slot = ((k >> 2) << 3) | (id & 7);
    int tile;
    if (tile_order) {  // every tile, in launch order
        if (slot >= grid_x * ((H + GSR_TILE - 1) / GSR_TILE)) return;
        tile = (int)tile_order[slot];
    } else {           // only the tiles of the scan's tier lists (the fused kernel did the others), longest tier first
        if ((uint32_t)slot >= tiers.n_big + tiers.n_mid8 + tiers.n_mid4) return;
        GSR_TIER_TILE(tile, tiers, (uint32_t)slot);
        // beside the fused launch (gsr_forward): these few waves are the forward's critical path and share their SIMDs with it
        if (tiers.split_len) __builtin_amdgcn_s_setprio(3);
    }
    if constexpr (SCORED) {
        __shared__ ScoreLds<true, 64> sl;
        composite_fwd_quadrant<C, AUX, true>(W, H, grid_x, tile, quad, (int)threadIdx.x, tile_start, stream, bg, image,
                                             n_contrib, final_T, values_sorted, covis, uncert, e, &sl, scores);
    } else
    composite_fwd_quadrant<C, AUX>(W, H, grid_x, tile, quad, (int)threadIdx.x, tile_start, stream, bg, image,
                                   n_contrib, final_T, values_sorted, covis, uncert, e);
