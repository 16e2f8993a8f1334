// The body of sort_composite_fwd_kernel and of sort_composite_fwd_scored_kernel (composite.hip), included in both: as text, not as
// a function, so that the unscored kernel compiles to the code it had before the scored twin existed.  The including kernel defines
// `constexpr bool SCORED` (scored_form) and `GsrScores scores`.
// SCORED: 3 KB more LDS — six workgroups per CU instead of eight in the :rgbd / :rgbdn modes, still eight in :rgb — and one more
// barrier per chunk, in front of the flush (score_flush).
    // instances resident in LDS at a time: one per thread and round (512 / 1024 — whole lists — cost 5 / 3 workgroups per CU
    // instead of 8: +13 % / +48 %, profiles/r03/experiments/small_ab_notes.txt)
    constexpr int CHUNK = 256;
    __shared__ uint32_t ids[1024];
    __shared__ LdsSplats<C, CHUNK> e;
    // Bins of >= 1024 keys hold every list this launch takes complete whatever the longest one
    // is (lists beyond the capacity are tier tiles; the host scatters their keys again) — smaller bins must hold them all
    if (totals[GSR_TOTAL_D] > cap_instances || (totals[GSR_TOTAL_MAX_LIST] > bin_cap && bin_cap < 1024u)) return;
    const int tile = (int)tile_order[blockIdx.x];  // launch order: longest lists first
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t start = tile_start[tile], end = tile_start[tile + 1];
    const uint32_t n = end - start;
    if (tid == 0) {
        tile_count[tile] = 0u;  // counter ready for the next view
        // identify_tile_range! (utils.jl:56-78): empty tiles keep the (0,0) of the prior fill!
        ranges[2 * tile] = n ? start : 0u;
        ranges[2 * tile + 1] = n ? end : 0u;
    }
    if (n > 1024u) return;  // a tier launch's tile (sort and forward)
    const int tile_x = tile % grid_x, tile_y = tile / grid_x;
    const int X0 = tile_x * GSR_TILE, Y0 = tile_y * GSR_TILE;
    const int quad = wave;  // 8x8 quadrant (qx = quad & 1, qy = quad >> 1) of the tile
    const uint32_t strip_bits = 0x10000u << quad;
    const int px = X0 + 8 * (quad & 1) + (lane & 7), py = Y0 + 8 * (quad >> 1) + (lane >> 3);
    const bool inside = px < W && py < H;
    float fx = (float)px, fy = (float)py;
    // (opaque to the optimiser: left alone it re-converts px / py inside the per-visit loop to save two registers —
    // two more VALU instructions per visit in a VALU-bound loop)
    asm volatile("" : "+v"(fx), "+v"(fy));
    FwdPixel<C> p;
    fwd_pixel_init<C>(p, inside);
    __shared__ ScoreLds<SCORED, CHUNK> sl;
    if constexpr (SCORED) {  // (ordered in front of the first visit by the barrier behind the sort)
        sl.v[0][tid] = 0u; sl.v[1][tid] = 0u; sl.v[2][tid] = 0u;
    }
    if (n > 0) {
        // (the sorting wave rotates with the workgroup id: wave w of every workgroup sits on SIMD w of its CU, and a fixed
        // sorter would load one SIMD of four with all the sorting)
        if (wave == (int)(blockIdx.x & 3u)) gsr_sort::wave_sort_ids_any(ids, n, lane, bins + (size_t)tile * bin_cap);
        __syncthreads();
        for (uint32_t cbase = 0; cbase < n; cbase += CHUNK) {
            const uint32_t i = cbase + (uint32_t)tid;
            if (i < n) {
                const uint32_t id = ids[i];
                const gsr_sort::InstanceVals v = gsr_sort::instance_vals<C>(id, X0, Y0, geom);
                if (KEEP) {
                    const uint32_t pos = start + i;
                    values_sorted[pos] = id;
                    stream.s0[pos] = v.v0; stream.s1[pos] = v.v1; stream.s2[pos] = v.v2;
                    if (C > 3) stream.s3[pos] = v.v3;
                }
                e(0, tid) = v.v0; e(1, tid) = v.v1;
                // LDS copy: (third colour, 1-based list position, depth | :rgb blend threshold, footprint masks)
                e(2, tid) = make_float4(v.v2.x, __uint_as_float(i + 1u), v.v2.z, v.v2.w);
                if (C > 3) e(C > 3 ? 3 : 0, tid) = v.v3;
            }
            __syncthreads();
            const int cnt = (int)min((uint32_t)CHUNK, n - cbase);
            for (int b = 0; b < cnt; b += 64) {
                if (p.done == ~0ull) break;  // the whole quadrant has saturated (a scalar compare)
                const int k = b + lane;
                const bool cand = k < cnt && (__float_as_uint(e(2, k).w) & strip_bits) != 0u;
                const unsigned long long m = wave_ballot(cand);
                if (m == 0ull) continue;
                if constexpr (SCORED)
                    fwd_blend_selected<C, AUX, CHUNK, true>(p, m, e, b, fx, fy, ids + cbase + b, covis, lds_address(&sl.v[0][0]));
                else
                fwd_blend_selected<C, AUX, CHUNK>(p, m, e, b, fx, fy, ids + cbase + b, covis);
            }
            if constexpr (SCORED) {
                // every wave's DS atomics of the chunk have landed; thread tid owns entry tid's words: one triple of global
                // atomics per tile instance that was blended at all (the next chunk's emit barrier orders the re-zeroing)
                score_drain();
                __syncthreads();
                if (tid < cnt) score_flush<CHUNK>(sl, tid, ids[cbase + (uint32_t)tid], scores);
            } else
            if (cbase + CHUNK < n) __syncthreads();  // the chunk is consumed before the next one overwrites it
        }
    }
    fwd_pixel_store<C, AUX>(p, inside, px, py, W, bg, image, n_contrib, final_T, uncert);
