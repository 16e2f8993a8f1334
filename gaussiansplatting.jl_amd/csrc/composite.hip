// Per-tile alpha compositing, forward and backward.
// Reference behaviour: src/rasterization/render.jl:1-130 (`render!`) and :132-286
// (`∇render!`); SURVEY.md A.8 / A.9.
//
// A tile's depth-sorted splat list is a contiguous slice of the packed stream written by
// tile_sort (three coalesced float4 planes) and carries a 16-bit row mask per instance.
//
// Forward (`composite_fwd_strip_kernel`): one wave64 per 8x8 pixel quadrant, lane <-> pixel.
// Per 64 instances one ballot over the quadrant masks gives the wave's work list; only those
// splats are staged in LDS and read back with wave-uniform (broadcast) ds_read_b128.
//
// Backward: instead of the reference's (C+6) global float atomics per (pixel, splat)
// (render.jl:242,275-282) ONE wave64 owns the whole tile (4 pixels per lane), reduces the
// partials of a splat over its 64 lanes with a transposed permlane-swap / DPP network
// (wave_reduce.h), and one 64-byte gradient ROW per (tile, splat) instance leaves the
// workgroup as plain stores; the per-Gaussian kernel sums a Gaussian's rows.
#include "gsr_kernels.h"
#include "gsr_dispatch.h"
#include "wave_reduce.h"
#include "tile_sort_device.h"


namespace {

struct Bg { float v[8]; };

// wave64 ballot straight from the compare mask (HIP's __ballot goes through v_cndmask + v_cmp_ne)
__device__ __forceinline__ unsigned long long wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// The Gaussian exponent  sigma = b·dx·dy + ½(a·dx² + c·dy²)  (render.jl:90-91 and :226-227) — ONE definition, with
// explicitly rounded operations, used by the forward AND the backward kernel: the backward replays exactly the
// contributor set the forward blended (`sigma >= 0`, `alpha >= 1/255` and the `T' < 1e-4` stop are decided on
// bit-identical sigma / alpha in both passes, whatever the compiler's FMA contraction would have done to two
// differently written expressions).  The sorted stream carries ha = a/2 and hc = c/2 (exact halvings).
struct SigmaX { float hxx, bdx; };  // the dx-dependent part, shared by the pixels of a column
__device__ __forceinline__ SigmaX sigma_x(float ha, float b, float dx) {
    return SigmaX{__fmul_rn(ha, __fmul_rn(dx, dx)), __fmul_rn(b, dx)};
}
__device__ __forceinline__ float sigma_of(const SigmaX sx, float hc, float dy, float dy2) {
    return __fmaf_rn(sx.bdx, dy, __fmaf_rn(hc, dy2, sx.hxx));
}
__device__ __forceinline__ float alpha_of(float opacity, float G) { return fminf(0.99f, __fmul_rn(opacity, G)); }

// N splats staged in LDS: the three (four with a normal) float4 planes of their stream entries in ONE array, so that the
// per-visit reads of a wave-uniform entry are one address (16·j: a scalar shift + one v_mov) and compile-time immediate
// offsets (plane · 16·N) instead of one address computation per plane — 2 VALU instructions per visit less in loops that
// are VALU-issue-bound; planes (not 48-byte records) keep the lane-contiguous staging stores conflict-free.
template <int C, int N> struct LdsSplats {
    float4 q[C > 3 ? 4 : 3][N];  // (fourth plane: normal xyz (:rgbdn) + the blend threshold in w, :rgbd / :rgbdn)
    __device__ __forceinline__ const float4& operator()(int plane, int j) const { return q[plane][j]; }
    __device__ __forceinline__ float4& operator()(int plane, int j) { return q[plane][j]; }
};

// feature c of a staged splat: rgb | depth | 1 | normal  (rasterizer.jl:380-385)
template <int C>
__device__ __forceinline__ void unpack_features(const float4& s1, const float4& s2, const float4& s3, float f[C]) {
    f[0] = s1.z; f[1] = s1.w; f[2] = s2.x;
    if (C > 3) { f[3] = s2.z; f[4] = 1.0f; }
    if (C > 5) { f[5] = s3.x; f[6] = s3.y; f[7] = s3.z; }
}

// ---------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------
// Forward: one wave64 per 8x8 quadrant (a square footprint is visited by 9.5 % fewer splats than a 16x4 strip).
// No workgroup barriers inside a batch, a quadrant stops as soon as ITS pixels have saturated, and a wave visits only
// the splats its quadrant-mask ballot selected.  Same per-pixel arithmetic in the same order as render.jl:82-117.
//
// The per-pixel state of a lane and the blend of the LDS-resident splats a ballot selected are shared by
//   * composite_fwd_strip_kernel: four independent single-wave workgroups per tile, each staging the splats its ballot
//     selected from the global stream into its own 64-entry LDS arrays (tiers of long lists; views in compact mode);
//   * sort_composite_fwd_kernel: the fused sort + forward, which composites straight from the 256-entry LDS chunk the
//     workgroup has just emitted — the stream in HBM is written for the backward and never read back here.
template <int C> struct FwdPixel {
    unsigned long long done;  // wave-level, in SGPRs: bit l <-> lane l has saturated or its pixel lies outside the image
    float T, unc;
    uint32_t last;
    float color[C];
};

template <int C>
__device__ __forceinline__ void fwd_pixel_init(FwdPixel<C>& p, bool inside) {
    p.done = wave_ballot(!inside); p.T = 1.0f; p.unc = 0.0f; p.last = 0;
#pragma unroll
    for (int c = 0; c < C; c++) p.color[c] = 0.0f;
}

// The state update of one visit for the lanes of `ok`, under EXEC narrowed to them:  T <- Tn,  last <- pos,
// colour[c] += f[c]·w  (feature 4 of :rgbd / :rgbdn is the constant 1: an add),  unc += w  (AUX).
// ONE asm statement per (C, AUX): between two statements the compiler may schedule VALU work of its own, which would then
// run under the narrowed mask.  Inside are the two mask moves, v_mov_b32, v_fmac_f32 and v_add_f32 — no memory instruction,
// nothing with a hazard against a scalar write of EXEC.  The saved mask is written before `ok` is read: early-clobber.
#define GSR_FWD_REGION(BODY) \
    "s_and_saveexec_b64 %[sv], %[ok]\n\tv_mov_b32 %[T], %[Tn]\n\tv_mov_b32 %[last], %[pos]\n\t" BODY "s_mov_b64 exec, %[sv]"
#define GSR_FWD_RGB "v_fmac_f32 %[c0], %[f0], %[w]\n\tv_fmac_f32 %[c1], %[f1], %[w]\n\tv_fmac_f32 %[c2], %[f2], %[w]\n\t"
#define GSR_FWD_D   "v_fmac_f32 %[c3], %[f3], %[w]\n\tv_add_f32 %[c4], %[c4], %[w]\n\t"
#define GSR_FWD_N   "v_fmac_f32 %[c5], %[f5], %[w]\n\tv_fmac_f32 %[c6], %[f6], %[w]\n\tv_fmac_f32 %[c7], %[f7], %[w]\n\t"
#define GSR_FWD_UNC "v_add_f32 %[unc], %[unc], %[w]\n\t"
#define GSR_FWD_OUT      [sv] "=&s"(saved), [T] "+v"(p.T), [last] "+v"(p.last)
#define GSR_FWD_OUT_RGB  GSR_FWD_OUT, [c0] "+v"(p.color[0]), [c1] "+v"(p.color[1]), [c2] "+v"(p.color[2])
#define GSR_FWD_OUT_D    GSR_FWD_OUT_RGB, [c3] "+v"(p.color[3]), [c4] "+v"(p.color[4])
#define GSR_FWD_OUT_N    GSR_FWD_OUT_D, [c5] "+v"(p.color[5]), [c6] "+v"(p.color[6]), [c7] "+v"(p.color[7])
#define GSR_FWD_IN       [ok] "s"(ok), [Tn] "v"(Tn), [pos] "v"(pos), [w] "v"(w)
#define GSR_FWD_IN_RGB   GSR_FWD_IN, [f0] "v"(f[0]), [f1] "v"(f[1]), [f2] "v"(f[2])
#define GSR_FWD_IN_D     GSR_FWD_IN_RGB, [f3] "v"(f[3])
#define GSR_FWD_IN_N     GSR_FWD_IN_D, [f5] "v"(f[5]), [f6] "v"(f[6]), [f7] "v"(f[7])
template <int C, bool AUX>
__device__ __forceinline__ void fwd_update_under_exec(FwdPixel<C>& p, unsigned long long ok, float Tn, float pos, float w, const float (&f)[C]) {
    unsigned long long saved;
    if constexpr (C == 3 && !AUX) asm volatile(GSR_FWD_REGION(GSR_FWD_RGB) : GSR_FWD_OUT_RGB : GSR_FWD_IN_RGB : "scc");
    if constexpr (C == 3 && AUX)  asm volatile(GSR_FWD_REGION(GSR_FWD_RGB GSR_FWD_UNC) : GSR_FWD_OUT_RGB, [unc] "+v"(p.unc) : GSR_FWD_IN_RGB : "scc");
    if constexpr (C == 5 && !AUX) asm volatile(GSR_FWD_REGION(GSR_FWD_RGB GSR_FWD_D) : GSR_FWD_OUT_D : GSR_FWD_IN_D : "scc");
    if constexpr (C == 5 && AUX)  asm volatile(GSR_FWD_REGION(GSR_FWD_RGB GSR_FWD_D GSR_FWD_UNC) : GSR_FWD_OUT_D, [unc] "+v"(p.unc) : GSR_FWD_IN_D : "scc");
    if constexpr (C == 8 && !AUX) asm volatile(GSR_FWD_REGION(GSR_FWD_RGB GSR_FWD_D GSR_FWD_N) : GSR_FWD_OUT_N : GSR_FWD_IN_N : "scc");
    if constexpr (C == 8 && AUX)  asm volatile(GSR_FWD_REGION(GSR_FWD_RGB GSR_FWD_D GSR_FWD_N GSR_FWD_UNC) : GSR_FWD_OUT_N, [unc] "+v"(p.unc) : GSR_FWD_IN_N : "scc");
}

// ---- per-Gaussian contribution scores (gsr_scores; the SCORED instantiations) ----
// What a set of views uses of a Gaussian, from the blend weights w = alpha·T of the visits that blend it: max_p w is RadSplat's
// pruning score (Niemeyer et al. 2024, eq. 7-8: prune below 0.01), sum_p w and the hit count are the importance terms of
// LightGaussian (Fan et al. 2023, global significance) and Mini-Splatting (Fang & Wang 2024).  No reference counterpart: the
// reference exports the per-PIXEL sum of the same w (uncertainties, render.jl:109) and nothing per Gaussian.
// All three are INTEGERS — max of the bits of w (w > 0: float order is unsigned order), a count, and the sum of
// q = rne(w · 2^24) (w <= 0.99: q < 2^24, a wave's 64 of them < 2^30, the four waves of a tile < 2^32) — so every grouping of
// the updates gives the same bits: per wave by DPP (gsr::wave_max_u32 / wave_sum_u32), per tile instance in N x 3 words of LDS
// (ds_max_u32 / ds_add_u32 from one lane of each quadrant wave), per Gaussian by ONE triple of non-returning global integer
// atomics per tile instance that was blended at all.  No float atomic anywhere.
// (SCORED inside the kernel bodies shared as text — composite_fwd_*_body.inc: dependent on the kernel's template parameters, so
// that the discarded branches of the unscored kernels are not instantiated)
template <int C, bool S> inline constexpr bool scored_form = S;
template <bool ON, int N> struct ScoreLds {};
template <int N> struct ScoreLds<true, N> { uint32_t v[3][N]; };  // [0] max of bits(w), [1] hits, [2] sum of q — per staged entry
// the byte address of an LDS object, as the DS instructions take it
__device__ __forceinline__ uint32_t lds_address(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}
// One visit's update of entry `j`'s three words (sc = LDS address of word [0][0]): the wave's totals are wave-uniform, so ONE
// lane issues the three DS atomics — under EXEC = lane 0, set and restored on the scalar unit like fwd_update_under_exec's
// region, not as `if (lane == 0)`: a branch per visit.  (The DS unit takes EXEC at issue; nothing in the region depends on a
// VALU write of EXEC or of an SGPR.  The compiler does not count these DS operations: score_drain waits for them.)
template <int N>
__device__ __forceinline__ void score_visit(uint32_t sc, int j, unsigned long long ok, float w) {
    const bool mine = __builtin_amdgcn_inverse_ballot_w64(ok);
    const uint32_t wmax = gsr::wave_max_u32(mine ? __float_as_uint(w) : 0u);
    const uint32_t qsum = gsr::wave_sum_u32(mine ? __float2uint_rn(__fmul_rn(w, 16777216.0f)) : 0u);
    const uint32_t hits = (uint32_t)__builtin_popcountll(ok);
    const uint32_t addr = sc + 4u * (uint32_t)j;
    unsigned long long saved;
    asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, 1\n\t"
                 "ds_max_u32 %[a], %[m]\n\tds_add_u32 %[a], %[h] offset:%[o1]\n\tds_add_u32 %[a], %[q] offset:%[o2]\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [sv] "=&s"(saved)
                 : [a] "v"(addr), [m] "v"(wmax), [h] "v"(hits), [q] "v"(qsum), [o1] "n"(4 * N), [o2] "n"(8 * N)
                 : "memory");
}
// Entry `k`'s words to its Gaussian `id`, by one thread, and zero again for the next chunk / batch.  Called behind a barrier
// of every wave that updates the words; the inline DS atomics are invisible to the compiler's counters, hence the explicit wait
// in front of that barrier (score_drain).
__device__ __forceinline__ void score_drain() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <int N>
__device__ __forceinline__ void score_flush(ScoreLds<true, N>& sl, int k, uint32_t id, const GsrScores& out) {
    const uint32_t hits = sl.v[1][k];
    if (hits) {
        if (out.max_weight) atomicMax(out.max_weight + id, sl.v[0][k]);
        if (out.hits) atomicAdd(out.hits + id, (unsigned long long)hits);
        if (out.weight_sum) atomicAdd(out.weight_sum + id, (unsigned long long)sl.v[2][k]);
        sl.v[0][k] = 0u; sl.v[1][k] = 0u; sl.v[2][k] = 0u;
    }
}

// Blend the LDS entries whose bits are set in `m` (bit k <-> entry e0 + k), front to back.  Plane 2 of an entry holds
// (third colour, 1-BASED LIST POSITION, depth, -): `last` is then a move between two VGPRs, not a v_mov of the scalar
// position.  `ids`: Gaussian id of entry 0, 1, ... (only read for the covisibility output).
// SCORED: every visit also updates the three score words of its entry (`sc`: LDS address of ScoreLds::v, score_visit).
template <int C, bool AUX, int N, bool SCORED = false>
__device__ __forceinline__ void fwd_blend_selected(FwdPixel<C>& p, unsigned long long m, const LdsSplats<C, N>& e, int e0, float fx, float fy,
                                                   const uint32_t* __restrict__ ids, uint8_t* __restrict__ covis, uint32_t sc = 0u) {
    while (m) {
        const int jb = __builtin_ctzll(m), j = e0 + jb;
        m &= m - 1;
        // (x = third colour, y = list position: ONE 64-bit LDS read — left as two fields of q[2] the compiler sinks
        // the position's read under EXEC = ok, which costs a masked region per visit)
        float4 c2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        c2 = e(2, j);  // (x = third colour, y = list position, z = blend threshold (:rgb) or depth)
        const float4 a = e(0, j), b = e(1, j);
        const float4 c3 = C > 3 ? e(C > 3 ? 3 : 0, j) : c2;
        const float dx = a.x - fx, dy = a.y - fy;
        const float sigma = sigma_of(sigma_x(a.z, a.w, dx), b.x, dy, __fmul_rn(dy, dy));
        const float alpha = alpha_of(b.y, __expf(-sigma));
        // Branch-free body: every lane computes the blend; the lanes that take it are a wave-level mask, built on the
        // scalar unit from the ballots of the two bare compares (no per-lane bool in between: the compiler would
        // materialise it with a v_cndmask and compare it back), and the state is updated under EXEC = that mask.  A lane
        // that is done, or whose pixel this splat does not touch, keeps its state untouched (what `continue`/`break`
        // leave behind, render.jl:92-101).  (As selects on the mask: three v_cndmask more per visit.  As `if (ok)`, or
        // with the saturating lanes in a wave-uniform rare path: a branch per visit, measured 10 % slower.)
        const float Tn = p.T * (1.0f - alpha);
        const unsigned long long small = wave_ballot(Tn < 1e-4f);
        // sigma >= 0 && alpha >= 1/255 as one unsigned compare against the instance's threshold (tile_sort_device.h)
        const unsigned long long touch = wave_ballot(__float_as_uint(sigma) < __float_as_uint(C == 3 ? c2.z : c3.w));
        const unsigned long long okpre = touch & ~p.done;
        const unsigned long long stop = okpre & small;
        p.done |= stop;
        const unsigned long long ok = okpre ^ stop;
        float f[C];
        unpack_features<C>(b, c2, c3, f);
        const float w = alpha * p.T;
        // (covisibility: decided on the transmittance BEFORE the update)
        // (a null `covis` empties the mask: as a test of its own in front of the store it is a second branch per visit)
        const unsigned long long seen = AUX ? ok & wave_ballot(p.T > 0.5f) & (covis ? ~0ull : 0ull) : 0ull;
        fwd_update_under_exec<C, AUX>(p, ok, Tn, c2.y, w, f);
        if (AUX && __builtin_amdgcn_inverse_ballot_w64(seen)) covis[ids[jb]] = 1;
        if constexpr (SCORED) score_visit<N>(sc, j, ok, w);
    }
}

template <int C, bool AUX>
__device__ __forceinline__ void fwd_pixel_store(const FwdPixel<C>& p, bool inside, int px, int py, int W, const Bg& bg,
                                                float* __restrict__ image, uint32_t* __restrict__ n_contrib,
                                                float* __restrict__ final_T, float* __restrict__ uncert) {
    if (inside) {
        const size_t pi = (size_t)px + (size_t)W * py;
        final_T[pi] = p.T;
        n_contrib[pi] = p.last;
#pragma unroll
        for (int c = 0; c < C; c++) image[(size_t)C * pi + c] = p.color[c] + p.T * bg.v[c];
        if (AUX && uncert) uncert[pi] = p.unc;
    }
}

// One quadrant wave walking its tile's slice of the GLOBAL stream (e: its 64-entry LDS staging array).
template <int C, bool AUX, bool SCORED = false>
__device__ __forceinline__ void composite_fwd_quadrant(int W, int H, int grid_x, int tile, int quad, int lane,
                                                       const uint32_t* __restrict__ tile_start, GsrStream stream,
                                                       const Bg& bg, float* __restrict__ image,
                                                       uint32_t* __restrict__ n_contrib, float* __restrict__ final_T,
                                                       const uint32_t* __restrict__ values_sorted,
                                                       uint8_t* __restrict__ covis, float* __restrict__ uncert,
                                                       LdsSplats<C, 64>& e, ScoreLds<SCORED, 64>* sl = nullptr,
                                                       GsrScores scores = GsrScores{nullptr, nullptr, nullptr}) {
    const int tile_x = tile % grid_x, tile_y = tile / grid_x;
    const uint32_t strip_bits = 0x10000u << quad;  // the instance's quadrant bit (tile_mask.h)
    const int px = tile_x * GSR_TILE + 8 * (quad & 1) + (lane & 7), py = tile_y * GSR_TILE + 8 * (quad >> 1) + (lane >> 3);
    const bool inside = px < W && py < H;
    const float fx = (float)px, fy = (float)py;
    const uint32_t start = tile_start[tile], end = tile_start[tile + 1];
    const int to_do = (int)(end - start);
    FwdPixel<C> p;
    fwd_pixel_init<C>(p, inside);
    if constexpr (SCORED) {  // (single wave, in-order LDS: visible to the first batch's atomics)
        sl->v[0][lane] = 0u; sl->v[1][lane] = 0u; sl->v[2][lane] = 0u;
    }
    for (int base = 0; base < to_do; base += 64) {
        if (p.done == ~0ull) break;  // the whole quadrant has saturated (a scalar compare)
        const int jj = base + lane;
        float4 r2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (jj < to_do) r2 = stream.s2[start + jj];
        const bool cand = jj < to_do && (__float_as_uint(r2.w) & strip_bits) != 0u;
        const unsigned long long m = wave_ballot(cand);
        if (m == 0ull) continue;
        // (Fetching the wave-uniform splats with scalar loads straight from the stream — s_load_dwordx4,
        // one candidate ahead, no LDS — measured 2.6x slower: the scalar cache does not keep up.)
        __builtin_amdgcn_wave_barrier();  // previous batch's LDS reads are done (single wave, in order)
        if (cand) {
            e(0, lane) = stream.s0[start + jj];
            e(1, lane) = stream.s1[start + jj];
            r2.y = __uint_as_float((uint32_t)(jj + 1));  // the forward has no use for the gradient-row slot: list position
            e(2, lane) = r2;
            if (C > 3) e(C > 3 ? 3 : 0, lane) = stream.s3[start + jj];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if constexpr (SCORED) {
            // the batch's words, per staged entry: lane <-> entry, flushed per batch — one triple of global atomics per
            // (quadrant, instance) this wave blended: the tier walk is the rare path
            fwd_blend_selected<C, AUX, 64, true>(p, m, e, 0, fx, fy, values_sorted + start + base, covis, lds_address(&sl->v[0][0]));
            score_drain();
            __builtin_amdgcn_wave_barrier();
            if (cand) score_flush<64>(*sl, lane, values_sorted[start + jj], scores);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else
        fwd_blend_selected<C, AUX, 64>(p, m, e, 0, fx, fy, values_sorted + start + base, covis);
    }
    fwd_pixel_store<C, AUX>(p, inside, px, py, W, bg, image, n_contrib, final_T, uncert);
}


template <int C, bool AUX>
__global__ __launch_bounds__(64) void composite_fwd_strip_kernel(int W, int H, int grid_x,
                                                                 const uint32_t* __restrict__ tile_start,
                                                                 const uint32_t* __restrict__ tile_order,
                                                                 GsrStream stream, Bg bg, float* __restrict__ image,
                                                                 uint32_t* __restrict__ n_contrib,
                                                                 float* __restrict__ final_T,
                                                                 const uint32_t* __restrict__ values_sorted,
                                                                 uint8_t* __restrict__ covis,
                                                                 float* __restrict__ uncert, GsrTierLists tiers) {
    constexpr bool SCORED = scored_form<C, false>;
    const GsrScores scores{nullptr, nullptr, nullptr};
#include "composite_fwd_strip_body.inc"
}
// The scored twin: the same walk with the per-Gaussian contribution scores (gsr_scores).  A kernel NAME of its own, not a
// template argument of the kernel above: the unscored instantiations keep their names, parameter lists and code.
template <int C, bool AUX>
__global__ __launch_bounds__(64) void composite_fwd_strip_scored_kernel(int W, int H, int grid_x,
                                                                 const uint32_t* __restrict__ tile_start,
                                                                 const uint32_t* __restrict__ tile_order,
                                                                 GsrStream stream, Bg bg, float* __restrict__ image,
                                                                 uint32_t* __restrict__ n_contrib,
                                                                 float* __restrict__ final_T,
                                                                 const uint32_t* __restrict__ values_sorted,
                                                                 uint8_t* __restrict__ covis,
                                                                 float* __restrict__ uncert, GsrTierLists tiers, GsrScores scores) {
    constexpr bool SCORED = scored_form<C, true>;
#include "composite_fwd_strip_body.inc"
}

// Sort + forward of a tile in ONE workgroup (fixed-capacity bins; a tile with more than 1024 instances is left to the
// tier sorts and a forward launch over the tier lists).
// Wave 0 sorts the tile's keys in registers; then, 256 instances at a time, all four waves EMIT a chunk of the sorted
// list — record gather -> packed stream entry, stored to HBM for the backward AND kept in LDS — and each wave composites
// its 8x8 quadrant straight from that LDS chunk.  Round 2 read the entries back from HBM (the workgroup's own stores,
// four times: 950 MB counted against 322 MB algorithmic, because a line lives ~18 us in an L2 the sort's gathers stream
// through); now the forward never reads the stream, needs no workgroup-scope release/acquire on global memory between
// the two phases, and no per-batch staging copy.  tile_sort alone is bound by HBM (gather + stream write) and the
// compositing alone by VALU issue; as phases of independent workgroups they share the CU at the same time.  Launched
// BEFORE the host has read the scan's totals, like the sort's main pass was: every workgroup checks the totals against
// the capacity of the buffers and leaves everything untouched when this view needs more (the host then runs the
// separate sort and forward launches).
// KEEP = false (GSR_FORWARD_ONLY, the reference's non-AD branch rasterizer.jl:214-248): the emitted chunk lives in LDS only —
// the 52-68 bytes per instance of stream + id that nothing but the backward reads are not stored.

template <int C, bool AUX, bool KEEP>
// (8 waves per SIMD: the sort needs 66 VGPRs left to itself; at 64 it does not spill and an eighth workgroup fits the CU)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void sort_composite_fwd_kernel(int W, int H, int grid_x,
                                                                 const uint32_t* __restrict__ tile_start,
                                                                 const uint32_t* __restrict__ tile_order,
                                                                 uint32_t* __restrict__ tile_count,
                                                                 const uint64_t* __restrict__ bins, uint32_t bin_cap,
                                                                 GsrGeom geom, GsrStream stream, Bg bg,
                                                                 float* __restrict__ image,
                                                                 uint32_t* __restrict__ n_contrib,
                                                                 float* __restrict__ final_T,
                                                                 uint32_t* __restrict__ values_sorted,
                                                                 uint32_t* __restrict__ ranges,
                                                                 uint8_t* __restrict__ covis, float* __restrict__ uncert,
                                                                 const uint32_t* __restrict__ totals,
                                                                 uint32_t cap_instances) {
    constexpr bool SCORED = scored_form<C, false>;
    const GsrScores scores{nullptr, nullptr, nullptr};
#include "composite_fwd_fused_body.inc"
}
// The scored twin (a kernel name of its own, like composite_fwd_strip_scored_kernel).  :rgbd / :rgbdn fit six workgroups per CU
// with the score words in LDS and are compiled for six waves per SIMD.
template <int C, bool AUX, bool KEEP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(C > 3 ? 6 : 8))) void sort_composite_fwd_scored_kernel(int W, int H, int grid_x,
                                                                 const uint32_t* __restrict__ tile_start,
                                                                 const uint32_t* __restrict__ tile_order,
                                                                 uint32_t* __restrict__ tile_count,
                                                                 const uint64_t* __restrict__ bins, uint32_t bin_cap,
                                                                 GsrGeom geom, GsrStream stream, Bg bg,
                                                                 float* __restrict__ image,
                                                                 uint32_t* __restrict__ n_contrib,
                                                                 float* __restrict__ final_T,
                                                                 uint32_t* __restrict__ values_sorted,
                                                                 uint32_t* __restrict__ ranges,
                                                                 uint8_t* __restrict__ covis, float* __restrict__ uncert,
                                                                 const uint32_t* __restrict__ totals,
                                                                 uint32_t cap_instances, GsrScores scores) {
    constexpr bool SCORED = scored_form<C, true>;
#include "composite_fwd_fused_body.inc"
}

// ---------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------
// accumulator row per staged splat: [0..2] v rgb, [3] v opacity, [4..6] v conic,
// [7..8] v mean2d, [9] v depth (C>=5), [10..12] v normal (C==8)
template <int C> struct AccRow { static constexpr int N = C == 3 ? 9 : (C == 5 ? 10 : 13); static constexpr int STRIDE = N | 1; };

// ACC — the backward's per-pixel arithmetic in its ACCURATE form (round 6; gsr_config.grad_precision = GSR_GRAD_ACCURATE /
// GSR_GRAD_FP32_REFERENCE): libm-accurate expf instead of v_exp_f32 on the rounded product sigma x log2(e), IEEE division
// instead of v_rcp_f32 for T / (1 - alpha) — what the reference's Julia source means by `exp` and `/` (render.jl:236-259).
// On needle-shaped splats the backward's sums cancel by up to the square of the 2-D axis ratio, and the few-ulp SYSTEMATIC
// errors of the two fast instructions — fed through the T recursion of hundreds of contributors — are what put ∇means of
// a 90 : 1 needle of radius 100 px (edge 8498) 4.1e-4 from float64: with ACC 2.3e-5, the oracle's own distance
// (profiles/r06/experiments/needle_exact_exp_div_variants.txt; the wave reduction round 5 suspected is NOT the source).
// Costs +12 % of this kernel, so it is a per-handle choice, not the default; gating it per instance on a "needle" bit of the
// stream was built and dropped: +2.5 % at config 3 (which has no needles), +9 % on the trained-like scene, and with
// ~1-ulp refinements instead of libm the gain drowned in last-bit noise (needle_gated_refinement_*.txt / .patch).
template <bool ACC> __device__ __forceinline__ float bwd_exp_neg(float sigma) { return ACC ? expf(-sigma) : __expf(-sigma); }
template <bool ACC> __device__ __forceinline__ float bwd_rcp(float x) { return ACC ? __fdiv_rn(1.0f, x) : __builtin_amdgcn_rcpf(x); }

// Both backward kernels — composite_bwd_kernel (a whole tile list) and composite_bwd_long_kernel (one segment of a long
// list) — walk with ONE wave64 for all 256 pixels of a tile: lane l owns (x, y), (x, y+4), (x, y+8), (x, y+12).  The LDS
// reads, the cross-lane reduction and the row store — ~60 % of the instructions of a visited (pixels, splat) pair — are
// then paid once for four pixels (measured at config 3: 1.115 / 0.975 / 0.917 ms for one / two / four pixels per lane).

// One 64-byte (:rgb 48-byte) gradient row per instance from its reduced sums r, plain stores, written for EVERY emitted
// instance exactly once per backward (zeros when no pixel touched it), so the row buffer needs no memset; the per-Gaussian
// kernel sums a Gaussian's rows in a fixed order — no fp32 atomics (35 M per view before), bit-reproducible gradients.
// a, b: planes 0 and 1 of the instance's stream entry; slot: its Gaussian-major row slot (uint bits).
template <int C, int VC>
__device__ __forceinline__ void bwd_store_row(float4* rows, const float4 a, const float4 b, float slot,
                                              const float (&r)[AccRow<VC>::N]) {
    constexpr int NA = AccRow<VC>::N;
    const float mo = -b.y, mh = -0.5f * b.y;  // vσ = -o·G·vα (render.jl:260)
    float4* row = rows + (size_t)GSR_ROW_F4(C) * __float_as_uint(slot);
    row[0] = make_float4(r[0], r[1], r[2], r[3]);
    row[1] = make_float4(mh * r[4], mh * r[5], mh * r[6], VC > 3 ? r[9 < NA ? 9 : 0] : 0.0f);
    // conic a = 2·ha, c = 2·hc (the stream carries the halves)
    row[2] = make_float4(mo * (2.0f * a.z * r[7] + a.w * r[8]), mo * (a.w * r[7] + 2.0f * b.x * r[8]),
                         VC > 5 ? r[10 < NA ? 10 : 0] : 0.0f, VC > 5 ? r[11 < NA ? 11 : 0] : 0.0f);
    if (C > 5) row[3] = make_float4(VC > 5 ? r[12 < NA ? 12 : 0] : 0.0f, 0.0f, 0.0f, 0.0f);
}

// Instances behind every pixel's last contributor are never staged: their rows are zero.  The wave's lanes take list
// positions p, p + 64, ... up to end.
template <int C>
__device__ __forceinline__ void bwd_zero_rows(float4* rows, const GsrStream stream, uint32_t p, uint32_t end) {
    for (; p < end; p += 64) {
        float4* row = rows + (size_t)GSR_ROW_F4(C) * __float_as_uint(stream.s2[p].y);
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        row[0] = z; row[1] = z; row[2] = z;
        if (C > 5) row[3] = z;
    }
}

// Stream entry p into slot k of a batch's LDS planes.  Plane 2 is staged as (third colour, footprint mask, depth | :rgb blend
// threshold, gradient-row slot): what a walk reads per splat is then one aligned 64-bit LDS read in :rgb mode.  Returns the
// footprint mask's bits.
template <int C>
__device__ __forceinline__ uint32_t bwd_stage_entry(const GsrStream& stream, uint32_t p, int k, float4* l0, float4* l1,
                                                    float4* l2, float4* l3) {
    l0[k] = stream.s0[p];
    l1[k] = stream.s1[p];
    const float4 t2 = stream.s2[p];
    l2[k] = make_float4(t2.x, t2.w, t2.z, t2.y);
    if (C > 3) l3[k] = stream.s3[p];
    return __float_as_uint(t2.w);
}

// The backward of a tile whose list is at most tiers.split_len long (the longer ones are composite_bwd_long_kernel's).
// BG0: the background is exactly (0, 0, 0) — the reference's default (rasterizer.jl:209) and what a trainer without a sky
// colour passes: the term -T_final/(1-α)·(bg·v) (render.jl:259) vanishes identically, and with it the per-pixel bgT state and
// one FMA per active visit.  WHO LAUNCHES WHAT (gsr_launch_composite_bwd, below; measured in
// profiles/r04/experiments/bwd_occupancy_ab.txt, A/B in one run):
//   C == 8 (:rgbdn): BG0 kernel WITH the rebuilt row coordinates (FY_REBUILD): 101 -> 94 VGPRs, four -> five waves per SIMD,
//                    0.907 -> 0.876 ms — launched whenever the background is zero;
//   C == 5 (:rgbd) : BG0 kernel WITHOUT the rebuilt coordinates: 88 -> 83 VGPRs, five waves as before, one FMA per active
//                    visit less, 0.720 -> 0.713 ms — launched whenever the background is zero (with the coordinates rebuilt it
//                    reaches 80 VGPRs = six waves and is 6 % SLOWER: 0.724 -> 0.770 ms);
//   C == 3 (:rgb)  : BG0 kernel whenever the background is zero and grad_precision is the default, PINNED AT SIX WAVES per SIMD
//                    through its register budget (composite_bwd_kernel_rgb_bg0, below), and with its instances reduced TWO AT A TIME (PAIR, in the
//                    kernel).  Left to itself the BG0 body has 70 VGPRs = seven waves and is slower than the general kernel
//                    (0.659 -> 0.676 ms; round 3's forced-occupancy probes: 789 / 735 / 677 / 695 us at 4 / 5 / 6 / 7 waves), which
//                    is why it was never launched before; pinned it is faster than the general kernel, and faster again with the
//                    paired reduction — 75 VGPRs, in the registers BG0 frees (profiles/bwd_zero_background/bench_ab.txt, DESIGN.md
//                    §4.1: parent, pinned, pinned + paired in the same sessions).  Same bits as the general kernel:
//                    fma(-0, rinv, d*T) = d*T, and the paired network adds what the unpaired one adds.  A non-zero background,
//                    the accurate kernels and the colour-only :rgbd / :rgbdn launches take the general kernel.
// VC: channels of the pixel cotangent that can be non-zero.  VC == 3 < C (the cotangent comes from the photometric loss head, which
// only sees features[1:3] — training.jl:656,684-685: depth / alpha / normal channels of vpixels are exact zeros and their feature
// gradients too): the pixels' cotangent state, the colour·v dot product and the reduction are the :rgb kernel's; the stream, the
// blend thresholds and the row layout stay the mode's.

// The walk itself is composite_bwd_body.inc, the text of both kernels below: as a function it is inlined with one VGPR more
// in six of the template's instantiations (profiles/bwd_zero_background/resource_usage.txt is taken with the text included).
// What it shares with composite_bwd_long_kernel — the per-pixel state, the decode and the visit of an instance, the one-at-a-time
// reduction — is text of its own (composite_bwd_state / _decode / _visit / _reduce.inc), included by both, for the same reason: each
// was tried as a function and changed the code of kernels it must not change (profiles/bwd_shared_visit/codegen_compare.txt).
template <int C, bool BG0, int VC = C, bool ACC = false>
__global__ __launch_bounds__(64, 1) void composite_bwd_kernel(int W, int H, int grid_x,
                                                 const uint32_t* __restrict__ tile_start,
                                                 const uint32_t* __restrict__ tile_order,
                                                 GsrStream stream, Bg bg,
                                                 const float* __restrict__ vpixels,
                                                 const uint32_t* __restrict__ n_contrib,
                                                 const float* __restrict__ final_T, GsrInst inst,
                                                 GsrTierLists tiers) {
    static_assert(!(C == 3 && BG0), ":rgb on a zero background is composite_bwd_kernel_rgb_bg0");
#include "composite_bwd_body.inc"
}
// :rgb on a zero background, default precision: the same walk with BG0 and PAIR, PINNED AT SIX WAVES per SIMD through its
// register budget.  amdgpu_waves_per_eu(6, 6): the allocator may use the 80 VGPRs of six waves and the kernel descriptor asks
// for at least the 73 that keep a seventh wave off the SIMD, so the kernel runs at the occupancy measured best for this walk
// whatever its register count.  (A kernel of its own, not an instantiation of the template above: the occupancy attribute
// __launch_bounds__(64, 1) expands to would win over a second one.)
// THE ROW-INDEPENDENT JOB: workgroups from job.first_wg on (none when job.n_wg == 0: the grid ends there) walk no tile.  They
// run bwd_row_job.h over a slice of the Gaussians — the direction Jacobian of the SH colour and the zero rows of culled
// Gaussians, for the per-Gaussian backward behind this launch — and return.  Launched behind the tile workgroups, which go
// longest list first, they take the wave slots that drain in the launch's last third and use the memory pipe this walk leaves
// idle.  (Defined at the end of this file, under `#pragma clang fp contract(off)`: pergauss.hip's floats.)
__device__ void bwd_row_job(const GsrRowJob& job, uint32_t w, int lane);
__global__ __attribute__((amdgpu_flat_work_group_size(1, 64), amdgpu_waves_per_eu(6, 6)))
void composite_bwd_kernel_rgb_bg0(int W, int H, int grid_x,
                                                 const uint32_t* __restrict__ tile_start,
                                                 const uint32_t* __restrict__ tile_order,
                                                 GsrStream stream, Bg bg,
                                                 const float* __restrict__ vpixels,
                                                 const uint32_t* __restrict__ n_contrib,
                                                 const float* __restrict__ final_T, GsrInst inst,
                                                 GsrTierLists tiers, GsrRowJob job) {
    constexpr int C = 3, VC = 3;
    constexpr bool BG0 = true, ACC = false;
    if (blockIdx.x >= job.first_wg) {
        bwd_row_job(job, blockIdx.x - job.first_wg, (int)threadIdx.x);
        return;
    }
#include "composite_bwd_body.inc"
}

// ---------------------------------------------------------------------------------
// backward of LONG lists, split along their LENGTH (round 5)
// ---------------------------------------------------------------------------------
// A list of tens of thousands of instances is serial for whoever walks it: the hot-tile scene's critical path was ONE wave of
// a neighbour of the hot tile visiting 15 000 entries that touch its 16x4 strip (profiles/r05/experiments/long_tiles.txt) —
// more waves per tile by PIXELS (round 2's four 16x4 strips per tile) do not help where one strip takes all the visits, and
// more waves in ONE workgroup stop at the four SIMDs of its CU (eight segment waves in one workgroup: 1.77 -> 1.24 ms only).
// Here a tile's list is cut into up to LONG_SEGS SEGMENTS, each walked by its own single-wave workgroup anywhere on the chip:
// a wave owns a contiguous run of list positions and ALL 256 pixels (four per lane, the main kernel's layout: row-then-column
// reduction, no cross-wave sums — each instance is reduced by exactly one wave and stored once).  The back-to-front recursions
// of a pixel (render.jl:237-258)
//     T <- T / (1 - alpha)           A <- alpha (colour . v) + (1 - alpha) A
// are affine in (T, A), so a segment's effect is (m, c) with m = prod (1 - alpha), c the A it leaves from A = 0:
//   PASS 1 (first launch): every wave walks its segment evaluating only the blend test, alpha and colour . v  ->  (m, c) per
//           pixel into `state` (global: [listed tile][segment][256 pixels][2]);
//   PASS 2 (second launch, same grid): wave g starts from  T = T_final / prod_{g' behind} m,  A = the composition of the
//           (m, c) behind it, and walks its segment again with the full gradient body.
// ~1.6 x the arithmetic of one walk, spread over the chip; no workgroup barrier anywhere.  The decisions (`bits(sigma) < X`,
// position < n_contrib) are the forward's, per pixel, as everywhere; what differs from the one-wave walk is the association of
// the products of (1 - alpha) across segment boundaries (last-bit level).
constexpr int LONG_SEGS = GSR_BWD_LONG_SEGS;

template <int C, bool BG0, int PASS>
__global__ __launch_bounds__(64) void composite_bwd_long_kernel(int W, int H, int grid_x,
                                                                const uint32_t* __restrict__ tile_start,
                                                                GsrStream stream, Bg bg,
                                                                const float* __restrict__ vpixels,
                                                                const uint32_t* __restrict__ n_contrib,
                                                                const float* __restrict__ final_T, GsrInst inst,
                                                                GsrTierLists tiers, float2* __restrict__ state) {
    // the names composite_bwd_visit.inc / composite_bwd_reduce.inc read: every channel, the fast exp and reciprocal, y per row,
    // one wave for all 16 rows of the tile
    constexpr int VC = C, BB = 64, ROWS = 16, wave = 0;
    constexpr bool ACC = false, FY_REBUILD = false;
    constexpr int NA = AccRow<C>::N, ST = AccRow<C>::STRIDE, PPL = 4;
    __shared__ float4 l0[BB], l1[BB], l2[BB];
    __shared__ float4 l3[C > 3 ? BB : 1];
    __shared__ float my[BB * ST];  // the wave's accumulator slab
    __builtin_amdgcn_s_setprio(3);  // these few waves are the critical path of the step; they share SIMDs with the main launch
    const int lane = threadIdx.x;
    const uint32_t listed = blockIdx.x / LONG_SEGS;
    const int g = (int)(blockIdx.x % LONG_SEGS);  // segment; g = 0 is the BACK of the list
    const gsr::LaneBits lane_bits(lane);
    const int red_slot = gsr::wave_reduce_index<NA>(lane);
    const bool red_writer = gsr::wave_reduce_writer(lane);
    const gsr::RowColConsts rowcol(lane);
    const gsr::RowColConstsD rowcol_d(lane);
    int tile;
    GSR_TIER_TILE(tile, tiers, listed);
    const int tile_x = tile % grid_x, tile_y = tile / grid_x;
    const int px = tile_x * GSR_TILE + (lane & 15);
    const int py0 = tile_y * GSR_TILE + (lane >> 4);
    const float fx = (float)px;
    const uint32_t start = tile_start[tile], end = tile_start[tile + 1];
    if (end == start) return;
    float fy[PPL], T[PPL], A[PPL], bgT[BG0 ? 1 : PPL], vp[PPL][C];
    int last_contributor[PPL];
#include "composite_bwd_state.inc"
    int tile_last = deepest;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tile_last = max(tile_last, __shfl_xor(tile_last, off));
    tile_last = __builtin_amdgcn_readfirstlane(tile_last);  // list positions tile_last-1 ... 0 are walked (the wave holds all 256 pixels)
    // segment g: positions [lo, hi), walked from hi - 1 down; whole 64-entry batches per segment
    const int seg = (((tile_last + LONG_SEGS - 1) / LONG_SEGS) + 63) & ~63;
    const int hi = tile_last - g * seg, lo = max(0, hi - seg);
    float2* const st_tile = state + (size_t)listed * LONG_SEGS * 256;
    if (PASS == 2 && g == 0) bwd_zero_rows<C>(inst.rows, stream, start + (uint32_t)tile_last + lane, end);  // once per tile
    if (hi <= 0) {  // an empty segment (a list shorter than LONG_SEGS batches): the identity
        if (PASS == 1) {
#pragma unroll
            for (int q = 0; q < PPL; q++) st_tile[(size_t)g * 256 + lane + 64 * q] = make_float2(1.0f, 0.0f);
        }
        return;
    }

    // one batch of <= 64 entries of the segment, staged into LDS; returns the candidate ballot
    auto stage = [&](int top /* first (highest) position of the batch + 1 */, int cnt) -> unsigned long long {
        __builtin_amdgcn_wave_barrier();  // the previous batch's LDS reads are done (single wave, in order)
        uint32_t mask = 0u;
        if (lane < cnt) mask = bwd_stage_entry<C>(stream, start + (uint32_t)(top - 1 - lane), lane, l0, l1, l2, l3);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        return wave_ballot(lane < cnt && (mask & 0xFFFFu) != 0u);
    };

    if (PASS == 1) {
        // ---- (m, c) of this segment, per pixel ----
        float m_[PPL], c_[PPL];
#pragma unroll
        for (int q = 0; q < PPL; q++) { m_[q] = 1.0f; c_[q] = 0.0f; }
        for (int top = hi; top > lo; top -= 64) {
            const int cnt = min(64, top - lo);
            unsigned long long wl = stage(top, cnt);
            while (wl) {
                const int j = __builtin_ctzll(wl);
                wl &= wl - 1;
                const int contributor = top - 1 - j;
#include "composite_bwd_decode.inc"
#pragma unroll
                for (int q = 0; q < PPL; q++) {
                    if (__builtin_amdgcn_readfirstlane((int)((entry_rowbits >> (4 * q)) & 0xFu)) == 0) continue;
                    const float dy = a.y - fy[q], dy2 = __fmul_rn(dy, dy);
                    const float sigma = sigma_of(sx, b.x, dy, dy2);
                    if (contributor < last_contributor[q] && __float_as_uint(sigma) < thr_bits) {
                        const float alpha = alpha_of(o, __expf(-sigma));
                        float cv = f[0] * vp[q][0];
#pragma unroll
                        for (int c = 1; c < C; c++) cv += f[c] * vp[q][c];
                        c_[q] = c_[q] + alpha * (cv - c_[q]);   // alpha cv + (1 - alpha) c: the A recursion from A = 0
                        m_[q] = m_[q] * (1.0f - alpha);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < PPL; q++) st_tile[(size_t)g * 256 + lane + 64 * q] = make_float2(m_[q], c_[q]);
        return;
    }

    // ---- PASS 2.  The state this segment starts from: everything BEHIND it (segments 0 .. g-1), back to front ----
    for (int k = 0; k < g; k++) {
#pragma unroll
        for (int q = 0; q < PPL; q++) {
            const float2 mc = st_tile[(size_t)k * 256 + lane + 64 * q];
            T[q] = T[q] / mc.x;               // (a pixel nothing of the segment blends into: m = 1, c = 0)
            A[q] = mc.x * A[q] + mc.y;
        }
    }
    // ---- the gradient walk of the segment: the main kernel's visit and reduction, text for text (ACC = false: one wave = the whole tile) ----
    for (int top = hi; top > lo; top -= 64) {
        const int cnt = min(64, top - lo);
        unsigned long long wl = stage(top, cnt);
        unsigned long long touched[1] = {0ull};
        while (wl) {
            const int j = __builtin_ctzll(wl);
            wl &= wl - 1;
            const int contributor = top - 1 - j;
#include "composite_bwd_visit.inc"
#include "composite_bwd_reduce.inc"
        }
        // flush: one gradient row per staged instance (zeros when nothing touched it), the main kernel's row format
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < cnt) {
            float r[NA];
            const bool hit = (touched[0] >> lane) & 1ull;
#pragma unroll
            for (int k = 0; k < NA; k++) r[k] = hit ? my[lane * ST + k] : 0.0f;
            bwd_store_row<C, C>(inst.rows, l0[lane], l1[lane], l2[lane].w, r);
        }
    }
}

// exactly zero (either sign) in every channel: the kernels' BG0 specialisation
bool bg_is_zero(const Bg& b) {
    for (int c = 0; c < 8; c++)
        if (b.v[c] != 0.0f) return false;
    return true;
}

Bg make_bg(const float* background, int channels) {
    Bg b;
    for (int c = 0; c < 8; c++) b.v[c] = (c < 3 && c < channels) ? background[c] : 0.0f;  // rasterizer.jl:411-414
    return b;
}

}  // namespace

void gsr_launch_composite_fwd(hipStream_t s, int channels, GsrCam cam, GsrTiles tiles, GsrStream stream, GsrFrame frame,
                              const GsrTierLists* only_listed) {
    const uint32_t* const tile_order = only_listed ? nullptr : tiles.order;
    const GsrTierLists tiers = only_listed ? *only_listed : GsrTierLists{};
    const int n_slots = tile_order ? cam.grid_x * cam.grid_y : (int)(tiers.n_big + tiers.n_mid8 + tiers.n_mid4);
    if (n_slots <= 0) return;
    dim3 grid(32 * ((n_slots + 7) / 8)), block(64);  // 8 XCD lanes x 4 strips per launch slot
    Bg bg = make_bg(frame.background, channels);
    gsr::dispatch_channels(channels, [&](auto c) {
        constexpr int CH = c;
        gsr::dispatch_bool(frame.covis || frame.uncert, [&](auto a) {
            constexpr bool AUX = a;
            if (frame.scores.any())
                hipLaunchKernelGGL((composite_fwd_strip_scored_kernel<CH, AUX>), grid, block, 0, s, cam.width, cam.height,
                                   cam.grid_x, tiles.start, tile_order, stream, bg, frame.image, frame.n_contrib, frame.final_T,
                                   frame.values_sorted, frame.covis, frame.uncert, tiers, frame.scores);
            else
            hipLaunchKernelGGL((composite_fwd_strip_kernel<CH, AUX>), grid, block, 0, s, cam.width, cam.height, cam.grid_x,
                               tiles.start, tile_order, stream, bg, frame.image, frame.n_contrib, frame.final_T,
                               frame.values_sorted, frame.covis, frame.uncert, tiers);
        });
    });
}

void gsr_launch_sort_composite_fwd(hipStream_t s, int channels, GsrCam cam, GsrTiles tiles, GsrKeys keys, GsrGeom geom,
                                   GsrStream stream, GsrFrame frame, uint32_t cap_instances, bool keep_backward_state) {
    dim3 grid(cam.grid_x * cam.grid_y), block(256);
    Bg bg = make_bg(frame.background, channels);
    gsr::dispatch_channels(channels, [&](auto c) {
        constexpr int CH = c;
        gsr::dispatch_bool(frame.covis || frame.uncert, [&](auto a) {
            constexpr bool AUX = a;
            gsr::dispatch_bool(keep_backward_state, [&](auto k) {
                constexpr bool KEEP = k;
                if (frame.scores.any())
                    hipLaunchKernelGGL((sort_composite_fwd_scored_kernel<CH, AUX, KEEP>), grid, block, 0, s, cam.width,
                                       cam.height, cam.grid_x, tiles.start, tiles.order, tiles.count, keys.bins, keys.cap, geom,
                                       stream, bg, frame.image, frame.n_contrib, frame.final_T, frame.values_sorted, tiles.ranges,
                                       frame.covis, frame.uncert, tiles.totals, cap_instances, frame.scores);
                else
                hipLaunchKernelGGL((sort_composite_fwd_kernel<CH, AUX, KEEP>), grid, block, 0, s, cam.width, cam.height,
                                   cam.grid_x, tiles.start, tiles.order, tiles.count, keys.bins, keys.cap, geom, stream, bg,
                                   frame.image, frame.n_contrib, frame.final_T, frame.values_sorted, tiles.ranges,
                                   frame.covis, frame.uncert, tiles.totals, cap_instances);
            });
        });
    });
}

bool gsr_launch_composite_bwd(hipStream_t s, int channels, GsrCam cam, GsrTiles tiles, GsrStream stream, GsrFrame frame,
                              const float* vpixels, GsrInst inst, const GsrRowJob* job, uint32_t split_len, bool color_only,
                              bool accurate) {
    dim3 grid(cam.grid_x * cam.grid_y), block(64);
    bool carried = false;
    Bg bg = make_bg(frame.background, channels);
    GsrTierLists none{};
    none.split_len = split_len;
    const bool bg0 = bg_is_zero(bg);
#define LAUNCH_K(CC, ZZ, VV, AA)                                                                                       \
    hipLaunchKernelGGL((composite_bwd_kernel<CC, ZZ, VV, AA>), grid, block, 0, s, cam.width, cam.height,               \
                       cam.grid_x, tiles.start, tiles.order, stream, bg, vpixels, frame.n_contrib, frame.final_T, inst, none)
    // accurate: the ACC instantiations (libm exp, IEEE division: gsr_config.grad_precision) — the general-background kernels only
#define LAUNCH2(CC, ZZ) do { if (accurate) LAUNCH_K(CC, false, CC, true); else LAUNCH_K(CC, ZZ, CC, false); } while (0)
    // the zero-background kernels where they pay (table above the kernel): every mode takes BG0 on a zero background, :rgb's
    // pinned at six waves through its register budget (capping it there with 1.25 KB of unused dynamic LDS per workgroup took
    // 0.738 ms: the code was still generated for seven waves' budget)
#define LAUNCH3(CC, ZZ) do { if (accurate) LAUNCH_K(CC, false, 3, true); else LAUNCH_K(CC, ZZ, 3, false); } while (0)
    // (written out: the instantiation set is irregular on purpose — no BG0 with ACC or for colour-only, VC = 3 only for colour-only)
    if (channels == 3) {
        if (bg0 && !accurate) {
            // the row-independent job rides this launch: job.n_wg workgroups behind the tiles'
            GsrRowJob j{};
            if (job && job->n > 0 && job->n_wg > 0) { j = *job; carried = true; }
            j.first_wg = grid.x;
            hipLaunchKernelGGL(composite_bwd_kernel_rgb_bg0, dim3(grid.x + j.n_wg), block, 0, s, cam.width, cam.height, cam.grid_x,
                               tiles.start, tiles.order, stream, bg, vpixels, frame.n_contrib, frame.final_T, inst, none, j);
        }
        else LAUNCH2(3, false);
    }
    else if (color_only) {
        // the cotangent of the loss head (channels >= 3 are zeros): the :rgb arithmetic on the mode's stream, the general kernel
        // (its BG0 form was never measured at a pinned occupancy)
        if (channels == 5) LAUNCH3(5, false); else LAUNCH3(8, false);
    }
    else if (channels == 5) { if (bg0) LAUNCH2(5, true); else LAUNCH2(5, false); }
    else if (bg0) LAUNCH2(8, true);
    else LAUNCH2(8, false);
#undef LAUNCH_K
#undef LAUNCH2
#undef LAUNCH3
    return carried;
}

void gsr_launch_composite_bwd_listed(hipStream_t s, int channels, GsrCam cam, GsrTiles tiles, GsrTierLists tiers,
                                     GsrStream stream, GsrFrame frame, const float* vpixels, GsrInst inst, float* long_state) {
    const uint32_t n_listed = tiers.n_big + tiers.n_mid8 + tiers.n_mid4;
    if (n_listed == 0) return;
    Bg bg = make_bg(frame.background, channels);
    dim3 grid(n_listed * LONG_SEGS), block(64);
    float2* st = reinterpret_cast<float2*>(long_state);
    gsr::dispatch_channels(channels, [&](auto c) {
        constexpr int CH = c;
        gsr::dispatch_bool(bg_is_zero(bg), [&](auto z) {
            constexpr bool BG0 = z;
            hipLaunchKernelGGL((composite_bwd_long_kernel<CH, BG0, 1>), grid, block, 0, s, cam.width, cam.height, cam.grid_x,
                               tiles.start, stream, bg, vpixels, frame.n_contrib, frame.final_T, inst, tiers, st);
            hipLaunchKernelGGL((composite_bwd_long_kernel<CH, BG0, 2>), grid, block, 0, s, cam.width, cam.height, cam.grid_x,
                               tiles.start, stream, bg, vpixels, frame.n_contrib, frame.final_T, inst, tiers, st);
        });
    });
}

// ---------------------------------------------------------------------------------
// The row-independent job of composite_bwd_kernel_rgb_bg0 (declared above it).  Last in the file: from here on no expression is
// contracted into FMAs, as in pergauss.hip, whose floats these are (bwd_row_job.h).
// ---------------------------------------------------------------------------------
#pragma clang fp contract(off)
#include "bwd_row_job.h"
namespace {
__device__ void bwd_row_job(const GsrRowJob& job, uint32_t w, int lane) { gsr::bwd_row_job_run(job, w, lane); }
}  // namespace
