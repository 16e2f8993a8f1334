// Internal interface between the C ABI (gsr_api.cpp) and the gfx950 kernels.
// Not installed; include/gsr.h is the public boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GSR_TILE 16         // GaussianSplatting.jl:55 BLOCK
#define GSR_BATCH 256       // GaussianSplatting.jl:56 BLOCK_SIZE
#define GSR_SORT_LDS_CAP 8192  // keys per tile sorted in LDS (64 KB); longer lists use the global path

// Camera + config constants, passed BY VALUE as a kernel argument (lands in SGPRs).
struct GsrCam {
    float R[9];  // row-major R[r*3+c] (converted from the ABI's column-major)
    float t[3];
    float focal[2];
    float principal[2];  // normalised
    float center[3];
    int width, height;
    int grid_x, grid_y;
    float near_plane, far_plane;
    int radius_clip;
    float blur_eps;
    int exact_cull;      // 1 = exact footprint culling (the default), 0 = the reference's lists (GSR_FLAG_REFERENCE_TILE_LISTS)
    const float* R_dev;  // optional device overrides (column-major (3,3), (3))
    const float* t_dev;
};

// Per-Gaussian geometry written by preprocess: ONE 64-byte record per Gaussian (a gather by
// id — the tile sort does 5.7 M of them per view — touches a single cache line).
//   q0 = mean2d.x, mean2d.y, conic.a, conic.b
//   q1 = conic.c, opacity, r, g
//   q2 = b, clamped bits (u32), depth, lpre (u32: exclusive prefix of tile-rect areas inside the
//        Gaussian's 256-wide block; + bpre[i >> 8] = Gaussian-major slot of its first instance)
//   q3 = rect xmin | ymin << 16, rect xmax | ymax << 16 (u32), blend-test threshold bits X (u32, tile_mask.h),
//        emitted-tile mask of the rect (u32, row-major bit per tile; meaningful for rects of <= 32 tiles: preprocess.hip DENSE_RECT)
struct GsrGeoRec { float4 q0, q1, q2, q3; };
// Tile rects of at most this many tiles get one gradient-row slot per EMITTED tile (ranked through the record's mask);
// larger ones one per tile of the rect (preprocess.hip: preprocess; pergauss.hip: pergauss_bwd; tile_sort_device.h: the emit's slot).
constexpr uint32_t GSR_DENSE_RECT = 32;
struct GsrGeom {
    GsrGeoRec* rec;
    float4* normal;   // camera-space normal (C == 8) or nullptr
    int32_t* radii;
    uint32_t* bsum;   // per 256-Gaussian block: sum of tile-rect areas (scanned into bpre by tile_scan)
    uint32_t* bpre;
};

// Sorted per-instance splat stream written by tile_sort (planes of float4, coalesced).
struct GsrStream {
    float4* s0;  // mean2d.x, mean2d.y, conic.a / 2, conic.b
    float4* s1;  // conic.c / 2, opacity, r, g
    float4* s2;  // b, slot (uint bits: Gaussian-major instance slot), depth | :rgb: blend-test threshold bits (tile_sort_device.h), row mask (uint bits: tile rows touched)
    float4* s3;  // :rgbd / :rgbdn: normal xyz (C == 8, else 0) + the blend-test threshold bits in w (tile_sort_device.h); :rgb: nullptr
};

// Backward: per-INSTANCE gradient rows (plain stores, no atomics), indexed by the
// Gaussian-major instance slot, so the rows of one Gaussian are contiguous and the
// per-Gaussian kernel sums them in a fixed order (deterministic gradients).
//   row = 4 x float4: {v r, v g, v b, v opacity}, {v conic a,b,c, v depth}, {v mean2d x,y, v normal x,y}, {v normal z,-,-,-}
// segments a long tile list is cut into by the list-parallel backward (composite_bwd_long_kernel)
#define GSR_BWD_LONG_SEGS 32
#define GSR_ROW_F4(C) ((C) > 3 ? 4 : 3)  // float4s per gradient row: 48 bytes in :rgb mode (9 floats used), 64 otherwise
struct GsrInst {
    float4* rows;  // D_slots x GSR_ROW_F4 float4; never cleared: composite_bwd stores the row of every emitted instance (gsr_backward)
};

// ---- what the launchers below share: plain bundles, unpacked by each launcher into its kernel's own parameter list ----
// The eight words tile_scan_kernel leaves in GsrTiles::totals (device) and mirrors into pinned host memory.
enum GsrTotal {
    GSR_TOTAL_D = 0,         // instances of the view (= tile_start[T])
    GSR_TOTAL_MAX_LIST = 1,  // longest tile list
    GSR_TOTAL_BIG = 2,       // tiles with a list over GSR_SORT_LDS_CAP (8192): tier_lists[0, T)
    GSR_TOTAL_MID4 = 3,      // tiles with a list in (1024, 4096]: tier_lists[2T, 3T)
    GSR_TOTAL_VISIBLE = 4,   // visible Gaussians; bit 31: one of them has a non-empty tile rect (the reference's D > 0)
    GSR_TOTAL_SLOTS = 5,     // sum of tile-rect areas = Gaussian-major instance slots (gradient rows); >= D
    GSR_TOTAL_MID8 = 6,      // tiles with a list in (4096, 8192]: tier_lists[T, 2T)
    GSR_TOTAL_SEQ = 7,       // device: the scan's ticket (zero between launches); host mirror: the forward's sequence number
    GSR_TOTAL_WORDS = 8
};
// The tile-side arrays of a view.
struct GsrTiles {
    uint32_t* start;       // [T + 1] exclusive scan of the counts
    uint32_t* count;       // [T] list lengths, counted by preprocess, re-zeroed by the sort for the next view
    uint32_t* order;       // [T] tile ids by descending list length: launch order of the compositing workgroups
    uint32_t* ranges;      // [2 T] identify_tile_range! (utils.jl:56-78)
    uint32_t* tier_lists;  // [3 T] written by tile_scan: [0, T) tiles with lists > 8192, [T, 2T) (4096, 8192], [2T, 3T) (1024, 4096]
    uint32_t* totals;      // [GSR_TOTAL_WORDS]
    int n_tiles, grid_x;
};
// Where a view's unsorted keys are.  cap > 0: keys of tile t at bins + t * cap — unless its list is longer than cap: the complete
// list is then at overflow + start[t]; cap == 0: compact layout, keys of tile t at bins + start[t].
struct GsrKeys { uint64_t* bins; uint32_t cap; const uint64_t* overflow /* or NULL */; };
// gsr_scores: the per-Gaussian contribution scores a scored forward accumulates into (composite.hip); any of them NULL
struct GsrScores {
    uint32_t* max_weight; unsigned long long* hits; unsigned long long* weight_sum;
    __host__ __device__ bool any() const { return max_weight || hits || weight_sum; }
};
// The frame a view renders into, and what the backward reads of it.
struct GsrFrame {
    const float* background;  // host, 3 floats
    float* image;             // (the backward launches do not touch it)
    uint32_t* n_contrib; float* final_T;
    uint32_t* values_sorted;  // sorted ids, per instance
    uint8_t* covis; float* uncert;  // gsr_aux.covisibilities / uncertainties, or NULL
    GsrScores scores;               // gsr_forward_scored's, or all NULL: the unscored kernels
};

// ---- preprocess.hip (compiled with -ffp-contract=off: bit-reproducible fp32) ----
// aggregating: the binning form gsr_policy_begin_view chose for this view (false = the direct form);
// returns the form that ran (gsr_stats.preprocess_form: 0 direct, 1 / 2 aggregating with 2 x 32 / 2 x 16-bit LDS words, 3 banded)
int gsr_launch_preprocess(hipStream_t s, int n, int K, int degree, int channels, const float* means,
                          const float* scales, const float* rots, const float* opac, const float* shs, GsrCam cam,
                          GsrGeom geom, GsrTiles tiles, uint32_t* n_visible /* per 256-block */,
                          GsrKeys keys /* (T+1) x cap keys; cap == 0: count only */, bool aggregating,
                          float* comp /* antialiased handle: add_blur's compensations (N), written where radii > 0, and the
                                         opacity of every later stage is opac * comp; NULL: the plain render */);
struct GsrBg8 { float v[8]; };
// compact binning mode: scatter the keys to tile_start[t] + arrival rank (tile_fill zeroed by the caller).
// only_above > 0: only the tiles whose list is LONGER than that (the lists that overflowed fixed-capacity bins) — the others'
// segments of `keys` and their fill cursors are not touched
void gsr_launch_emit_compact(hipStream_t s, int n, GsrCam cam, GsrGeom geom, const uint32_t* tile_start, uint32_t* tile_fill,
                             uint64_t* keys, uint32_t max_list /* longest tile list of the view */, uint32_t only_above);

// ---- pergauss.hip (-ffp-contract=off) ----
// per-workgroup partials of the pose gradient (12 floats per 256 Gaussians), summed in a fixed order by a finishing launch
inline size_t gsr_pose_partial_floats(int64_t n) { return n <= 0 ? 0 : (size_t)((n + 255) / 256) * 12; }
void gsr_launch_pergauss_bwd(hipStream_t s, int n, int K, int degree, int channels, const float* means,
                             const float* scales, const float* rots, const float* shs, GsrCam cam, GsrGeom geom,
                             GsrInst inst, float2* vmean2d, float* vmeans, float* vshs, float* vopac,
                             float* vscales, float* vrots, float* vR, float* vt /* both or neither */,
                             float* pose_part /* scratch of gsr_pose_partial_floats(n) floats, needed when vR is given */,
                             float* vcolors /* (3,N) or NULL: factored SH gradient instead of vshs */,
                             bool fp32_chain /* ∇scales / ∇rotations by the reference's fp32 trees (GSR_GRAD_FP32_REFERENCE) */,
                             const float* opac, const float* comp /* antialiased handle: the caller's opacities and the forward's
                                                                     compensations (∇add_blur joins both chains); else both NULL */,
                             const float* sh_jac /* the composite_bwd launch before carried the row-independent job (GsrRowJob): its
                                                    Jacobian buffer, read instead of the SH bands, and the rows of culled Gaussians
                                                    are left to the job; NULL: everything is this launch's */);
// backward epilogue = trainer tail (single-GPU step): no gradient arrays, the parameters / Adam states in S are
// updated in place and the activated copies of the next forward written (adam_math.h)
namespace gsr { struct TailState; }
void gsr_launch_pergauss_bwd_tail(hipStream_t s, int n, int K, int degree, int channels, GsrCam cam, GsrGeom geom,
                                  GsrInst inst, float2* vmean2d, const gsr::TailState& S, bool fp32_chain,
                                  const float* comp /* antialiased handle (the opacities are S.opac_act), or NULL */);
void gsr_launch_update_stats(hipStream_t s, int n, const int32_t* radii, const float2* vmean2d, int width, int height,
                             int32_t* max_radii, float* accum, float* denom);

// ---- sh_views.hip (-ffp-contract=off) ----
void gsr_launch_sh_grad_views(hipStream_t s, int n, int K, int degree, int n_views, const float* centers,
                              const float* means, const float* vc_all, float* vshs);
// the same rebuild with the trainer tail applied in place of the ∇shs store (multi-GPU trainer step; S.points = the means)
void gsr_launch_sh_views_tail(hipStream_t s, int n, int K, int degree, int n_views, const float* centers,
                              const float* vc_all, const float* vmeans, const float* vopac_act, const float* vscales_act,
                              const float* vrot, const gsr::TailState& S);

// ---- binning.hip ----
// exclusive scan of tiles.count -> tiles.start[T+1], and of the per-block rect-area sums geom.bsum[n_blocks] -> geom.bpre;
// tiles.totals (GsrTotal), tiles.tier_lists and tiles.order, the last by a third workgroup of the same launch
void gsr_launch_tile_scan(hipStream_t s, GsrTiles tiles, GsrGeom geom, int n_blocks, const uint32_t* bvis,
                          uint32_t* host_mirror /* pinned host: the totals + seq in [GSR_TOTAL_SEQ], or NULL */, uint32_t seq);
// The sorts the fused launch (gsr_launch_sort_composite_fwd) leaves, after the host has read the scan's totals:
// main_pass: one wave per tile over every list of up to 1024 keys — a view the fused launch did not take; it also writes
// tiles.ranges and re-zeroes tiles.count.  Always: one launch per non-empty tier list (the counts are host-side numbers), less
// the first4 / first8 leading tiles of the two mid tiers that gsr_launch_tile_sort_mid has already sorted.
void gsr_launch_tile_sort(hipStream_t s, int channels, bool main_pass, GsrTiles tiles, GsrKeys keys, uint32_t n_mid4,
                          uint32_t n_mid8, uint32_t n_big, uint32_t first4, uint32_t first8,
                          uint64_t* big_scratch /* 2 slabs of slab_stride keys per tile over 8192 */, size_t slab_stride,
                          GsrGeom geom, GsrStream stream, uint32_t* values_sorted);
// the sorts of the (1024, 4096] / (4096, 8192] tiers launched BEFORE the host has the counts: grids are guesses, every workgroup
// checks tiles.totals — instances <= cap_instances, longest list <= keys.cap, its slot < the tier's count — else leaves
void gsr_launch_tile_sort_mid(hipStream_t s, int channels, GsrTiles tiles, GsrKeys keys, uint32_t grid4, uint32_t grid8,
                              GsrGeom geom, GsrStream stream, uint32_t* values_sorted, uint32_t cap_instances);

// ---- composite.hip ----
void gsr_launch_fill_background(hipStream_t s, size_t n_pixels, int channels, GsrFrame frame);  // (defined in binning.hip)
// Tiles whose list is longer than split_len (a tier boundary of the scan: 1024, 4096, 8192, or 0xFFFFFFFF for none)
// are left out by gsr_launch_composite_bwd and walked by four waves each (one 16x4 pixel strip per wave) in the
// listed launch, on a second stream.
struct GsrTierLists {  // the scan's tier lists: [0, T) lists > 8192, [T, 2T) (4096, 8192], [2T, 3T) (1024, 4096]
    const uint32_t* lists;
    uint32_t n_tiles, n_big, n_mid8, n_mid4;  // a tier that is not split has count 0 here
    uint32_t split_len;  // (forward launch over the lists: non-zero = its waves run at raised issue priority, beside another launch)
};
// tile = the tile of listed slot `slot` < n_big + n_mid8 + n_mid4 (the three lists back to back, longest tier first).  A statement,
// not a function: composite.hip's forward kernel schedules its prologue differently around an inlined call, in every form tried
// (profiles/bwd_shared_visit/codegen_compare.txt).
#define GSR_TIER_TILE(tile, tiers, slot)                                                                                       \
    do {                                                                                                                       \
        uint32_t b_ = (slot);                                                                                                  \
        const uint32_t* list_ = (tiers).lists;                                                            /* lists > 8192 */   \
        if (b_ >= (tiers).n_big) { b_ -= (tiers).n_big; list_ = (tiers).lists + (tiers).n_tiles;          /* (4096, 8192] */   \
            if (b_ >= (tiers).n_mid8) { b_ -= (tiers).n_mid8; list_ = (tiers).lists + 2 * (size_t)(tiers).n_tiles; } }  /* (1024, 4096] */ \
        (tile) = (int)list_[b_];                                                                                               \
    } while (0)
void gsr_launch_composite_fwd(hipStream_t s, int channels, GsrCam cam, GsrTiles tiles, GsrStream stream, GsrFrame frame,
                              const GsrTierLists* only_listed /* NULL: every tile, in tiles.order */);
// sort + forward of every tile in one launch (fixed-capacity bins, no list beyond 1024 instances; checked on the
// device against the scan's totals — a view that does not qualify leaves everything untouched)
void gsr_launch_sort_composite_fwd(hipStream_t s, int channels, GsrCam cam, GsrTiles tiles, GsrKeys keys, GsrGeom geom,
                                   GsrStream stream, GsrFrame frame, uint32_t cap_instances,
                                   bool keep_backward_state /* false (GSR_FORWARD_ONLY): the sorted stream and ids are not stored */);
// The row-independent job (bwd_row_job.h): n_wg extra single-wave workgroups behind the tile workgroups of the :rgb
// zero-background launch, `slice` Gaussians each (gsr_policy_bwd_row_job).  Of a visible Gaussian they store the nine floats of
// d rgb / d dir (splat_math.h: sh_dir_jacobian) into jac, of a culled one the zero rows of every gradient array — what the
// per-Gaussian backward otherwise does from the SH bands, in a kernel that leaves the memory pipe idle.
struct GsrRowJob {
    uint32_t first_wg;      // the tile workgroups of the launch: the job's are first_wg ... first_wg + n_wg - 1
    uint32_t n_wg, slice;   // n_wg * slice >= n
    int n, K, degree;
    const float* means; const float* shs; const int32_t* radii;
    float center[3];        // the camera centre (view_dir)
    float* jac;             // 9 floats per Gaussian, written where radii > 0 (degree > 0)
    float* vmeans; float* vshs; float* vopac; float* vscales; float4* vrots;  // zeros where radii <= 0
};
// returns whether the launch carried `job` (the :rgb zero-background kernel at the default precision only; else it is ignored)
bool gsr_launch_composite_bwd(hipStream_t s, int channels, GsrCam cam, GsrTiles tiles, GsrStream stream, GsrFrame frame,
                              const float* vpixels, GsrInst inst, const GsrRowJob* job /* or NULL */,
                              uint32_t split_len /* tiles with a longer list are left to the listed launch */,
                              bool color_only /* channels >= 3 of vpixels are zeros (the loss head's cotangent) */,
                              bool accurate /* libm exp + IEEE division per pixel (gsr_config.grad_precision); the caller then
                                               leaves EVERY tile to this launch (split_len = 0xFFFFFFFF) */);
void gsr_launch_composite_bwd_listed(hipStream_t s, int channels, GsrCam cam, GsrTiles tiles, GsrTierLists tiers,
                                     GsrStream stream, GsrFrame frame, const float* vpixels, GsrInst inst,
                                     float* long_state /* GSR_BWD_LONG_SEGS x 512 floats per listed tile */);

// ---- trainer.hip ----
#define GSR_ADAM_MAX_GROUPS 8
void gsr_launch_prologue_fwd(hipStream_t s, int n, int k_rest, int scale_dims, const float* sh_color,
                             const float* sh_remainder, const float* opacities, const float* scales, float* shs,
                             float* opacities_act, float* scales_act);
void gsr_launch_prologue_bwd(hipStream_t s, int n, int k_rest, int scale_dims, const float* opacities_act,
                             const float* scales_act, const float* vshs, const float* vopacities_act,
                             const float* vscales_act, float* v_sh_color, float* v_sh_remainder, float* v_opacities,
                             float* v_scales);
void gsr_launch_adam(hipStream_t s, int n_groups, float* const* theta, const float* const* grad, float* const* mu,
                     float* const* nu, const long long* count, const float* lr_t, float beta1, float beta2, float eps);

void gsr_launch_trainer_tail(hipStream_t s, int n, int k_rest, int scale_dims, const float* const* grads,
                             float* const* theta, float* const* mu, float* const* nu, const float* lr_t, float beta1,
                             float beta2, float eps, float* shs, float* opac_act, float* scales_act);
size_t gsr_findall_scratch_bytes(long long n);
void gsr_launch_findall(hipStream_t s, long long n, const uint8_t* mask, uint32_t* indices, uint32_t* count_dev,
                        uint32_t* scratch);
void gsr_launch_gather_rows(hipStream_t s, int n_groups, const void* const* src, void* const* dst, const int* row_words,
                            const uint32_t* idx, long long count);
void gsr_launch_triad(hipStream_t s, size_t n4, float* a, const float* b, const float* c, float q);

// ---- densify.hip (compiled with -ffp-contract=off) ----
#define GSR_COMPOSE_MAX_GROUPS 24
void gsr_launch_grad_mean(hipStream_t s, long long n, const float* accum, const float* denom, float* out);
void gsr_launch_densify_mask(hipStream_t s, int kind, long long n, long long n_grad, const float* grad, const float* scales,
                             int scale_dims, const float* opacities, const int32_t* max_radii, float thr, float gamma,
                             float min_opacity, int max_screen_size, uint8_t* mask);
// valid[i] = score[i] >= threshold as unsigned integers; words = 1: uint32 scores, 2: uint64 (gsr_contribution_mask)
void gsr_launch_contribution_mask(hipStream_t s, long long n, int words, const void* score, unsigned long long threshold,
                                  uint8_t* valid);
void gsr_launch_compose_rows(hipStream_t s, int n_groups, const void* const* src, void* const* dst, const int* row_words,
                             const int* new_zero, const uint32_t* keep_idx, long long n_keep, const uint32_t* sel_idx,
                             long long n_sel, int reps);
void gsr_launch_split_transform(hipStream_t s, long long n_new, int scale_dims, float* points, const float* rots,
                                float* scales, uint32_t seed);
void gsr_launch_reset_opacity(hipStream_t s, long long n, float* opacities);
void gsr_launch_morton_codes(hipStream_t s, long long n, const float* points, const float lo[3], const float inv_extent[3],
                             unsigned long long* codes);
void gsr_launch_nonfinite_scan(hipStream_t s, int n_groups, const float* const* src, const int* row_words, long long n_rows,
                               uint32_t* counts, uint32_t* first_bad);
void gsr_launch_ply_rows(hipStream_t s, bool pack, long long n, int kr, float* points, float* dc, float* rest, float* opac,
                         float* scales, float* rots, float* rows);

// ---- mcmc.hip (compiled with -ffp-contract=off): the MCMC densification strategy ----
void gsr_launch_mcmc_weights(hipStream_t s, long long n, int scale_dims, const float* opac, const float* scales, float min_opacity,
                             float log_max_scale, uint32_t* q, uint8_t* dead);
size_t gsr_mcmc_sample_scratch_words(long long n);  // 8-byte words
void gsr_launch_mcmc_sample(hipStream_t s, long long n, const uint32_t* q, long long m, uint32_t seed, uint32_t* sampled,
                            int32_t* counts, unsigned long long* total, unsigned long long* scratch);
void gsr_launch_mcmc_split_sampled(hipStream_t s, long long n, int scale_dims, const int32_t* counts, const float* binoms, int n_max,
                                   float min_opacity, float* opac, float* scales);
void gsr_launch_mcmc_relocation_params(hipStream_t s, long long m, const float* o, const int32_t* ratio, const float* binoms,
                                       int n_max, float min_opacity, float* new_o, float* coeff);
void gsr_launch_mcmc_relocate_rows(hipStream_t s, int n_groups, void* const* x, const int* row_words, const int* new_zero,
                                   long long n, const uint32_t* dead, const uint32_t* sampled, long long m);
void gsr_launch_mcmc_inject_noise(hipStream_t s, long long n, int scale_dims, float* points, const float* opac, const float* scales,
                                  const float* rots, float lr, float max_kick, uint32_t seed);
size_t gsr_mcmc_regularization_scratch_floats(long long n);
void gsr_launch_mcmc_regularization(hipStream_t s, long long n, int scale_dims, const float* opac, const float* scales,
                                    float opacity_reg, float scale_reg, float* loss_out, float* vopac, float* vscales,
                                    float* scratch);

// ---- ssim.hip (compiled twice: *_exact = -ffp-contract=off + IEEE divisions, bit-exact vs the oracle; *_fast = contracted
// multiply-adds + hardware reciprocals, the default path; gsr_ssim_precision selects) ----
#define GSR_SSIM_DECL(SUF)                                                                                              \
    void gsr_launch_ssim_fwd_##SUF(hipStream_t s, int W, int H, int CH, int B, const float* img, const float* ref, float C1, \
                                   float C2, int train, float* ssim_map, float* d0, float* d1, float* d2);             \
    void gsr_launch_ssim_bwd_##SUF(hipStream_t s, int W, int H, int CH, int B, const float* img, const float* ref,      \
                                   const float* dL_dmap, const float* d0, const float* d1, const float* d2, float* dL_dimg); \
    /* fused loss head: image (C,W,H) vs target (W,H,3); partial: [gsr_loss_partial_pairs][2] per-wave sum|x-y|, sum ssim */ \
    size_t gsr_loss_partial_pairs_##SUF(int W, int H);                                                                 \
    void gsr_launch_loss_fwd_##SUF(hipStream_t s, int W, int H, int C, const float* image, const float* target, float C1, \
                                   float C2, float* d0, float* d1, float* d2, float* partial);                         \
    void gsr_launch_loss_bwd_##SUF(hipStream_t s, int W, int H, int C, const float* image, const float* target, float lambda, \
                                   const float* d0, const float* d1, const float* d2, const float* partial, float* loss_out, \
                                   float* vpixels);
GSR_SSIM_DECL(exact)
GSR_SSIM_DECL(fast)
#undef GSR_SSIM_DECL

// ---- bilateral.hip (compiled with -ffp-contract=off) ----
namespace gsr {
struct AdamHyper;
// constants of the TV prior (bilateral_grid.jl:106-119), evaluated once on the host for every kernel that uses them:
// term = weight · ((Sx/nx + Sy/ny) + Sz/nz) / n12, ∂term/∂θ = weight · ((tx·rx + ty·ry) + tz·rz)
struct BilateralTv { float weight, nx, ny, nz, n12, rx, ry, rz; };
}
int gsr_bilateral_chunks(int W, int H, int gx, int gy);
size_t gsr_bilateral_partial_bytes(int W, int H, int gx, int gy, int gz);
void gsr_launch_bilateral_fwd(hipStream_t s, int W, int H, int C, const float* image, const float* grid, int gx, int gy,
                              int gz, float* out);
void gsr_launch_bilateral_bwd(hipStream_t s, int W, int H, int C, const float* image, const float* grid, int gx, int gy,
                              int gz, const float* vout, float* vimage, float* vgrid, float* partial);
void gsr_launch_bilateral_tv(hipStream_t s, int n, int gx, int gy, int gz, const float* grids, const gsr::BilateralTv& tv,
                             float* loss_out, float* grad_out, float* partial);
void gsr_launch_bilateral_adam_tail(hipStream_t s, int n, int gx, int gy, int gz, float* grids, float* mu, float* nu,
                                    const float* vgrid, int view, const gsr::BilateralTv& tv, const gsr::AdamHyper& h,
                                    float* tv_loss_out, float* partial);

// ---- geometry.hip (compiled with -ffp-contract=off): depth-normal consistency and flatten losses ----
size_t gsr_normal_loss_scratch_floats(int W, int H);
void gsr_launch_normal_loss_fwd(hipStream_t s, int W, int H, const float* image, const float* focal, const float* principal,
                                float weight, float* loss_out, float* stats_out, float* weights_out, float* scratch);
void gsr_launch_normal_loss_bwd(hipStream_t s, int W, int H, const float* image, const float* focal, const float* principal,
                                float weight, float* vpixels, const float* scratch);
size_t gsr_flatten_loss_scratch_floats(int64_t n);
void gsr_launch_flatten_loss(hipStream_t s, int n, int scale_dims, const float* scales, float weight, float* loss_out,
                             float* vscales, float* scratch);

// ---- depth.hip (compiled with -ffp-contract=off): anchored depth supervision; `anchor` = the 5 floats of gsr_depth_anchor ----
size_t gsr_depth_loss_scratch_size(int W, int H);
void gsr_launch_depth_target(hipStream_t s, int W, int H, const float* prior, const float* anchor, float qstep, float* target_out,
                             float* half_band_out, uint8_t* flags_out);
void gsr_launch_depth_loss_fwd(hipStream_t s, int W, int H, int C, const float* image, const float* prior, const float* anchor,
                               float qstep, float lambda_grad, float weight, float* loss_out, float* stats_out, float* target_out,
                               float* half_band_out, uint8_t* flags_out, void* scratch);
void gsr_launch_depth_loss_bwd(hipStream_t s, int W, int H, int C, const float* image, float lambda_grad, float weight,
                               float* vpixels, const void* scratch);

// ---- sky.hip (compiled with -ffp-contract=off): sky-dome composite, sky-mask loss and their pullback ----
size_t gsr_sky_scratch_size(int W, int H);
void gsr_launch_sky_composite_fwd(hipStream_t s, int W, int H, int C, const float* image, const float* sky_rgb,
                                  const float* sky_weight, float loss_weight, float* out, float* loss_out, void* scratch);
void gsr_launch_sky_composite_bwd(hipStream_t s, int W, int H, int C, const float* image, const float* sky_rgb,
                                  const float* sky_weight, float loss_weight, float* vpixels, float* vsky, const void* scratch);

// ---- eval.hip (compiled with -ffp-contract=off): 8-bit SSIM / MSE / PSNR / L1 of a frame, and its RGB8 export ----
size_t gsr_eval_scratch_size(int W, int H);
void gsr_launch_eval_metrics(hipStream_t s, int W, int H, int C, const float* image, const float* sky_rgb,
                             const float* target_f32, const unsigned char* target_u8, int quantize, float* ssim_map, float* out,
                             void* scratch);
void gsr_launch_frame_rgb8(hipStream_t s, int W, int H, int C, const float* image, const float* sky_rgb, int flip_rows,
                           unsigned char* rgb8_out);

// ---- knn.hip (compiled with -ffp-contract=off): exact 3-NN of a point cloud and the initial scales from it ----
size_t gsr_knn_scratch_size(long long n);
void gsr_launch_knn_scales(hipStream_t s, long long n, const float* points, const int32_t* order, float point_size,
                           int scale_dims, float* scales_out, float* dist2_out, void* scratch);

// ---- filter3d.hip (compiled with -ffp-contract=off): the 3-D smoothing filter — camera sweep, apply and its pullback ----
size_t gsr_filter3d_scratch_size(long long n);
void gsr_launch_filter3d_compute(hipStream_t s, long long n, const float* points, int n_cameras, const float* cams,
                                 float near_plane, float k, float* filter, uint8_t* seen, uint32_t* count, void* scratch);
void gsr_launch_filter3d_apply(hipStream_t s, long long n, const float* opac, const float* scales, const float* filter, int raw,
                               float* opac_out, float* scales_out);
void gsr_launch_filter3d_apply_bwd(hipStream_t s, long long n, const float* opac, const float* scales, const float* filter,
                                   const float* g_opac, const float* g_scales, float* v_opac, float* v_scales);

// ---- vq.hip (compiled with -ffp-contract=off): SH codebook k-means — nearest code on the f32 MFMA, integer sums, update, decode ----
size_t gsr_vq_scratch_size(int n_codes, int dim);
void gsr_launch_vq_assign(hipStream_t s, int n, int n_codes, int dim, const float* rows, const float* codebook,
                          const uint16_t* prev, uint16_t* indices, float* err, uint32_t* changed, void* scratch);
void gsr_launch_vq_accumulate(hipStream_t s, int n, int n_codes, int dim, const float* rows, const uint16_t* indices,
                              const uint8_t* wq, long long* sums, unsigned long long* wsum);
void gsr_launch_vq_update(hipStream_t s, int n_codes, int dim, const long long* sums, const unsigned long long* wsum,
                          float* codebook, uint32_t* empty);
void gsr_launch_vq_decode(hipStream_t s, int n, int n_codes, int dim, const float* codebook, const uint16_t* indices,
                          float* rows_out);

// ---- vq_grad.hip (compiled with -ffp-contract=off): SH codebook fine-tuning — the stable grouping of the rows by code, the fixed-order per-code gradient sums ----
size_t gsr_vq_group_scratch_size(long long n, int n_codes);
void gsr_launch_vq_group(hipStream_t s, int n, int n_codes, const uint16_t* indices, uint32_t* order, uint32_t* offsets,
                         void* scratch);
size_t gsr_vq_codebook_grad_scratch_size(long long n, int n_codes, int dim);
void gsr_launch_vq_codebook_grad(hipStream_t s, int n, int n_codes, int dim, const float* g_rows, long long row_stride,
                                 const uint32_t* order, const uint32_t* offsets, float* g_codebook, void* scratch);

// ---- quant.hip (compiled with -ffp-contract=off): the quantised model container — block ranges, 8/16-bit codes, the decode, the one-launch fake pass ----
void gsr_launch_quant_ranges(hipStream_t s, long long n, int cols, const float* rows, int block_rows, float* ranges);
void gsr_launch_quant_encode(hipStream_t s, long long n, int cols, int bits, int kind, const float* rows, int block_rows,
                             const float* ranges, void* codes);
void gsr_launch_quant_decode(hipStream_t s, long long n, int cols, int bits, int kind, const void* codes, int block_rows,
                             const float* ranges, float* rows_out);
void gsr_launch_quant_fake(hipStream_t s, int n_groups, long long n, const float* const* in, float* const* out,
                           const float* const* ranges, const int* cols, const int* bits, const int* kind, const int* block_rows);

// ---- tsdf.hip (compiled with -ffp-contract=off): TSDF fusion of a rendered frame, surface-nets count and emit ----
// the volume: nx x ny x nz samples, sample (i, j, k) at o + h*(i, j, k)
struct GsrTsdfGrid {
    int nx, ny, nz;
    float o[3];
    float h;
};
// world->camera R (column-major as in the ABI) and t, the focal lengths, the principal point in pixels
struct GsrTsdfCam {
    float R[9];
    float t[3];
    float fx, fy, cx, cy;
};
size_t gsr_mesh_scratch_size(int nx, int ny, int nz);
void gsr_launch_tsdf_integrate(hipStream_t s, const GsrTsdfGrid& g, const GsrTsdfCam& c, int W, int H, int C, const float* image,
                               float min_alpha, float near_plane, float trunc, float* volume, float* color);
void gsr_launch_mesh_count(hipStream_t s, const GsrTsdfGrid& g, const float* volume, uint32_t* counts, void* scratch);
void gsr_launch_mesh_emit(hipStream_t s, const GsrTsdfGrid& g, const float* volume, const float* color, const void* scratch,
                          long long max_vertices, long long max_faces, float* vertices, float* vertex_colors, int32_t* faces);
