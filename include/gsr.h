/*
 * gsr.h — C ABI of libgsr_hip.so, the MI355X (gfx950) drop-in for the differentiable
 * rasterizer of GaussianSplatting.jl.
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * reference repository, `src/rasterization/` unless stated).  Conventions:
 *   - every pointer marked "device" is a HIP device address owned by the caller; the
 *     library never frees or retains it beyond the call;
 *   - array layouts are the reference's (Julia column-major): means (3,N), scales (3,N),
 *     rotations (4,N) as (w,x,y,z), opacities (1,N), shs (3,K,N), image (C,W,H) channel
 *     fastest, n_contrib / final_T (W,H) x fastest, tile_ranges (2,T);
 *   - all work is enqueued on the `stream` argument (a hipStream_t passed as void*);
 *     the only host synchronisation in steady state is the instance-count read-back inside
 *     gsr_forward (the reference has the same one: rasterizer.jl:337).  Scratch is grow-only
 *     (rasterizer.jl:275-278,340-343): a call that has to GROW a scratch buffer (first view, more
 *     Gaussians, a much denser view) frees and reallocates it with hipFree / hipMalloc, which
 *     synchronise the device — exactly where the reference reallocates;
 *   - every function returns 0 on success or a negative GSR_E_* code; no C++ exception
 *     crosses this boundary; gsr_last_error_string() describes the last failure on the
 *     calling thread;
 *   - a handle supports one outstanding forward -> backward pair (as the reference's
 *     GaussianRasterizer object does, rasterizer.jl:13-15); distinct handles are
 *     independent.
 */
#ifndef GSR_H
#define GSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_API __attribute__((visibility("default")))

enum {
    GSR_OK = 0,
    GSR_E_INVALID_ARG = -1, /* reference: @assert / error() in rasterizer.jl:51,66-68,281 */
    GSR_E_OOM = -2,
    GSR_E_HIP = -3,         /* a HIP runtime call failed */
    GSR_E_STATE = -4        /* backward without a matching forward */
};

/* Number of blended feature channels (rasterizer.jl:47-51 `n_color_features`). */
enum { GSR_MODE_RGB = 3, GSR_MODE_RGBD = 5, GSR_MODE_RGBDN = 8 };

/* Replaces the keyword arguments of `GaussianRasterizer(kab; width, height, mode,
 * near_plane, far_plane)` (rasterizer.jl:60-65) and the constants hard-coded in
 * `rasterize` (radius_clip = 3, blur_eps = 0.3: rasterizer.jl:294-295,505).  Unlike the
 * reference (rasterizer.jl:66) width/height need not be multiples of 16: partial tiles
 * are masked. */
typedef struct gsr_config {
    int32_t width, height;
    int32_t mode;        /* GSR_MODE_* */
    float near_plane;    /* 0.2  */
    float far_plane;     /* 1000 */
    int32_t radius_clip; /* 3 px */
    float blur_eps;      /* 0.3  */
    uint32_t flags;      /* GSR_FLAG_* */
    uint64_t bins_budget_bytes; /* 0 = default.  Cap on the fixed-capacity per-tile key bins of the fast binning mode
                          * ((tiles+1) x capacity x 8 B); default max(512 MiB, 160 B x instance count of the last view).
                          * Where bins for the longest list would exceed it — a few very deep tiles — the bins are sized for the
                          * other tiles (4 x the mean list, at least 1024 keys) and only the lists beyond that capacity are
                          * scattered a second time (+ 8 B per instance); a budget below bins of 2 x the mean list (or of 64
                          * keys) selects the compact mode (count -> scan -> scatter, 8 B per instance, no bins).  Same lists,
                          * same results in every mode. */
    /* The behaviour switches are PER HANDLE (ABI 5), as the reference's knobs are constructor keywords (rasterizer.jl:60-65).
     * ABI 6: 0 = GSR_DEFAULT everywhere, so that a zero-initialised (memset) gsr_config means "the defaults" — under ABI 5's
     * encoding (-1 default, 0 / 1 explicit) it silently pinned fast SSIM and direct binning.  GSR_DEFAULT follows the
     * process-wide default (gsr_ssim_precision / gsr_preprocess_form below, themselves started from GSR_SSIM_EXACT /
     * GSR_PREPROCESS_AGG), read at every call; an explicit value pins the handle whatever another thread sets process-wide —
     * e.g. a GUI render worker next to a trainer (gui/worker.jl:47-58).  Other values: GSR_E_INVALID_ARG. */
    int32_t ssim_precision;  /* arithmetic of gsr_loss_l1_ssim on this handle: GSR_DEFAULT, GSR_SSIM_FAST, GSR_SSIM_EXACT */
    int32_t preprocess_form; /* binning form of gsr_forward on this handle: GSR_DEFAULT (by size), GSR_PREPROCESS_DIRECT,
                              * GSR_PREPROCESS_AGGREGATING */
    /* New in ABI 6 */
    int32_t form_tuner;      /* on 4K-class grids, where neither binning form wins everywhere, the handle times four views'
                              * first kernel (two per form) and keeps the faster form (gsr_policy.h; results are bit-identical
                              * either way): GSR_DEFAULT (on; GSR_FORM_TUNER=0 in the environment turns the default off),
                              * GSR_TUNER_OFF (the previous view's skew decides, as before the tuner existed), GSR_TUNER_ON.
                              * An explicit preprocess_form pins the form and leaves the tuner nothing to decide. */
    int32_t grad_precision;  /* arithmetic of gsr_backward where fp32 shortcuts show on needle-shaped splats (2-D axis ratio beyond
                              * ~10 : 1), whose sums cancel by up to the square of that ratio:
                              *   GSR_DEFAULT: (i) ∇render!'s per-pixel exp / reciprocal are the hardware's fast instructions
                              *     (v_exp_f32 on sigma x log2 e, v_rcp_f32); (ii) the chain of ∇scales / ∇rotations (∇inverse ->
                              *     ∇perspective -> ∇covar_world_to_cam -> ∇quat_scale_to_cov -> ∇unnorm_quat2rot, projection.jl:132-257,
                              *     render.jl:302-366) is evaluated in float64 from the raw inputs.  ∇means of a 90 : 1 needle of
                              *     radius 100 px is then ~4e-4 from float64 (the reference's fp32 atomics: 0.2 .. 3e-4), everything
                              *     well conditioned ~1e-6;
                              *   GSR_GRAD_ACCURATE: (i) libm-accurate exp and IEEE division — what the reference's source means by
                              *     `exp` and `/` (render.jl:236-259) — with (ii) unchanged: the closest to float64 the library gets
                              *     (that needle: 2e-5); ∇render! +12 %, and long tile lists are not split along their length;
                              *   GSR_GRAD_FP32_REFERENCE: (i) as GSR_GRAD_ACCURATE, (ii) the reference's own fp32 expression trees,
                              *     operation for operation: reference-parity runs (equal to the fp32 CPU oracle to ~1e-6 on
                              *     well-conditioned Gaussians; on needles ∇rotations carry the fp32 chain's 1e-4 .. 1e-3). */
} gsr_config;
#define GSR_DEFAULT 0
enum { GSR_SSIM_FAST = 1, GSR_SSIM_EXACT = 2 };
enum { GSR_PREPROCESS_DIRECT = 1, GSR_PREPROCESS_AGGREGATING = 2 };
enum { GSR_TUNER_OFF = 1, GSR_TUNER_ON = 2 };
enum { GSR_GRAD_FP32_REFERENCE = 1, GSR_GRAD_ACCURATE = 2 };

/* Tile lists.  DEFAULT (flags = 0): exact footprint culling at binning — a (Gaussian, tile)
 * instance none of whose pixels can reach alpha >= 1/255 is not emitted at all.  The reference
 * emits it and then skips it pixel by pixel (render.jl:95), so the image, final_T, every
 * gradient, radii and ∇means_2d are unchanged (image / final_T bit-identical, tested at 1 M
 * Gaussians); only the INTERNAL lists shrink: gsr_stats.n_rendered, GSR_BUF_TILE_RANGES and
 * GSR_BUF_VALUES_SORTED describe the culled lists (each an order-preserving subsequence of the
 * reference's), and GSR_BUF_N_CONTRIB counts positions in them.  No caller of the reference reads
 * those (bstate / istate are private to rasterize / ∇rasterize).
 * GSR_FLAG_REFERENCE_TILE_LISTS: keep exactly the reference's lists (duplicate_with_keys!,
 * utils.jl:85-120) — for list-level parity checks; ~7 % slower at 1 M Gaussians @1080p. */
#define GSR_FLAG_REFERENCE_TILE_LISTS 2u
/* Bit 1u is RETIRED: ABI 1 used it for GSR_FLAG_EXACT_TILE_CULL (the opposite meaning, when exact culling was opt-in).
 * gsr_create rejects it with GSR_E_INVALID_ARG so that a caller built against the old header fails loudly instead of
 * silently getting the other list mode. */
#define GSR_FLAG_RETIRED_BIT0 1u
/* Antialiased rendering (the Mip-Splatting 2-D filter; the Inria code's `antialiasing`, gsplat's rasterize_mode="antialiased").
 * The reference carries the mode dormant: add_blur returns compensation = sqrt(max(0, det S / det(S + blur_eps I)))
 * (render.jl:387-396), project! / ∇project! take a `compensations` array (projection.jl:45,93,125,190-194), rasterize passes
 * `nothing`.  With this flag every Gaussian's opacity is multiplied by its compensation of the view before anything reads it:
 * the image, the lists and every side output are exactly those of the plain render of opacities o * compensation, so a splat
 * the blur_eps dilation widened keeps the integrated contribution its 3-D Gaussian projects to.  Culling decisions that depend
 * on the opacity see the product (a visible Gaussian whose effective opacity is below 1/255 emits no instance).  The
 * compensations of the last forward are GSR_BUF_COMPENSATIONS.  The gradients gsr_backward / gsr_backward_trainer_tail return
 * on such a handle are those of the ANTIALIASED image: vopacities is with respect to the caller's activated opacity (not the
 * effective one), and vmeans / vscales / vrotations / vR / vt include the compensation's own pullback (∇add_blur,
 * render.jl:398-413).  A per-handle mode like the other switches; no struct changed, GSR_ABI_VERSION stays. */
#define GSR_FLAG_ANTIALIASED 4u

/* ABI version of this header: bumped whenever a struct of this file changes size or a flag / enum value changes meaning.
 *   1: round-1 layout (flag bit 1u = exact tile cull, smaller gsr_config / gsr_aux / gsr_stats / gsr_grads)
 *   2: round-2 layout (flag bit 1u = reference tile lists) — never given a number at the time
 *   3: round-3 layout (GSR_FLAG_REFERENCE_TILE_LISTS = 2u, bit 1u rejected, gsr_check_abi)
 *   4: gsr_aux grew by `flags` (GSR_FORWARD_ONLY) + `reserved`; gsr_sh_grad_from_views_tail.
 *   5: gsr_config grew by `ssim_precision` + `preprocess_form` (per-handle switches); gsr_stats.reserved became
 *      `preprocess_form` (the form that ran); gsr_get_ssim_precision / gsr_get_preprocess_form; late: gsr_grads and
 *      gsr_tail_state grew by `flags` + `reserved` (GSR_GRADS_COLOR_COTANGENT).
 *   6: this layout: gsr_config's switches re-encoded with 0 = default (a zero-initialised config is the default config) and
 *      grown by `form_tuner` + `grad_precision`; gsr_stats grew by the handle's view-history counters; gsr_check_abi also
 *      takes sizeof(gsr_tail_state); GSR_GRADS_COLOR_COTANGENT is checked against the cotangent gsr_loss_l1_ssim wrote;
 *      the policies are GPU-free exports of their own (gsr_policy.h). */
#define GSR_ABI_VERSION 6

/* Positional arguments of `rasterize(means_3d, shs, opacities, scales, rotations, ...)`
 * (rasterizer.jl:255-267).  opacities / scales are the ACTIVATED values, as the
 * reference's functor prologue produces them (rasterizer.jl:228-248). */
typedef struct gsr_inputs {
    int32_t n;              /* number of Gaussians */
    int32_t n_coeffs;       /* K: SH coefficients stored per Gaussian (1, 4, 9 or 16) */
    int32_t sh_degree;      /* active degree, (sh_degree+1)^2 <= K */
    const float* means;     /* device (3,N) */
    const float* shs;       /* device (3,K,N) */
    const float* opacities; /* device (1,N) */
    const float* scales;    /* device (3,N) */
    const float* rotations; /* device (4,N), 16-byte aligned (simd.jl:1-11) */
    float background[3];    /* keyword `background` */
} gsr_inputs;

/* The fields `rasterize` reads from `camera::Camera` (rasterizer.jl:285-291,310,321;
 * camera.jl:2-16).  R_dev/t_dev are the optional positional `R_w2c`, `t_w2c` device
 * arrays of the pose-optimisation variant (rasterizer.jl:261, projection.jl:71-75);
 * when non-NULL they override R/t. */
typedef struct gsr_camera {
    float R[9];             /* world->camera rotation, column-major */
    float t[3];
    float focal[2];         /* pixels */
    float principal[2];     /* normalised to [0,1] (projection.jl:268) */
    float camera_center[3];
    const float* R_dev;     /* device (3,3) column-major or NULL */
    const float* t_dev;     /* device (3) or NULL */
} gsr_camera;

/* Optional side outputs of `render!` (render.jl:7-8,109-112,128); keywords
 * `covisibilities`, `uncertainties` of rasterize (rasterizer.jl:265-266). */
typedef struct gsr_aux {
    uint8_t* covisibilities; /* device (N) Bool, set to 1 where T > 0.5, never cleared; or NULL */
    float* uncertainties;    /* device (W,H); or NULL.  Fully overwritten: the sum of alpha·T over the splats the pixel blends
                              * (render.jl:65,109,128); all zeros when the view renders no instance (n_rendered = 0) */
    /* `rast.gstate.radii` (states.jl:12, Int32 (N)) — read by the densification strategy right after
     * the step (strategy.jl:85-86).  When non-NULL the forward writes the radii THERE instead of into
     * handle-owned memory, so the caller's own GeometryState stays truthful; the array must stay valid
     * until the matching gsr_backward (which re-reads it).  NULL: handle-owned (GSR_BUF_RADII). */
    int32_t* radii;
    /* GSR_FORWARD_*.  New in ABI 4.  The reference's functor has a branch for rendering outside AD (rasterizer.jl:214-248,
     * `within_gradient`), used by `validate` (training.jl:501-504), the GUI (gui/worker.jl:654-657) and
     * scripts/render-views.jl: the same `rasterize`, whose backward state nobody will read. */
    uint32_t flags;
    uint32_t reserved; /* 0 */
} gsr_aux;
/* gsr_aux.flags — GSR_FORWARD_ONLY: this forward will not be differentiated.  The image, final_T, n_contrib, radii, tile ranges
 * and the geometry records are produced as always (image / final_T bit-identical to a training forward), but the sorted
 * splat stream and the sorted ids — 52-68 bytes per tile instance that only gsr_backward reads, a third of the fused
 * forward's HBM traffic — are not written and no gradient-row storage is reserved: GSR_BUF_VALUES_SORTED and
 * GSR_BUF_INSTANCE_AUX report 0 bytes, and gsr_backward / gsr_backward_trainer_tail / gsr_update_stats after such a forward
 * fail with GSR_E_STATE.  (Tiles with more than 1024 instances, and views binned in compact mode, still go through the
 * stream: they are the rare path.) */
#define GSR_FORWARD_ONLY 1u

typedef struct gsr_stats {
    int64_t n_rendered;         /* D: tile instances (rasterizer.jl:337) */
    int32_t n_visible;          /* V: count(radii > 0) */
    int32_t max_tile_instances; /* longest per-tile list */
    uint64_t generation;        /* ordinal of this forward on the handle (1, 2, ...): pass it to
                                 * gsr_backward (gsr_grads.forward_generation) to have the pairing checked */
    int64_t bins_bytes;         /* bytes of unsorted-key storage this view used (bins: (T+1) x capacity x 8; compact: 8 D;
                                 * bins + overflow tiles: the sum) */
    int32_t compact_binning;    /* 0: fixed-capacity bins; 1: the whole view was binned count -> scan -> scatter (no budget for
                                 * bins, or bins of < 1024 keys overflowed); 2: bins, and the lists beyond their capacity
                                 * scattered a second time (the rest of the view stayed on the fast path) */
    int32_t preprocess_form;    /* the binning form this view's first kernel ran in: 0 direct, 1 aggregating (2 x 32-bit LDS
                                 * words), 2 aggregating (2 x 16-bit words), 3 aggregating in horizontal bands of the tile grid */
    /* New in ABI 6 — the handle's VIEW HISTORY (gsr_policy.h: gsr_policy_state), cumulative since gsr_create.  gsr_forward keeps
     * state from one view to the next (bins capacity, compact mode, the form tuner, the held fused launch); a training run in
     * which N, D and the list skew drift can read here what that state did: in steady state none of the first four moves. */
    uint32_t bins_regrowths;    /* views after which the bins' capacity grew (a hipFree + hipMalloc before the next view) */
    uint32_t compact_fallbacks; /* views whose small bins overflowed: filled in vain, then binned again compactly */
    uint32_t tuner_rearms;      /* times the form tuner started over after a decision (scene size moved by 25 %, or 4096 views) */
    uint32_t scratch_regrowths; /* reallocations of any grow-only scratch buffer of the handle (each synchronises the device) */
    uint32_t fused_relaunches;  /* early fused launches that found the per-instance buffers too small: a no-op + the redo */
    uint32_t held_views;        /* views whose fused launch was held so that the tier walk could run beside it */
    uint32_t bin_capacity;      /* keys per tile of THIS view's bins (0: the view was binned compactly) */
    int32_t tuner_form;         /* the form tuner's decision on this handle: -1 none (yet / not its territory), 0 direct, 1 aggregating */
    float tuner_ms[2];          /* the measurement behind it: faster of two timed views of the direct / the aggregating form */
    uint32_t tier_tiles[3];     /* tiles of THIS view whose list has (1024, 4096], (4096, 8192], > 8192 instances: the lists the
                                 * fused sort + forward launch leaves to the tier sorts and the tier walk */
    uint32_t reserved;
} gsr_stats;

/* Cotangents returned by `∇rasterize` (rasterizer.jl:549): caller-provided device
 * buffers, fully overwritten (culled Gaussians and SH bands above sh_degree get exact
 * zeros, projection.jl:172-176).  Gradients are w.r.t. the ACTIVATED opacity/scale.
 * On a GSR_FLAG_ANTIALIASED handle they are the gradients of the antialiased image: vopacities is w.r.t. the caller's
 * activated opacity, not the effective one (opacity x compensation), and the geometry gradients carry ∇add_blur.
 * vR/vt (pose optimisation, projection.jl:243-256) may be NULL. */
typedef struct gsr_grads {
    float* vmeans;     /* (3,N) */
    float* vshs;       /* (3,K,N) */
    float* vopacities; /* (1,N) */
    float* vscales;    /* (3,N) */
    float* vrotations; /* (4,N) */
    float* vR;         /* (3,3) column-major or NULL */
    float* vt;         /* (3) or NULL */
    float* vcolors;    /* (3,N) or NULL.  New: when given, vshs is NOT written (may be NULL)
                        * and the view's SH-coefficient gradient is returned in its factored form — the colour
                        * cotangent after the clamp mask, vc — from which gsr_sh_grad_from_views rebuilds
                        * Σ_views basis(dir_view) x vc_view.  3 floats per Gaussian cross the links, not 3K. */
    float* vmeans2d;   /* (2,N) or NULL: `rast.gstate.∇means_2d` (states.jl:8; rasterizer.jl:440,474) — when given
                        * the screen-space mean gradient the densification statistics read (strategy.jl:85-86) is
                        * written THERE (fully overwritten; zeros for culled Gaussians) instead of into
                        * handle-owned memory (GSR_BUF_GRAD_MEANS2D then returns this pointer). */
    uint64_t forward_generation; /* 0: unchecked.  Otherwise must equal the gsr_stats.generation of the forward
                        * this backward belongs to: an intervening forward on the same handle (e.g. an eval
                        * render between a training forward and its pullback) is reported as GSR_E_STATE instead
                        * of silently producing the gradients of the wrong view. */
    uint32_t flags;    /* GSR_GRADS_* (new in ABI 5, late): 0 = none */
    uint32_t reserved; /* must be 0 */
} gsr_grads;
/* gsr_grads.flags / gsr_tail_state.flags — the caller's promise that channels >= 3 of `vpixels` (depth, alpha, normal) are exact
 * zeros: the cotangent gsr_loss_l1_ssim writes — the photometric loss only sees features[1:3] (training.jl:656,684-685) — not
 * touched since.  ∇render! then runs the :rgb arithmetic on the mode's stream: the :rgbdn backward 0.885 -> 0.702 ms, :rgbd
 * 0.713 -> 0.700 (config 3).  Gradients equal the unflagged call's up to the association of fp32 sums.  Ignored in :rgb mode.
 * ABI 6: the promise is CHECKED as far as the library can see — the flag is honoured only for the very buffer the handle's
 * last gsr_loss_l1_ssim wrote for THIS forward (pointer and forward generation recorded by the loss head); any other vpixels
 * with the flag set is GSR_E_INVALID_ARG instead of silently dropped depth / normal gradients.  What it cannot see is a term
 * added to that buffer in place afterwards: GSR_CHECK_COLOR_COTANGENT=1 in the environment makes every flagged backward
 * reduce |vpixels[3:]| first (one pass over the image + a host wait — debugging only) and fail with GSR_E_INVALID_ARG when it
 * is not exactly zero.  (Likewise a debugging switch, read at every allocation of handle scratch: GSR_DEBUG_FILL=nan / big fills
 * each new allocation of the handle's float-only buffers with the word 0xFFFFFFFF / 0x7F7F7F7F, so that a kernel that reads a
 * float it never wrote cannot pass on the zeros of fresh pages; index, key and count buffers are never filled.  And
 * GSR_DEBUG_GUARD=1, read at the same place: every handle buffer is allocated 4 KiB longer than its capacity and the extra
 * bytes hold a guard word — 0x7F7F7F7F behind the float-only buffers, a small valid value (1, or 0 behind lists of ids)
 * behind index, key and count buffers; capacities, gsr_memory_usage and every result are unchanged.  The guards are compared
 * whenever such a buffer is freed and by gsr_debug_check_guards below: a kernel that stores past the end of a handle buffer
 * is named.  Costs nothing when unset.) */
#define GSR_GRADS_COLOR_COTANGENT 0x1u

typedef struct gsr_handle gsr_handle;

/* GaussianRasterizer(kab; width, height, mode, ...) — rasterizer.jl:60-90. */
GSR_API int gsr_create(const gsr_config* cfg, gsr_handle** out);
/* KA.unsafe_free!(rast) — rasterizer.jl:136-145. */
GSR_API int gsr_destroy(gsr_handle* h);
/* release_scene_buffers!(rast) — rasterizer.jl:111-123. */
GSR_API int gsr_release_scene_buffers(gsr_handle* h);
/* memory_usage(rast) — rasterizer.jl:127-134 (device bytes owned by the handle). */
GSR_API int64_t gsr_memory_usage(const gsr_handle* h);
/* Debugging (no reference counterpart; a new function, no struct change: GSR_ABI_VERSION stays).  Synchronises the device and
 * compares the guard behind every buffer the handle owns, plus what was found when a guarded buffer was freed (regrowth,
 * gsr_release_scene_buffers).  GSR_OK, or GSR_E_STATE with gsr_last_error_string() naming the buffer, the first damaged byte
 * offset past its capacity and the word found there.  Handles created without GSR_DEBUG_GUARD=1 have no guards: GSR_OK. */
GSR_API int gsr_debug_check_guards(gsr_handle* h);
/* New in ABI 6 (no reference counterpart: the reference reallocates its states whenever the model or the instance count grew,
 * rasterizer.jl:275-278,340-343).  Pre-size the handle's grow-only scratch for views of up to n_gaussians Gaussians and
 * n_instances tile instances, so that the forwards that follow allocate nothing — a reallocation inside gsr_forward is a hipFree
 * + hipMalloc pair, i.e. a device synchronisation in the middle of a training step.  Where a trainer calls it: right after a
 * densification round changed the model (the reference empties its allocation cache at the same place, strategy.jl:92), with
 * headroom for the next rounds; the Python mirror's post_train_step does (1.5 x).  The key bins are not covered: their capacity is
 * a policy of its own (gsr_policy.h).  Never shrinks; 0 / smaller values are no-ops.
 * A call that has to REALLOCATE a buffer that already existed frees what the handle's last forward left in it, so it ENDS that
 * forward: until the next gsr_forward, gsr_backward / gsr_backward_trainer_tail / gsr_update_stats fail with GSR_E_STATE (before
 * any launch), gsr_buffer reports a null pointer and 0 bytes for the per-forward buffers (GSR_BUF_RADII, _GRAD_MEANS2D,
 * _VALUES_SORTED, _GEOM, _NORMALS, _GRAD_ROWS, _INSTANCE_AUX, _COMPENSATIONS) and gsr_copy_buffer of any of their bytes fails with GSR_E_STATE.
 * So reserve after gsr_update_stats, not between a forward and what reads it.  A call that reallocates nothing — sizes within
 * capacity, (0, 0), the first allocation of a buffer that did not exist, a repeat of an earlier call — leaves the forward live,
 * bit for bit.  The view history, the key bins and the loss head's scratch are not touched either way. */
GSR_API int gsr_reserve(gsr_handle* h, int64_t n_gaussians, int64_t n_instances);
/* A new function, no struct change: GSR_ABI_VERSION stays.  Ends the handle's live forward exactly as a reallocating gsr_reserve
 * does (see there), freeing nothing.  For a binding that owns the arrays it hands to gsr_aux.radii / gsr_grads.vmeans2d and is
 * about to replace them: the handle keeps those addresses until the next gsr_forward and must not be asked to read them again. */
GSR_API int gsr_drop_forward(gsr_handle* h);
/* Memory planning; no GPU needed.  The capacity — keys per tile — of the fixed-capacity key bins gsr_forward chooses for the view
 * AFTER one that rendered n_rendered instances with a longest tile list of max_tile_instances on a width x height image, under
 * bins_budget_bytes (0 = the default budget, see gsr_config) and with bins of current_capacity keys in place (0 = none: no view
 * yet, or the handle is in compact mode).  It is the policy's own function (gsr_policy_end_view calls the same helper): the
 * capacity only grows, and where bins in place have to grow they grow by at least a quarter of current_capacity, within the
 * budget's cap and the ceiling of 2^20 keys — so the result can exceed the longest list + 25 %.  0 = no bins: compact mode.  The
 * bins take (tiles + 1) x capacity x 8 bytes; a view whose longest list exceeds the capacity scatters those lists a second time
 * (+ 8 bytes per instance: gsr_stats.compact_binning == 2).
 * (No reference counterpart: the reference's BinningState is O(instances), states.jl:66-85.) */
GSR_API uint32_t gsr_bins_capacity_after(int64_t n_rendered, int32_t max_tile_instances, int32_t width, int32_t height,
                                         uint64_t bins_budget_bytes, uint32_t current_capacity);

/* rasterize(...) — rasterizer.jl:255-408: project! + spherical_harmonics! +
 * count_tiles_per_gaussian! + cumsum! + duplicate_with_keys! + sortperm!/_permute! +
 * identify_tile_range! + render!.  Writes image_out (C,W,H); returns an all-zero image
 * when nothing is visible (rasterizer.jl:338).  aux and stats may be NULL.
 * Synchronisation: all device work is ordered on `stream`.  The call returns after the host has read the instance
 * count of this view (the reference's one read-back, rasterizer.jl:337) — it spins on a word of pinned host memory
 * the tile scan writes; by then the sort + forward of the tiles is already queued behind the scan (it checks the
 * scan's totals against the capacity of the handle's buffers on the device), so the GPU does not wait for the host. */
GSR_API int gsr_forward(gsr_handle* h, const gsr_inputs* in, const gsr_camera* cam, float* image_out,
                        const gsr_aux* aux, void* stream, gsr_stats* stats);

/* Per-Gaussian contribution scores: which Gaussians a set of views actually uses.  No reference counterpart — the reference
 * exports the per-PIXEL sum of the blend weights (gsr_aux.uncertainties) and nothing per Gaussian.  The quantities are those of
 *   RadSplat        (Niemeyer et al., 2024, eq. 7-8): h_g = max over pixels and views of the blend weight w = alpha·T; prune h_g < 0.01
 *   LightGaussian   (Fan et al., 2023) / Mini-Splatting (Fang & Wang, 2024): the sum of w over the pixels that blend g, and the hit count
 * without the volume weighting and the keep-fraction rules, which are the caller's.
 * For every (pixel, list entry) that render! BLENDS (alpha >= 1/255, sigma >= 0, the pixel not stopped, and not the entry that
 * stops it with T' < 1e-4 — exactly the entries that add to the image), with w the fp32 alpha·T the pixel's colour is scaled by:
 *   max_weight[g]  max=  the bits of w            (w > 0: float order is unsigned order; read the word back as a float)
 *   hits[g]        +=    1
 *   weight_sum[g]  +=    q = round-to-nearest-even(w · 2^24)     (w <= 0.99 and w >= 1e-4 / 255: 6 <= q < 2^24; value = sum / 2^24)
 * All three are integers, so the result is bit-identical from run to run and across the default / reference tile lists, the
 * binning forms, compact mode, the fused launch and the tier walk, and GSR_FORWARD_ONLY.  The arrays are the caller's, device,
 * (N) each, ACCUMULATED INTO AND NEVER CLEARED (like covisibilities): scoring V views is V calls on the same arrays.  Any of the
 * three pointers may be NULL; culled Gaussians and instances no pixel blends are not touched.  On a GSR_FLAG_ANTIALIASED handle w
 * is that of the effective opacity.  hits and weight_sum must be 8-byte aligned; flags and reserved must be 0. */
typedef struct gsr_scores {
    uint32_t* max_weight; /* device (N) or NULL */
    uint64_t* hits;       /* device (N) or NULL */
    uint64_t* weight_sum; /* device (N) or NULL */
    uint32_t flags;       /* 0 */
    uint32_t reserved;    /* 0 */
} gsr_scores;
/* gsr_forward with the scores of this view accumulated into `scores`.  scores == NULL, or all three pointers NULL: gsr_forward
 * itself (the same launches of the same kernels) — gsr_forward(...) IS gsr_forward_scored(..., NULL, ...).  Works together with
 * every gsr_aux member.  The scored kernels do one wave reduction pair per visit and one triple of integer atomics per blended
 * tile instance more than the plain ones: an offline pass over the training views, not a training forward. */
GSR_API int gsr_forward_scored(gsr_handle* h, const gsr_inputs* in, const gsr_camera* cam, float* image_out,
                               const gsr_aux* aux, const gsr_scores* scores, void* stream, gsr_stats* stats);
/* The keep mask of a pruning rule on accumulated scores, compared in integers: valid_out[i] = 1 where Gaussian i is KEPT, else 0.
 *   GSR_SCORE_MAX_WEIGHT  bits(max_weight[i]) >= bits((float)threshold)     (RadSplat: threshold 0.01)
 *   GSR_SCORE_WEIGHT_SUM  weight_sum[i] >= ceil(threshold · 2^24)
 *   GSR_SCORE_HITS        hits[i] >= ceil(threshold)
 * Only the rule's own array is read (the others may be NULL).  threshold must be finite and >= 0 (and its fixed-point form must
 * fit 64 bits).  valid_out feeds gsr_mask_findall / gsr_compose_rows like gsr_densify_mask's GSR_DENSIFY_PRUNE mask. */
enum { GSR_SCORE_MAX_WEIGHT = 0, GSR_SCORE_WEIGHT_SUM = 1, GSR_SCORE_HITS = 2 };
GSR_API int gsr_contribution_mask(int64_t n, int rule, double threshold, const uint32_t* max_weight, const uint64_t* hits,
                                  const uint64_t* weight_sum, uint8_t* valid_out, void* stream);

/* ∇rasterize(vpixels, ...) — rasterizer.jl:416-550 (the pullback of the rrule,
 * rasterizer.jl:552-573): ∇render! + ∇project! + ∇spherical_harmonics!.
 * vpixels: device (C,W,H).  `in`/`cam` must be the ones given to gsr_forward.
 * All work is ordered on `stream`; when the view has a few very long tile lists (> 1024 instances, at most 256 such
 * tiles) their part of ∇render! runs on a stream the handle owns, forked from and joined back into `stream` with
 * events — nothing the caller has to do. */
GSR_API int gsr_backward(gsr_handle* h, const gsr_inputs* in, const gsr_camera* cam, const float* vpixels,
                         const gsr_grads* grads, void* stream);

/* How the host thread waits inside gsr_forward for the instance count (the reference blocks in a synchronous
 * device->host copy there, rasterizer.jl:337).  Process-wide; the three values are stored and read atomically (a forward
 * running on another thread sees the old or the new policy, never a mix of fields from both: they are packed in one word).
 *   sleep_us == 0 (default: 30, 0, 0): spin for `spin_us` microseconds, then poll with sched_yield() — other runnable threads
 *   (RCCL's proxy threads on an 8-rank host) get the core at once; no timers; a pure spin's step time.
 *   sleep_us > 0 (opt-in, e.g. 100, 0, 50): sleep through the expected wait (a running average per handle; the host runs
 *   ahead of the GPU, so the wait is about the same every step) except for its last `spin_us` microseconds, then
 *   sched_yield() for `yield_us`, then sleeps of `sleep_us` — a fraction of the CPU time, at the mercy of the host's timer
 *   wake-up latency.
 *   (1000000, 0, 0) is a pure spin. */
GSR_API int gsr_host_wait_policy(int spin_us, int yield_us, int sleep_us);

/* Views into the state the reference keeps in rast.gstate / bstate / istate
 * (states.jl:2-111); valid until the next gsr_forward / release on this handle.
 * gsr_buffer() copies nothing: it returns the device address and byte size. */
enum {
    GSR_BUF_RADII = 0,         /* int32 (N)        gstate.radii — read by densification (strategy.jl:85-86); the caller's
                                *                   own array when the forward was given gsr_aux.radii */
    GSR_BUF_GRAD_MEANS2D = 1,  /* float (2,N)      gstate.∇means_2d, valid after gsr_backward (the caller's own array when
                                *                   the backward was given gsr_grads.vmeans2d) */
    GSR_BUF_N_CONTRIB = 2,     /* uint32 (W,H)     istate.n_contrib */
    GSR_BUF_FINAL_T = 3,       /* float (W,H)      istate.accum_α */
    GSR_BUF_TILE_RANGES = 4,   /* uint32 (2,T)     istate.ranges */
    GSR_BUF_VALUES_SORTED = 5, /* uint32 (D)       bstate.gaussian_values_sorted (0-based ids) */
    GSR_BUF_GEOM = 6,          /* 16 x 32-bit (N): one 64-byte record per Gaussian (stale where radii == 0):
                                *   [0..1] mean2d, [2..4] conic a,b,c, [5] opacity, [6..8] rgb, [9] clamped bits (u32,
                                *   bit c = channel c), [10] depth, [11] u32 instance-slot prefix inside the 256-block,
                                *   [12] u32 rect xmin|ymin<<16, [13] u32 rect xmax|ymax<<16 (utils.jl:18-29), [14] u32 blend-test
                                *   threshold X of the Gaussian (see GSR_BUF_INSTANCE_AUX), [15] u32 bit mask of the rect's tiles (row-major) the Gaussian
                                *   was binned into (rects of at most 32 tiles) */
    GSR_BUF_NORMALS = 7,       /* float4 (N): camera-space normal (mode RGBDN only) */
    GSR_BUF_GRAD_ROWS = 8,     /* 12 (:rgb) or 16 x float per slot, Gaussian-major: the per-instance gradient rows of the last
                                *   gsr_backward.  A Gaussian whose tile rect has at most 32 tiles owns one slot per tile it
                                *   was binned into (in row-major tile order); larger rects one per tile of the rect */
    GSR_BUF_INSTANCE_AUX = 9,  /* 4 x 32-bit (D), sorted instance order (plane s2 of the splat stream):
                                *   [0] blue, [1] u32 Gaussian-major slot, [2] depth (:rgbd / :rgbdn) or, in :rgb mode, the u32 blend-test
                                *   threshold X (bits(sigma) < X is the reference's blend test; 0: never blends), [3] u32 footprint masks
                                *   (bits 0..15 tile rows, 16..19 8x8 quadrants the instance can touch; bit 20: the splat is a
                                *   needle — 2-D axis ratio beyond 10 : 1 —, evaluated in the backward's accurate arithmetic) */
    GSR_BUF_COMPENSATIONS = 10 /* float (N): the reference's `compensations` (projection.jl:45) of the last gsr_forward on a
                                *   GSR_FLAG_ANTIALIASED handle, handle-owned, stale where radii == 0; the backward re-reads it.
                                *   A handle without the flag has no such buffer: null pointer, 0 bytes */
};
GSR_API int gsr_buffer(const gsr_handle* h, int which, const void** dev_ptr, size_t* bytes);
/* Copy of one of those buffers into caller memory, enqueued on `stream` by the library's own HIP
 * runtime (hosts that cannot wrap foreign device pointers — and must not dlopen a second HIP
 * runtime to copy them — use this).  dst: device, at least `bytes` bytes; bytes must not exceed
 * what gsr_buffer reports. */
GSR_API int gsr_copy_buffer(const gsr_handle* h, int which, void* dst, size_t bytes, void* stream);

/* update_stats!(strategy, rast.gstate.radii, rast.gstate.∇means_2d, resolution) —
 * src/strategy.jl:107-136 (`_update_stats!`): for every Gaussian visible in the last
 * forward, max_radii = max(max_radii, radius), accum += ‖∇mean_2d · resolution · 0.5‖,
 * denom += 1.  All three are caller-owned device arrays of N elements (the DefaultStrategy's
 * densification state); needs a completed gsr_forward/gsr_backward pair on the handle. */
GSR_API int gsr_update_stats(gsr_handle* h, int32_t* max_radii, float* accum_grad_means2d, float* denom, void* stream);

/* _fused_ssim / fused_ssim_bwd — src/fused_ssim.jl:373-408.  Arrays are (W,H,CH,B),
 * x fastest.  With train == 0 the three partial-derivative maps may be NULL. */
GSR_API int gsr_ssim_forward(int W, int H, int CH, int B, const float* img, const float* ref, float C1, float C2,
                             int train, float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12,
                             void* stream);
GSR_API int gsr_ssim_backward(int W, int H, int CH, int B, const float* img, const float* ref, const float* dL_dmap,
                              const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                              float* dL_dimg, void* stream);

/* Arithmetic of the three SSIM entry points (gsr_ssim_forward / gsr_ssim_backward / gsr_loss_l1_ssim): the PROCESS-WIDE
 * DEFAULT — what gsr_ssim_forward / gsr_ssim_backward (no handle) use, and gsr_loss_l1_ssim on a handle whose
 * gsr_config.ssim_precision is GSR_DEFAULT; a handle created with GSR_SSIM_FAST / GSR_SSIM_EXACT there is not affected.  Stored and read
 * atomically; gsr_get_ssim_precision returns the current value (so that a scoped override can restore what it found).
 *   0 (default): multiply-adds contracted to FMAs and the six divisions of the SSIM formula (fused_ssim.jl:219-233) taken over
 *      two hardware reciprocals — what a GPU compiler makes of the reference's own source; results agree with the
 *      fp32-as-written evaluation to ~1e-6 relative (the loss to 1e-6 absolute, its pullback to 1e-5 relative L2);
 *   1: every fp32 operation as written, IEEE divisions: bit-identical to the CPU oracle (the parity tests' twin), ~35 us
 *      slower per 1080p loss evaluation.
 * GSR_SSIM_EXACT=1 in the environment starts the process in mode 1. */
GSR_API int gsr_ssim_precision(int exact);
GSR_API int gsr_get_ssim_precision(void);

/* Form of the binning inside gsr_forward's first kernel (preprocess: projection.jl:69-129 + spherical_harmonics! +
 * utils.jl:85-142 fused): the PROCESS-WIDE DEFAULT, used by handles whose gsr_config.preprocess_form is GSR_DEFAULT (a
 * handle created with GSR_PREPROCESS_DIRECT / GSR_PREPROCESS_AGGREGATING there is pinned).  Outputs are identical in every form (only the arbitrary order of the unsorted
 * keys inside a tile's bin differs), this is a performance switch and the tests' handle on both code paths.
 *  -1 (default): chosen per call — the aggregating form for scenes of >= 250 000 Gaussians on grids whose counter words
 *      fit the LDS three times per CU (up to ~10 700 tiles with 2 x 32-bit words: 1080p; up to ~21 500 with 2 x 16-bit words
 *      while the bins' capacity is below 65 024: 1440p; 4K no), else the direct form;
 *   0: always the direct form (one returning global atomic per instance pair; the rect walk is spread evenly over the
 *      lanes of each wave, as in the aggregating form);
 *   1: the aggregating form wherever its LDS fits (a workgroup adds its requests up per counter word in LDS and issues
 *      one global atomic per word, in address order; both rect walks are spread evenly over the lanes of each wave).
 * GSR_PREPROCESS_AGG=0/1 in the environment starts the process in mode 0 / 1. */
GSR_API int gsr_preprocess_form(int form);
GSR_API int gsr_get_preprocess_form(void);

/* The photometric loss head of Trainer.step! — src/training.jl:656,684-694:
 *   image = features[1:3,:,:]; permute to (W,H,3,1);
 *   L = (1-lambda)*mean|image-target| + lambda*(1-mean(fused_ssim(image; ref=target)))
 * and its pullback to the rasterizer output.  image: device (C,W,H) as written by
 * gsr_forward; target: device (W,H,3); loss_out: device scalar; vpixels: device (C,W,H)
 * (channels >= 3 zeroed).  Scratch is owned by the handle. */
GSR_API int gsr_loss_l1_ssim(gsr_handle* h, const float* image, const float* target, float lambda_dssim,
                             float* loss_out, float* vpixels, void* stream);

/* The functor prologue `(rast::GaussianRasterizer)(means_3d, opacities, scales, rotations,
 * sh_color, sh_remainder, ...)` (rasterizer.jl:200-253) up to its call of rasterize():
 *   shs = hcat(sh_color (3,1,N), sh_remainder (3,k_rest,N))          (rasterizer.jl:218-228)
 *   opacities_act = NU.sigmoid.(opacities (1,N))                     (rasterizer.jl:229-234)
 *   scales_act = exp.(scales), an isotropic (1,N) scale tiled x3     (rasterizer.jl:235-247)
 * scale_dims is 1 (isotropic) or 3.  k_rest may be 0 (sh_remainder NULL).  All device. */
GSR_API int gsr_prologue_forward(int32_t n, int32_t k_rest, int32_t scale_dims, const float* sh_color,
                                 const float* sh_remainder, const float* opacities, const float* scales, float* shs,
                                 float* opacities_act, float* scales_act, void* stream);
/* Pullback of the prologue — what Zygote derives around the rrule of rasterize
 * (rasterizer.jl:552-573) for the raw parameters the trainer optimises
 * (training.jl:646-656): vshs is split, v_opacities = v_act * a(1-a), v_scales = v_act * exp(s)
 * (summed over the three tiled rows when isotropic). */
GSR_API int gsr_prologue_backward(int32_t n, int32_t k_rest, int32_t scale_dims, const float* opacities_act,
                                  const float* scales_act, const float* vshs, const float* vopacities_act,
                                  const float* vscales_act, float* v_sh_color, float* v_sh_remainder,
                                  float* v_opacities, float* v_scales, void* stream);

/* `NU.step!(opt, θ, ∇)` of NerfUtils 0.2's Adam (external dependency, Project.toml:76; call
 * sites training.jl:234-239,778), for up to GSR_ADAM_MAX_GROUPS parameter arrays in ONE
 * launch.  Each group is one `NU.Adam` (its own lr; μ, ν of the parameter's length).
 * `current_step` is the optimizer's counter AFTER its increment (1 on the first step).
 *   μ = β1 μ + (1-β1) g;  ν = β2 ν + (1-β2) g²;
 *   θ -= lr · sqrt(1-β2^t)/(1-β1^t) · μ / (sqrt(ν) + ϵ)            (ϵ = 1f-15: training.jl:229)
 * theta, mu, nu are updated in place; grad is read only.  All device. */
#define GSR_ADAM_MAX_GROUPS 8
typedef struct gsr_adam_group {
    float* theta;
    const float* grad;
    float* mu;
    float* nu;
    int64_t count; /* elements */
    float lr;
    uint32_t current_step;
} gsr_adam_group;
GSR_API int gsr_adam_step(const gsr_adam_group* groups, int32_t n_groups, float beta1, float beta2, float eps,
                          void* stream);

/* The whole trainer tail of `step!` in one pass over the parameters (SURVEY.md §8f rank 1:
 * "fusing it removes 3 more round-trips"): pullback of the functor prologue
 * (rasterizer.jl:218-247) + `NU.step!` on the six optimizers (training.jl:768-779) + the
 * prologue of the NEXT forward.  Group order everywhere: points, features_dc, features_rest,
 * opacities, scales, rotations (training.jl:415-416).
 *   grads: the gradients gsr_backward wrote, w.r.t. the ACTIVATED values
 *   theta/mu/nu[6], lr[6], current_step[6] (counters AFTER increment): the raw parameters and
 *          the NU.Adam states, updated in place
 *   shs (3,K,N), opacities_act (1,N), scales_act (3,N): on entry the activated copies the
 *          forward of THIS step used (σ' and exp' are taken from them), on exit those of the
 *          updated parameters, ready for the next gsr_forward.
 * Bit-identical θ, μ, ν to gsr_prologue_backward + gsr_adam_step; features_rest may be empty
 * (k_rest = 0). */
typedef struct gsr_tail_grads {
    const float* vmeans;        /* (3,N) */
    const float* vshs;          /* (3,K,N) */
    const float* vopacities;    /* (1,N)  w.r.t. sigmoid(opacities) */
    const float* vscales;       /* (3,N)  w.r.t. exp(scales) */
    const float* vrotations;    /* (4,N) */
} gsr_tail_grads;
GSR_API int gsr_trainer_tail_step(int32_t n, int32_t k_rest, int32_t scale_dims, const gsr_tail_grads* grads,
                                  float* const theta[6], float* const mu[6], float* const nu[6], const float lr[6],
                                  const uint32_t current_step[6], float beta1, float beta2, float eps, float* shs,
                                  float* opacities_act, float* scales_act, void* stream);

/* Single-GPU trainer step: gsr_backward with gsr_trainer_tail_step applied in its epilogue
 * ("fuse the trainer tail into the per-Gaussian backward").  Equivalent to
 *     gsr_backward(h, in, cam, vpixels, &grads, stream);
 *     gsr_trainer_tail_step(n, K-1, scale_dims, &grads, theta, mu, nu, ..., stream);
 * with bit-identical θ, μ, ν and activated copies, but the 59·N gradient floats are never written:
 * they live in registers between ∇project / ∇spherical_harmonics and the Adam update.  Not for the
 * multi-GPU step (the gradients must be exchanged before the update) and not with pose gradients.
 *   in : the inputs of the matching gsr_forward.  They must BE the trainer's arrays —
 *        in->means == theta[0], in->rotations == theta[5], in->shs == shs,
 *        in->opacities == opacities_act, in->scales == scales_act (checked; GSR_E_INVALID_ARG) —
 *        because they are updated in place.  K = in->n_coeffs; features_rest holds K-1 bands.
 *   vmeans2d : (2,N) gstate.∇means_2d of this backward, or NULL (handle-owned GSR_BUF_GRAD_MEANS2D)
 *   forward_generation : gsr_stats.generation of the forward being differentiated, or 0 */
typedef struct gsr_tail_state {
    float* theta[6];            /* points, features_dc, features_rest, opacities, scales, rotations */
    float* mu[6];
    float* nu[6];
    float lr[6];
    uint32_t current_step[6];   /* counters AFTER increment (NU.Adam counts from 1) */
    float beta1, beta2, eps;
    int32_t scale_dims;         /* 3, or 1 for isotropic scenes */
    float* shs;                 /* (3,K,N) */
    float* opacities_act;       /* (1,N) */
    float* scales_act;          /* (3,N) */
    float* vmeans2d;
    uint64_t forward_generation;
    uint32_t flags;             /* GSR_GRADS_* (gsr_grads.flags) */
    uint32_t reserved;          /* must be 0 */
} gsr_tail_state;
GSR_API int gsr_backward_trainer_tail(gsr_handle* h, const gsr_inputs* in, const gsr_camera* cam,
                                      const float* vpixels, const gsr_tail_state* st, void* stream);

/* Boolean-mask compaction of per-Gaussian arrays — the `x[:, mask]` / `x[:, :, mask]` /
 * `x[mask]` logical indexing that `prune_points!`, `densify_clone!`, `densify_split!` and
 * `_prune_optimizer!` apply to every parameter, both Adam moments and the densification
 * statistics (src/densification.jl:29-62,64-121,138-191,279-288).
 *   gsr_mask_findall : indices (0-based, ascending) of the non-zero bytes of mask[n] — Julia's
 *                      `findall(mask)`; *count_out (device) receives their number.  `scratch`
 *                      is gsr_mask_findall_scratch_bytes(n) bytes of device memory.
 *   gsr_gather_rows  : dst[g][r, :] = src[g][indices[r], :] for up to GSR_ADAM_MAX_GROUPS arrays
 *                      in one launch; a row is row_words 4-byte words (float / int32 / uint32).
 * All pointers device; order-preserving, bit-exact. */
typedef struct gsr_gather_group {
    const void* src;
    void* dst;
    int32_t row_words;
} gsr_gather_group;
GSR_API size_t gsr_mask_findall_scratch_bytes(int64_t n);
GSR_API int gsr_mask_findall(const uint8_t* mask, int64_t n, uint32_t* indices, uint32_t* count_out, void* scratch,
                             void* stream);
GSR_API int gsr_gather_rows(const gsr_gather_group* groups, int32_t n_groups, const uint32_t* indices, int64_t count,
                            void* stream);

/* Adaptive density control of the reference's DefaultStrategy on the device (SURVEY.md §8f rank 3;
 * src/densification.jl:1-297, src/gaussians.jl:119-137).  The host keeps the reference's control flow
 * (densify_and_prune! -> densify_clone! -> densify_split! -> prune_points!, strategy.jl:78-105); every
 * per-Gaussian pass is one of these launches.  All pointers device, caller-owned.
 *
 * gsr_densify_grad_mean : ∇means_2d = accum ./ denom with NaN -> 0                 (densification.jl:7-10)
 * gsr_densify_mask      : kind GSR_DENSIFY_CLONE  mask = grad >  thr && max(exp(scales)) < gamma   (:34-38)
 *                              GSR_DENSIFY_SPLIT  mask = grad >= thr && max(exp(scales)) > gamma   (:73-80; `grad`
 *                                                 holds n_grad <= n entries, rows beyond it count as 0: padded_grad)
 *                              GSR_DENSIFY_PRUNE  mask = sigmoid(opacity) > min_opacity, and when max_screen_size > 0
 *                                                 && max_radii < max_screen_size && max(exp(scales)) < gamma  (:18-25)
 *                         scales are the RAW log-scales (scale_dims = 3, or 1 for an isotropic model).  Every comparison
 *                         is the reference's own: strict where it is strict, and false on a NaN — a NaN grad, opacity or
 *                         scale on ANY axis (Julia's `maximum` propagates it) leaves the row out of all three masks.  With
 *                         max_screen_size = 0 the prune mask reads neither scales nor max_radii (both may be NULL).
 * gsr_compose_rows      : the row surgery of append_gaussians! / _append_optimizer! / prune_points! /
 *                         _prune_optimizer! (:138-297) for up to GSR_COMPOSE_MAX_GROUPS arrays in one launch:
 *                           dst[r]                      = src[keep_idx[r]]                 r < n_keep (keep_idx NULL: r)
 *                           dst[n_keep + k*n_sel + j]   = new_zero ? 0 : src[sel_idx[j]]   j < n_sel, k < reps
 *                         clone: keep = identity, sel = findall(mask), reps 1; split: keep = findall(!mask),
 *                         sel = findall(mask), reps 2 (Julia's block `repeat`); prune: keep = findall(valid), n_sel 0.
 *                         new_zero = 1 for the Adam moments (their new rows are zeros).
 * gsr_split_transform   : on the 2m rows a split appended: sigma = exp(scale); point += R(q)·(sigma .* randn3);
 *                         scale = log(sigma / 1.6)   (:81-104, _add_split_noise! :121-135).  The normals come from a
 *                         counter-based generator keyed by (seed, row) — the reference uses the backend's device RNG.
 * gsr_reset_opacity     : opacity = inverse_sigmoid(min(0.1, sigmoid(opacity)))  (gaussians.jl:119-126,137).  `min` is Julia's:
 *                         a NaN opacity stays a NaN (gsr_count_nonfinite still sees it); an opacity whose fp32 sigmoid
 *                         underflows to 0 becomes -Inf, as log(0 / 1) is.
 * tests/densify_ref.py states all of this in float64; tests/test_gpu_density_edges.py holds the kernels to it. */
enum { GSR_DENSIFY_CLONE = 0, GSR_DENSIFY_SPLIT = 1, GSR_DENSIFY_PRUNE = 2 };
#define GSR_COMPOSE_MAX_GROUPS 24
typedef struct gsr_compose_group {
    const void* src;
    void* dst;
    int32_t row_words; /* 4-byte words per row */
    int32_t new_zero;  /* appended rows are zeros (Adam moments) instead of copies */
} gsr_compose_group;
GSR_API int gsr_densify_grad_mean(int64_t n, const float* accum_grad_means2d, const float* denom, float* grad_out, void* stream);
GSR_API int gsr_densify_mask(int32_t kind, int64_t n, int64_t n_grad, const float* grad, const float* scales,
                             int32_t scale_dims, const float* opacities, const int32_t* max_radii, float grad_threshold,
                             float gamma, float min_opacity, int32_t max_screen_size, uint8_t* mask, void* stream);
GSR_API int gsr_compose_rows(const gsr_compose_group* groups, int32_t n_groups, const uint32_t* keep_idx, int64_t n_keep,
                             const uint32_t* sel_idx, int64_t n_sel, int32_t reps, void* stream);
GSR_API int gsr_split_transform(int64_t n_new, int32_t scale_dims, float* points, const float* rotations, float* scales,
                                uint32_t seed, void* stream);
GSR_API int gsr_reset_opacity(int64_t n, float* opacities, void* stream);
/* Not in the reference: 63-bit Morton (Z-order) codes of the Gaussians' positions inside the host-given box (21 bits per
 * axis) — the sort key of the OPTIONAL spatial re-sort a trainer may run after a densification (the arrays are composed
 * anyway there: gsr_compose_rows with keep_idx = the sorting permutation, `gs.ids` keeps the identities).  Spatially ordered
 * Gaussians make the binning's counter traffic and the tile sort's record gathers coherent: config 3 steps in 1.41 ms
 * instead of 1.43.  box_lo / box_hi: host pointers to 3 floats. */
GSR_API int gsr_morton_codes(int64_t n, const float* points, const float* box_lo, const float* box_hi, uint64_t* codes,
                             void* stream);

/* The first step of a training run: the initial scales of a model built from a point cloud (src/dataset.jl:236-249
 * `compute_scales`; what simple-knn is to the original 3DGS code).  Per point i the three smallest
 *   d2(i,j) = (dx*dx + dy*dy) + dz*dz   (fp32, uncontracted; dx = x_i - x_j, …)   over all rows j != i
 * — j is excluded by index, a duplicate at distance 0 is a neighbour —, ascending, found by an EXACT search (the multiset
 * equals a brute-force search's for every input and every `order`), and from them, as the reference does on the tree's
 * distances:   q_k = sqrtf(d2_k)·sqrtf(d2_k);  md = ((q_0 + q_1) + q_2) / 3;  s = logf(sqrtf(fmaxf(1e-7f, md) · point_size)).
 *   points     : device, (n,3) rows.
 *   order      : device, n row numbers, or NULL = 0, 1, …: the order in which the search groups the points (64 consecutive
 *                entries share a box).  A permutation along a space-filling curve (gsr_morton_codes + a sort) makes the
 *                search fast; any permutation gives the same bits.  Entries are clamped into [0, n): a vector that is no
 *                permutation gives wrong numbers, never an access outside the arrays.
 *   scales_out : device, (n,scale_dims): s in all three columns, or ((s + s) + s) / 3 in the one (the isotropic model's
 *                `mean(scales; dims=1)`, gaussians.jl:53).
 *   dist2_out  : device, (n,3): the three d2, ascending; NULL: not wanted.
 *   scratch    : device, gsr_knn_scratch_bytes(n) bytes (16 per point + 24 per 64 points), 16-byte aligned.
 * n == 0: GSR_OK, nothing is launched.  GSR_E_INVALID_ARG, before anything touches the device: 1 <= n <= 3 (the reference's
 * knn(…, 4) throws there) or n >= 2^31, scale_dims not 1 or 3, !(point_size > 0), a null points / scales_out / scratch,
 * scratch_bytes < gsr_knn_scratch_bytes(n), a misaligned scratch.  A point with a non-finite coordinate is never anybody's
 * neighbour; its own row is unspecified.  gsr_knn_scratch_bytes is 0 for n <= 0 (and n >= 2^31). */
GSR_API size_t gsr_knn_scratch_bytes(int64_t n);
GSR_API int gsr_knn_scales(int64_t n, const float* points, const int32_t* order, float point_size, int32_t scale_dims,
                           float* scales_out, float* dist2_out, void* scratch, size_t scratch_bytes, void* stream);

/* The 3-D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024, §4.1): the world-space companion of
 * GSR_FLAG_ANTIALIASED.  Every Gaussian is low-pass filtered by the highest rate at which any training camera samples it;
 * the filter is folded into the ACTIVATED scales and opacities in front of gsr_forward.  No handle, no struct, nothing read
 * back to the host.  Arrays are device, contiguous float32 unless stated.
 *
 * gsr_filter3d_compute: the sweep of n points against n_cameras cameras, redone when the points change (after every
 * densification round).  camera_table: n_cameras rows of GSR_FILTER3D_CAMERA_FLOATS floats,
 *     R[9] (column-major) t[3]   as in gsr_camera
 *     focal[2]
 *     pp[2]    = principal · resolution
 *     lo[2]    = -margin · resolution         hi[2] = (1 + margin) · resolution
 *     inv_f    = 1 / max(focal)
 *     one pad word
 * Per point p and camera v, every operation ONE rounded fp32 operation in this association:
 *     xc[i] = ((R[i]*p0 + R[i+3]*p1) + R[i+6]*p2) + t[i]     i = 0,1,2 ;  z = xc[2]
 *     u[j]  = focal[j]*xc[j] + pp[j]*z                         j = 0,1
 *     valid = (z > near_plane) && (lo[j]*z <= u[j]) && (u[j] <= hi[j]*z) for both j      (any NaN: not valid)
 *     tau   = z * inv_f
 *     tmin(p) = min of tau over the valid cameras ;  seen(p) = some camera is valid
 *     filter(p) = k * tmin(p) where seen(p), else the maximum of filter over the seen points (0 when no point is seen)
 * — the paper's highest sampling rate max_v focal_v / depth_v, inverted; k = sqrt(variance), 0.2 in the paper.  Minimum and
 * maximum are exact in any order: the output is the same bits in every run.
 *   filter : (n), fully overwritten.      seen : (n) bytes, 1 / 0, or NULL.      count : one uint32, the seen points, or NULL.
 *   scratch: gsr_filter3d_scratch_bytes(n) bytes (1 per point, 8 per 1024 points, 8 more), 8-byte aligned.
 * GSR_E_INVALID_ARG: n < 0 or n >= 2^31, n_cameras < 1, near_plane or k negative or NaN, a null points / camera_table /
 * filter / scratch, scratch_bytes too small, a misaligned scratch.  n == 0: GSR_OK, nothing is launched.
 *
 * gsr_filter3d_apply: opacities_act (n), scales_act (n,3) — what gsr_prologue_forward wrote, scales > 0 — and filter (n) to
 *     f2 = f*f ;  se[i] = sqrtf(s[i]*s[i] + f2) ;  r[i] = s[i] / se[i] ;  c = (r[0]*r[1])*r[2] ;  o_eff = o * c
 * in scales_out / opacities_out (other arrays than the inputs).  c = sqrt(det S / det(S + f2 I)) of the paper, as a product
 * of ratios that cannot underflow for small scales; o_eff · Π se = o · Π s.  A row with f == 0 passes through bit for bit.
 * raw != 0: logf(se[i]) and logit(o_eff) instead, the values a .ply stores — an exported model renders filtered in any
 * viewer.  (1 - o_eff is formed as (1 - o) + o·(1 - c), 1 - c from 1 - r[i] = f2 / (se[i]·(se[i] + s[i])): no cancellation.)
 *
 * gsr_filter3d_apply_backward: the pullback, the filter a constant.  g_opacities (n) / g_scales (n,3): the cotangents
 * w.r.t. the EFFECTIVE values, as gsr_backward wrote them;
 *     vo = g_o * c ;  vs[i] = g_s[i]*r[i] + ((g_o*o)*P[i]) * (f2 / ((se[i]*se[i])*se[i])),  P[i] = product of the other two r
 * w.r.t. the activated values, for gsr_prologue_backward / gsr_trainer_tail_step.  v_opacities / v_scales may be
 * g_opacities / g_scales (in place).  The fused gsr_backward_trainer_tail cannot carry this step: a filtered training step
 * runs gsr_backward + gsr_filter3d_apply_backward + gsr_trainer_tail_step, as with gsr_flatten_loss. */
#define GSR_FILTER3D_CAMERA_FLOATS 22
GSR_API size_t gsr_filter3d_scratch_bytes(int64_t n);
GSR_API int gsr_filter3d_compute(int64_t n, const float* points, int32_t n_cameras, const float* camera_table, float near_plane,
                                 float k, float* filter, uint8_t* seen, uint32_t* count, void* scratch, size_t scratch_bytes,
                                 void* stream);
GSR_API int gsr_filter3d_apply(int64_t n, const float* opacities_act, const float* scales_act, const float* filter, int32_t raw,
                               float* opacities_out, float* scales_out, void* stream);
GSR_API int gsr_filter3d_apply_backward(int64_t n, const float* opacities_act, const float* scales_act, const float* filter,
                                        const float* g_opacities, const float* g_scales, float* v_opacities, float* v_scales,
                                        void* stream);

/* SH codebook compression: exact k-means (Lloyd) over (n, dim) rows, the vector quantisation of features_rest that
 * LightGaussian, Compact3D and "Compressed 3D Gaussian Splatting" apply after pruning.  features_rest in
 * the (3, k_rest, N) layout is such a matrix with dim = 3*k_rest.  No handle, no struct, nothing read back to the host.
 * Arrays are device, contiguous, float32 unless stated.  1 <= dim <= 48, 1 <= n_codes <= 65536, 0 <= n < 2^24 (the integer
 * sums below cannot overflow); indices are uint16.
 *
 * gsr_vq_assign: the nearest code of every row.  Every operation ONE rounded fp32 operation:
 *     n2_j  = fmaf(c_jd, c_jd, n2_j)      d = 0 .. dim-1, from 0
 *     h_j   = 0.5f * n2_j
 *     t_ij  = fmaf(x_id, c_jd, t_ij)      d ascending, from -h_j          ( = x.c - |c|^2/2: its maximum is the nearest code)
 *     index_i = the lowest j whose t_ij is not NaN and is >= every non-NaN t_ik ;  0 when every t_ik is NaN
 *     err_i   = sum over d of (x_id - c_jd)^2 for that j:  r = x_id - c_jd ;  err = fmaf(r, r, err), d ascending, from 0
 * The chain t_ij is what the f32-input matrix instruction computes with C = -h_j (two steps of d per instruction; dim is
 * padded with zero columns, and fmaf(0, 0, acc) changes at most the sign of a zero), so the search runs on the matrix cores
 * and is still this definition bit for bit, whatever the reduction order of the arg-max.
 *   indices : (n) uint16, fully overwritten.     err : (n), or NULL.
 *   prev    : (n) uint16 or NULL; may be `indices` itself.
 *   changed : one uint32, overwritten: the number of rows whose index differs from prev (all n when prev is NULL); or NULL.
 *   scratch : gsr_vq_scratch_bytes(n, n_codes, dim) bytes, 16-byte aligned (the codebook re-laid for the search: up to 220
 *             bytes per code, whole chunks of 256 codes).
 *
 * gsr_vq_accumulate: per-code INTEGER sums — any order of the rows gives the same bits, no float atomics:
 *     sums[j][d] += wq_i * rne(clamp(x_id, -128, 128) * 2^24)   as int64, j = indices[i] ;  a NaN x_id counts as 0
 *     wsum[j]    += wq_i                                        as uint64
 *   wq : (n) uint8 weights, NULL: every weight is 1.  sums (n_codes, dim) int64 and wsum (n_codes) uint64 are the caller's:
 *   accumulated into, never cleared.  255 * 2^31 * 2^24 < 2^63.
 *
 * gsr_vq_update: c_jd = (float)((double)sums[j][d] / ((double)wsum[j] * 16777216.0)) where wsum[j] > 0; a code with
 *   wsum[j] == 0 keeps its row bit for bit.  empty : one uint32, overwritten: the number of such codes; or NULL.
 *
 * gsr_vq_decode: rows_out[i] = codebook[indices[i]], (n, dim).
 *
 * An index >= n_codes (accumulate, decode) is read as n_codes - 1: wrong numbers, never an access outside the arrays.
 * GSR_E_INVALID_ARG, before anything touches the device: n, n_codes or dim out of range, a null array that is not optional,
 * a misaligned array (uint16: 2, uint32: 4, 64-bit sums: 8, scratch: 16 bytes), scratch_bytes too small.  n == 0: GSR_OK,
 * nothing is launched.  gsr_vq_scratch_bytes is 0 for n <= 0 and for sizes out of range. */
GSR_API size_t gsr_vq_scratch_bytes(int64_t n, int32_t n_codes, int32_t dim);
GSR_API int gsr_vq_assign(int64_t n, int32_t n_codes, int32_t dim, const float* rows, const float* codebook, const uint16_t* prev,
                          uint16_t* indices, float* err, uint32_t* changed, void* scratch, size_t scratch_bytes, void* stream);
GSR_API int gsr_vq_accumulate(int64_t n, int32_t n_codes, int32_t dim, const float* rows, const uint16_t* indices,
                              const uint8_t* wq, int64_t* sums, uint64_t* wsum, void* stream);
GSR_API int gsr_vq_update(int32_t n_codes, int32_t dim, const int64_t* sums, const uint64_t* wsum, float* codebook,
                          uint32_t* empty, void* stream);
GSR_API int gsr_vq_decode(int64_t n, int32_t n_codes, int32_t dim, const float* codebook, const uint16_t* indices,
                          float* rows_out, void* stream);

/* SH codebook fine-tuning: training THROUGH the codebook, the indices fixed and the code rows the parameters (DESIGN.md
 * section 24).  The pullback of rows[i] = codebook[indices[i]] is a scatter-add of n gradient rows into n_codes rows; here it
 * is a sum in a FIXED order, with no float atomics: the same bits in every run.  Same ranges and conventions as gsr_vq_*.
 *
 * Grouping (gsr_vq_group, once per set of indices).  Let c_i = min(indices[i], n_codes - 1).
 *     offsets[j] = #{ i : c_i < j },  j = 0 .. n_codes          (uint32, n_codes + 1 entries; offsets[n_codes] = n)
 *     order      = the row numbers 0 .. n-1 sorted by (c_i, i)   (uint32, n entries: the STABLE counting sort)
 * Both are uniquely determined: any correct implementation gives the same integers.
 *
 * Gradient (gsr_vq_codebook_grad, every step).  For code j, L_0 is the list of rows g[order[offsets[j]]], ...,
 * g[order[offsets[j+1] - 1]] — ascending row numbers.  With the radix R = GSR_VQ_SUM_RADIX:
 *     reduce(L):  if |L| = 1, that value, bit for bit (no add)
 *                 else reduce([chunk_0, chunk_1, ...]), chunk_c the serial fp32 sum of L[R c .. R c + R - 1]:
 *                      s = L[R c];  s = s + L[R c + 1];  s = s + L[R c + 2]; ...     (one rounded fp32 add each, ascending)
 *     g_codebook[j][d] = reduce(L_0)[d];   an empty code gets +0.0f
 * Every column d by itself; no fused operation, no double precision.  With n < 2^24 the recursion has at most four levels.
 * A NaN or Inf in a row reaches its own code and column only.  g_codebook is fully overwritten, whatever it held.
 * Error bound: a serial fp32 sum of at most 64 terms is within 63 * 2^-24 * sum|x| of the exact sum to first order; four
 * levels compound to less than 256 * 2^-24:  |g_codebook[j][d] - exact| <= 2^-16 * sum over the code's rows of |g[i][d]|.
 *
 *   g_rows     : row i starts at g_rows + i * row_stride floats; row_stride >= dim, 4-byte alignment is enough.  The (N, K, 3)
 *                vshs that gsr_backward writes is read in place with g_rows = vshs + 3, row_stride = 3 * K.
 *   order, offsets : as above, 4-byte aligned.  An order entry >= n is read as n - 1, offsets[j] as min(offsets[j], n), a code
 *                whose end lies before its start is empty: wrong numbers, never an access outside the arrays.
 *   g_codebook : (n_codes, dim).
 *   scratch    : gsr_vq_group_scratch_bytes(n, n_codes) / gsr_vq_codebook_grad_scratch_bytes(n, n_codes, dim) bytes, 16-byte
 *                aligned, written before it is read.  The gradient's holds the per-level slot prefixes (n_codes + 1 uint32 per
 *                level, made per call from offsets) and the partial rows: at level l at most floor(n / R^l) + min(n_codes, n).
 * Nothing is read back to the host; the launches are sized from n and n_codes alone, ceil(log_R n) levels (at least one).
 * GSR_E_INVALID_ARG, before anything touches the device, as for gsr_vq_*; also row_stride < dim.  n == 0: GSR_OK, nothing is
 * launched and nothing written.  The scratch sizes are 0 for n <= 0 and for sizes out of range. */
#define GSR_VQ_SUM_RADIX 64
GSR_API size_t gsr_vq_group_scratch_bytes(int64_t n, int32_t n_codes);
GSR_API int gsr_vq_group(int64_t n, int32_t n_codes, const uint16_t* indices, uint32_t* order, uint32_t* offsets,
                         void* scratch, size_t scratch_bytes, void* stream);
GSR_API size_t gsr_vq_codebook_grad_scratch_bytes(int64_t n, int32_t n_codes, int32_t dim);
GSR_API int gsr_vq_codebook_grad(int64_t n, int32_t n_codes, int32_t dim, const float* g_rows, int64_t row_stride,
                                 const uint32_t* order, const uint32_t* offsets, float* g_codebook,
                                 void* scratch, size_t scratch_bytes, void* stream);

/* The quantised model container: per-(block, column) ranges of an (n, cols) float32 group, 8- or 16-bit codes, the decode,
 * and the per-step quantise-dequantise pass - the last step of LightGaussian, Compact3D and "Compressed
 * 3D Gaussian Splatting": with the SH codebook of gsr_vq_* a degree-3 Gaussian is 6 + 3 + 1 + 3 + 4 + 2 = 19 bytes.  No
 * handle, nothing read back to the host.  Arrays are device, contiguous, float32 unless stated.
 *
 * A group is an (n, cols) row-major float32 array: 1 <= cols <= 48, 0 <= n < 2^31, 1 <= bits <= 16.  Codes are uint8 when
 * bits <= 8, else uint16, in the same (n, cols) layout.  block_rows is 0 (one block: the whole array) or a multiple of 64 in
 * [64, 1024]; block b holds rows [b*block_rows, min(n, (b+1)*block_rows)); n_blocks = 1 for block_rows = 0, else
 * ceil(n / block_rows).  ranges is (n_blocks, 2, cols) float32: [b][0][c] = lo, [b][1][c] = hi.
 *
 * Every operation below is ONE rounded fp32 operation, with subnormals kept.
 *
 *   ranges:  lo / hi = the minimum / maximum over the FINITE values of (block, column) in the order of the monotone integer
 *            key of the bits (so -0 < +0); a (block, column) without a finite value gets lo = hi = +0
 *   encode:  span = hi - lo;   ok = span > 0 && span < +Inf          (false also for NaN ranges)
 *            Lf = (float)(2^bits - 1);   inv = Lf / span;   step = span / Lf
 *            t = (x - lo) * inv          (the difference is rounded, then the product)
 *            t = isnan(t) ? 0 : fminf(fmaxf(t, 0), Lf);   q = (uint) rintf(t)   (ties to even);   !ok: q = 0
 *   decode:  x' = ok ? fmaf((float) min(q, 2^bits - 1), step, lo) : lo
 *   fake:    x' = decode(encode(x)), the codes never written; the same bits as the two calls
 *
 * kind = GSR_QUANT_UNIT_QUAT applies to cols = 4 rows (w, x, y, z).  ranges is not read and may be NULL; the range is the
 * constant [-1, 1].  In front of encode each row is normalised and sign-fixed:
 *     n2 = ((w*w + x*x) + y*y) + z*z ;  inv = 1.0f / sqrtf(n2) ;  s = (w < 0) ? -inv : inv ;  u_k = q_k * s
 * A row whose n2 is not > 0 or not finite becomes (1, 0, 0, 0).  Decode returns the dequantised u without renormalising (the
 * rasterizer normalises).
 *
 * gsr_quant_ranges: `ranges` is fully overwritten, whatever it held.  The one-block form reduces across workgroups through
 *   integer min / max atomics on the keys (no float atomics): the same bits in every run.
 * gsr_quant_fake: up to GSR_QUANT_MAX_GROUPS groups of the same n in ONE launch; rows_out == rows_in (in place) is allowed,
 *   any other overlap is not.
 * Error bound of a finite x in [lo, hi], ok:  |x' - x| <= step/2 + 9 ulp(max(|lo|, |hi|)), step and 1 / step
 * normal numbers (derived in DESIGN.md section 25).
 *
 * A code > 2^bits - 1 is read as 2^bits - 1, and damaged ranges give wrong numbers: never an access outside the arrays.
 * GSR_E_INVALID_ARG, before anything touches the device: n, cols, bits, kind or block_rows out of range, UNIT_QUAT with
 * cols != 4, a null array that is not optional, a misaligned array (float32: 4, uint16 codes: 2 bytes), n_groups outside
 * [0, GSR_QUANT_MAX_GROUPS].  n == 0: GSR_OK; gsr_quant_ranges with block_rows = 0 still writes its one block (+0, +0). */
#define GSR_QUANT_LINEAR 0
#define GSR_QUANT_UNIT_QUAT 1
#define GSR_QUANT_MAX_GROUPS 8
typedef struct gsr_quant_group {
    const float* rows_in;
    float* rows_out;
    int32_t cols;
    int32_t bits;
    int32_t kind;
    int32_t block_rows;
    const float* ranges;
} gsr_quant_group;
GSR_API int gsr_quant_ranges(int64_t n, int32_t cols, const float* rows, int32_t block_rows, float* ranges, void* stream);
GSR_API int gsr_quant_encode(int64_t n, int32_t cols, int32_t bits, int32_t kind, const float* rows, int32_t block_rows,
                             const float* ranges, void* codes, void* stream);
GSR_API int gsr_quant_decode(int64_t n, int32_t cols, int32_t bits, int32_t kind, const void* codes, int32_t block_rows,
                             const float* ranges, float* rows_out, void* stream);
GSR_API int gsr_quant_fake(const gsr_quant_group* groups, int32_t n_groups, int64_t n, void* stream);

/* TSDF fusion of rendered depth frames and surface-nets mesh extraction: one surface of the scene from the :rgbd / :rgbdn
 * frames, made on the device.  No handle, no struct, nothing read back to the host.
 *
 * The volume: nx x ny x nz samples; sample (i, j, k) sits at world origin + voxel_size*(i, j, k), each coordinate computed as
 * origin[a] + voxel_size*(float)idx; linear index l = i + nx*(j + ny*k), x fastest.
 *   volume : (nz, ny, nx, 2) float32, {tsdf, weight} per sample, 8-byte aligned.  A fresh volume is tsdf = 1, weight = 0.
 *   color  : (nz, ny, nx, 3) float32 or NULL.
 * Every side is in [1, 65535]; the extraction also asks for nx*ny*nz <= 2^30.
 *
 * gsr_tsdf_integrate: fuses one frame into the volume.  image: the rasterizer's frame (H, W, C >= 5), channel fastest:
 * channels 0..2 rgb, 3 the depth sum D, 4 alpha.  cam: R (column-major), t, focal and principal are read.  Per sample, in fp32,
 * every operation ONE rounded operation in this association:
 *     p = sample position ;  pc[r] = ((R[r]*px + R[r+3]*py) + R[r+6]*pz) + t[r] ;  z = pc[2]
 *     skip unless z > near_plane
 *     u = (fx*pc[0])/z + cx ;  v = (fy*pc[1])/z + cy ;  cx = principal[0]*(float)W, cy = principal[1]*(float)H
 *     iu = floor(u + 0.5), iv = floor(v + 0.5)       (the rasterizer's convention: 0-based pixel i samples u = i)
 *     skip unless 0 <= iu < W, 0 <= iv < H, alpha >= min_alpha       (a NaN anywhere skips)
 *     d = D/alpha ;  sdf = d - z ;  skip unless sdf >= -trunc ;  s = min(1, sdf/trunc)
 *     tsdf' = (tsdf*w + s)/(w + 1) ;  w' = w + 1 ;  colour' = (colour*w + clamp(rgb/alpha, 0, 1))/(w + 1) per channel
 * A skipped sample's entry is neither read nor written.  Views are fused in call order: run-to-run bit-identical.
 * GSR_E_INVALID_ARG: a side < 1 or > 65535, a null origin / cam / image / volume, a misaligned volume, voxel_size, trunc or
 * min_alpha not > 0, W or H < 1, C < 5, a non-positive focal length, a NaN near_plane.  A refused call touches nothing.
 *
 * Extraction, naive surface nets.  A sample is inside when tsdf < 0 and observed when weight > 0.  Cell (i, j, k) (i < nx-1,
 * ...) is active when its 8 corners are observed and not all on one side; every active cell gives one vertex, in ascending
 * cell index i + (nx-1)*(j + (ny-1)*k): local = the mean of the crossing points a + s*(b - a), s = Ta/(Ta - Tb), over the
 * cell's sign-changing edges, summed in this order: the 4 x-edges, then the y-edges, then the z-edges, within an axis the two
 * fixed coordinates counting up with the lower axis fastest; world = origin + voxel_size*((float)idx + local).  The vertex
 * colour is the sum of the 8 corners' colours in corner order (corner = dx + 2*dy + 4*dz) times 0.125.  Every grid edge
 * p -> p + e_a (a = 0, 1, 2) whose ends are observed and on different sides gives one quad when the four cells around it
 * exist and are active: with (b, c) = (a+1, a+2) mod 3, c0 = p - e_b - e_c, c1 = p - e_c, c2 = p, c3 = p - e_b, written as the
 * triangles (c0, c1, c2), (c0, c2, c3) of vertex ids when p is inside and (c3, c2, c1), (c3, c1, c0) when p + e_a is: the normal
 * points from inside to outside.  Quads ascend in 3*l(p) + a.
 *   gsr_mesh_scratch_bytes: 4 bytes per cell, 8 per run of whole rows of about 2048 cells, 8 more; 0 when the volume has no cell (or is refused).
 *   gsr_mesh_count : counts[0] <- the vertices, counts[1] <- the quads (two uint32 on the device); leaves in the scratch what
 *                    gsr_mesh_emit needs.  scratch: gsr_mesh_scratch_bytes, 8-byte aligned.
 *   gsr_mesh_emit  : after gsr_mesh_count on the same volume and scratch.  Writes the first min(vertices, max_vertices) rows of
 *                    vertices (x, y, z) and vertex_colors, and the first min(2*quads, max_faces) rows of faces (int32 x 3), and
 *                    nothing beyond them.  color and vertex_colors are given together or both NULL.
 * A volume without a cell (a side of 1) is an empty mesh: counts <- {0, 0}, no scratch is needed, nothing else is written. */
GSR_API int gsr_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, const float* origin, float voxel_size, float trunc, int32_t W,
                               int32_t H, int32_t C, const float* image, const gsr_camera* cam, float min_alpha, float near_plane,
                               float* volume, float* color, void* stream);
GSR_API size_t gsr_mesh_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
GSR_API int gsr_mesh_count(int32_t nx, int32_t ny, int32_t nz, const float* volume, uint32_t* counts, void* scratch,
                           size_t scratch_bytes, void* stream);
GSR_API int gsr_mesh_emit(int32_t nx, int32_t ny, int32_t nz, const float* origin, float voxel_size, const float* volume,
                          const float* color, const void* scratch, size_t scratch_bytes, int64_t max_vertices, int64_t max_faces,
                          float* vertices, float* vertex_colors, int32_t* faces, void* stream);

/* The non-finite gradient guard of `step!` under GSP_DEBUG (src/training.jl:772-777: `isfinite(sum(∇ᵢ))` per parameter)
 * and the per-parameter counts of `nonfinite_gradient_report` (:534-552), in one pass over up to GSR_ADAM_MAX_GROUPS
 * gradient arrays of n_rows Gaussians each (rows of row_words floats; row_words = 0 skips an empty array):
 *   counts[g]    = number of Gaussians whose row holds a NaN or ±Inf          (device, n_groups)
 *   first_bad[g] = smallest such Gaussian index, 0xFFFFFFFF if none           (device, n_groups) */
GSR_API int gsr_count_nonfinite(const float* const* arrays, const int32_t* row_words, int32_t n_groups, int64_t n_rows,
                                uint32_t* counts, uint32_t* first_bad, void* stream);

/* The vertex rows of a 3DGS .ply scene (`export_ply` / `import_ply`, src/gaussians.jl:140-247):
 * per Gaussian  x y z | nx ny nz (0) | f_dc_0..2 | f_rest_0..3·k_rest-1 (channel-major) | opacity | scale_0..2 | rot_0..3,
 * i.e. 17 + 3·k_rest floats of RAW parameters.  gsr_ply_pack_rows gathers the model's arrays (device, the reference's
 * layouts: points (3,N), features_dc (3,1,N), features_rest (3,k_rest,N), opacities (1,N), scales (3,N), rotations (4,N))
 * into the row matrix `rows` (device, N x (17 + 3·k_rest)); gsr_ply_unpack_rows scatters a row matrix back (normals are
 * ignored).  Header and disk I/O stay with the host. */
GSR_API int gsr_ply_pack_rows(int64_t n, int32_t k_rest, const float* points, const float* features_dc,
                              const float* features_rest, const float* opacities, const float* scales, const float* rotations,
                              float* rows, void* stream);
GSR_API int gsr_ply_unpack_rows(int64_t n, int32_t k_rest, const float* rows, float* points, float* features_dc,
                                float* features_rest, float* opacities, float* scales, float* rotations, void* stream);

/* Bilateral grid appearance correction (src/bilateral_grid.jl; switched on by `use_bilateral_grid`, src/utils.jl:56-63;
 * used by `step!`, training.jl:676-681,703-706,784-790).  Each training image owns a (gx,gy,gz,12) grid of 3x4 affine
 * colour transforms, coefficient (d-1)*4 + c mapping input channel c (r, g, b, 1) to output channel d; all grids of a
 * trainer are one (gx,gy,gz,12,n) array.  Images are (C,W,H), C = 3, 5 or 8 (the rasterizer's modes).  All pointers
 * device, all sizes >= 1.  Every entry point refuses gz > 64 (the pullback's LDS) and gx*gy*gz > 16384 (the TV and
 * the Adam tail stage one grid slab in 64 KiB of LDS; one limit for all four, so any grid they accept works with all
 * of them).  Every result is run-to-run bit-identical: no float atomics anywhere.
 *
 * gsr_bilateral_slice_forward  : `bilateral_slice(image, grid)` (bilateral_grid.jl:75-85,152-175): channels 0-2 of
 *                                `out` get the corrected rgb, channels >= 3 are copied, so `out` can go to
 *                                gsr_loss_l1_ssim in place of the render.
 * gsr_bilateral_slice_backward : its pullback (bilateral_grid.jl:87-100,177-242).  vout: the cotangent of `out`;
 *                                vimage (may be vout: in place) gets ∇image, channels >= 3 the cotangent unchanged — the
 *                                loss head's buffer stays valid for GSR_GRADS_COLOR_COTANGENT; vgrid (gx,gy,gz,12) gets
 *                                the FULL ∇grid of the view (overwritten).  scratch: gsr_bilateral_scratch_bytes(W, H,
 *                                gx, gy, gz) bytes.
 * gsr_bilateral_tv             : weight · tv_loss(grids) (bilateral_grid.jl:102-119) into *loss_out (device) and,
 *                                unless grad_out is NULL, weight · ∇tv_loss into grad_out (gx,gy,gz,12,n).  scratch:
 *                                gsr_bilateral_tv_scratch_bytes(n_images) bytes.
 * gsr_bilateral_adam_tail      : `NU.step!(bgrid.optimizer, bgrid.grids, ∇grids)` (training.jl:784-790) where ∇grids =
 *                                tv_weight · ∇tv_loss(grids) + the slice gradient `vgrid_view` of view `view` (0-based),
 *                                in one pass over all grids; *tv_loss_out (device) = tv_weight · tv_loss of the grids
 *                                BEFORE the update (the TV term of the step's loss, training.jl:703-706).  θ, μ, ν
 *                                bit-identical to gsr_bilateral_tv (gradient) + adding vgrid_view to view `view` +
 *                                gsr_adam_step.  current_step counts from 1 (after the increment).  scratch:
 *                                gsr_bilateral_tv_scratch_bytes(n_images) bytes. */
GSR_API size_t gsr_bilateral_scratch_bytes(int32_t W, int32_t H, int32_t gx, int32_t gy, int32_t gz);
GSR_API size_t gsr_bilateral_tv_scratch_bytes(int32_t n_images);
GSR_API int gsr_bilateral_slice_forward(int32_t W, int32_t H, int32_t C, const float* image, const float* grid, int32_t gx,
                                        int32_t gy, int32_t gz, float* out, void* stream);
GSR_API int gsr_bilateral_slice_backward(int32_t W, int32_t H, int32_t C, const float* image, const float* grid, int32_t gx,
                                         int32_t gy, int32_t gz, const float* vout, float* vimage, float* vgrid,
                                         void* scratch, size_t scratch_bytes, void* stream);
GSR_API int gsr_bilateral_tv(int32_t n_images, int32_t gx, int32_t gy, int32_t gz, const float* grids, float weight,
                             float* loss_out, float* grad_out, void* scratch, size_t scratch_bytes, void* stream);
GSR_API int gsr_bilateral_adam_tail(int32_t n_images, int32_t gx, int32_t gy, int32_t gz, float* grids, float* mu, float* nu,
                                    const float* vgrid_view, int32_t view, float tv_weight, float lr, uint32_t current_step,
                                    float beta1, float beta2, float eps, float* tv_loss_out, void* scratch,
                                    size_t scratch_bytes, void* stream);

/* Geometry regularisation of :rgbdn training (src/geometry_regularization.jl; switched on by `use_normal_loss`, used by
 * `step!`, training.jl:625-733): the only producer of a cotangent on the depth, alpha and normal channels.  The frame is
 * the rasterizer's :rgbdn image (8,W,H): channels 0-2 rgb, 3 blended depth D, 4 alpha, 5-7 the blended normal; C must
 * be 8.  The pixel rays are computed in the kernels from cam->focal and cam->principal by the fp32 expression of
 * `pixel_rays` (geometry_regularization.jl:53-62); nothing else of `cam` is read.  All array pointers device.  Every
 * result is run-to-run bit-identical: no float atomics anywhere; nothing is read back by the host.
 *
 * gsr_normal_loss_forward  : weight · depth_normal_consistency_loss (geometry_regularization.jl:87-183) into *loss_out,
 *                            (Σw, count) of the valid centres into stats_out[0..1], and, unless weights_out is NULL, the
 *                            detached weight map (W,H) (0 on the border and on invalid centres).  The "too little
 *                            evidence" gate (count < 64 or Σw < 16; W <= 2 or H <= 2) is applied on the device: loss 0.
 *                            Every decision of the validity mask is the reference's fp32 expression.  One intended
 *                            deviation: a centre with w = 0 contributes exactly nothing, also when its stencil holds
 *                            NaN / Inf (the reference's `sum(w .* (1 .- cosθ))` would turn NaN on 0 · NaN).
 *                            scratch: gsr_normal_loss_scratch_bytes(W, H) bytes; the backward of the same image reads it.
 * gsr_normal_loss_backward : ADDS weight · ∂loss/∂(D, alpha, normal) onto channels 3..7 of vpixels (8,W,H); channels 0..2
 *                            are not touched, pixels that receive nothing are not written, a gated view adds nothing.  So
 *                            the loss head's zeros, or another depth term, compose with it.  `scratch` is the one
 *                            gsr_normal_loss_forward filled for the same image, camera and (any) weight: the gate and the
 *                            normaliser are read from it on the device.  vpixels must not be the image.  A vpixels this
 *                            was added onto must NOT go to gsr_backward with GSR_GRADS_COLOR_COTANGENT.
 * gsr_flatten_loss         : weight · flatten_loss(scales) (geometry_regularization.jl:197-211) = weight · mean_i
 *                            exp(min_j scales_raw[j, i]) into *loss_out (0 for n = 0); scales_raw (scale_dims, N), raw
 *                            (pre-exp), scale_dims 1 or 3.  Unless vscales is NULL, the gradient w.r.t. the ACTIVATED
 *                            scale — the constant weight / n on the first axis that holds the minimum (the reference's
 *                            cumsum tie-break; row 0 for scale_dims = 1) — is ADDED onto vscales (3,N), the array
 *                            gsr_backward wrote: gsr_prologue_backward / gsr_trainer_tail_step then yield the reference's
 *                            weight · exp(s) / n on the raw scale.  The fused gsr_backward_trainer_tail never
 *                            materialises ∇scales: steps with the regulariser on run gsr_backward + gsr_flatten_loss +
 *                            gsr_trainer_tail_step.  scratch: gsr_flatten_loss_scratch_bytes(n) bytes (may be NULL for
 *                            n = 0). */
GSR_API size_t gsr_normal_loss_scratch_bytes(int32_t W, int32_t H);
GSR_API int gsr_normal_loss_forward(int32_t W, int32_t H, int32_t C, const float* image, const gsr_camera* cam, float weight,
                                    float* loss_out, float* stats_out, float* weights_out, void* scratch,
                                    size_t scratch_bytes, void* stream);
GSR_API int gsr_normal_loss_backward(int32_t W, int32_t H, int32_t C, const float* image, const gsr_camera* cam, float weight,
                                     float* vpixels, const void* scratch, size_t scratch_bytes, void* stream);
GSR_API size_t gsr_flatten_loss_scratch_bytes(int32_t n);
GSR_API int gsr_flatten_loss(int32_t n, int32_t scale_dims, const float* scales_raw, float weight, float* loss_out,
                             float* vscales, void* scratch, size_t scratch_bytes, void* stream);

/* Anchored depth supervision of :rgbd / :rgbdn training (src/depth_supervision.jl:406-536; switched on by `use_depth_loss`,
 * used by `step!`, training.jl:604-620,709-718): `depth_target` and `ssi_depth_loss` on the device.  The frame is the
 * rasterizer's image (C,W,H), C = 5 (:rgbd) or 8 (:rgbdn): channel 3 is the blended depth D, channel 4 alpha; nothing else
 * of a record is read.  `prior` is the (W,H) relative depth prior, `anchor` its per-camera affine alignment (DepthAnchor,
 * depth_supervision.jl:51-57; `disparity` > 0 selects the inverse-depth model), `qstep` the quantisation step of the
 * prior's encoding.  The target, the deadband half-width and the masks are built in the kernels from `prior` and `anchor`:
 *   affine = a·t + b (a multiply, then an add);  valid = isfinite(t) & t > 0 & affine > 0;
 *   target = min(affine, 1/floor) (disparity) or 1/(affine + floor) (depth);  half_band = 0.5·qstep·|a| (· target² in the
 *   depth model);  far_extrap = target < p_far
 * every decision in the reference's fp32 expression.  All array pointers device; nothing is read back by the host; no
 * float atomics anywhere: every result is run-to-run bit-identical.
 *
 * Intended deviation from the reference: a pixel with w = 0 (invalid, or clamp(alpha,0,1) <= 1e-3) contributes exactly
 * nothing to the loss, to σ and to the gradients, also when its D or its prior is NaN / Inf — it is selected out, not
 * multiplied by zero (the reference's `sum(w .* ...)` would turn NaN on 0 · NaN).  The same holds for a forward-difference
 * pair whose min(w_s, w_s') = 0.  A non-finite alpha counts as 0, in Σα and as a weight.
 *
 * gsr_depth_target         : the maps alone: target_out (W,H), half_band_out (W,H), flags_out (W,H) bytes with bit 0 =
 *                            valid and bit 1 = far_extrap; each may be NULL.
 * gsr_depth_loss_forward   : weight · ssi_depth_loss into *loss_out = weight · (data + lambda_grad · (grad_x + grad_y)) /
 *                            max(Σα, 1); unless NULL, stats_out[0..3] = (Σα, Σw_supported, μ, σ) (Σα before the max) and
 *                            the three maps as above.  scratch: gsr_depth_loss_scratch_bytes(W, H) bytes, 16-byte aligned
 *                            (a header, per-tile partials and a 16-byte record per pixel); the backward reads it.
 * gsr_depth_loss_backward  : ADDS weight · ∂loss/∂(D, alpha) onto channels 3 and 4 of vpixels (C,W,H); σ, the weights and
 *                            Σα are detached, as in the reference.  Channels 0..2 (and 5..7 for C = 8) are not touched, a
 *                            pixel that receives nothing is not written: the loss head's zeros and the depth-normal term
 *                            compose with it.  `scratch` is the one gsr_depth_loss_forward filled for the same image,
 *                            prior, anchor and qstep (lambda_grad and weight may differ).  vpixels must not be the image.
 *                            A vpixels this was added onto must NOT go to gsr_backward with GSR_GRADS_COLOR_COTANGENT. */
typedef struct gsr_depth_anchor { float a, b, floor, disparity, p_far; } gsr_depth_anchor;
GSR_API size_t gsr_depth_loss_scratch_bytes(int32_t W, int32_t H);
GSR_API int gsr_depth_target(int32_t W, int32_t H, const float* prior, const gsr_depth_anchor* anchor, float qstep,
                             float* target_out, float* half_band_out, uint8_t* flags_out, void* stream);
GSR_API int gsr_depth_loss_forward(int32_t W, int32_t H, int32_t C, const float* image, const float* prior,
                                   const gsr_depth_anchor* anchor, float qstep, float lambda_grad, float weight, float* loss_out,
                                   float* stats_out, float* target_out, float* half_band_out, uint8_t* flags_out, void* scratch,
                                   size_t scratch_bytes, void* stream);
GSR_API int gsr_depth_loss_backward(int32_t W, int32_t H, int32_t C, const float* image, const float* prior,
                                    const gsr_depth_anchor* anchor, float qstep, float lambda_grad, float weight, float* vpixels,
                                    const void* scratch, size_t scratch_bytes, void* stream);

/* Sky dome, the per-pixel part (src/sky_dome.jl; switched on by `use_sky_dome` / `use_sky_loss`, used by `step!`,
 * training.jl:593-598,634-639,673-676,721-725, and by `validate`, :512-516).  The dome itself — a frozen shell of Gaussians
 * with trainable colours — is rendered by a second, independent :rgb handle (gsr_create with far_plane = 4·radius;
 * sky_dome.jl:144,186-195); these entry points do the work the step adds per pixel.  New functions, no struct change:
 * GSR_ABI_VERSION stays.  `image` is the scene's frame (C,W,H), C = 5 (:rgbd) or 8 (:rgbdn), rendered over a ZERO background
 * (training.jl:596): channels 0..2 rgb, 4 alpha — the raw channel, never clamped (sky_dome.jl:306-309).  C = 3 is
 * GSR_E_INVALID_ARG: :rgb has no alpha row (sky_dome.jl:221, training.jl:349).  `sky_rgb` is the dome's frame (3,W,H),
 * `sky_weight` the (W,H) sky mask in [0, 1] or NULL.  All array pointers device; no float atomics: every result is run-to-run
 * bit-identical, and every argument is checked before the device is touched.
 *
 * gsr_sky_scratch_bytes       : bytes of `scratch` for a W x H frame (16 + 16 per 1024 pixels); 8-byte aligned.
 * gsr_sky_composite_forward   : `composite_sky` (sky_dome.jl:246-250): out[0..2] = image[0..2] + (1 - alpha) · sky_rgb (a product,
 *                               then a sum, per channel).  `out` (C,W,H) may be `image` itself — the in-place `composite_sky!`
 *                               (:217-228); otherwise channels >= 3 are copied, so `out` is a whole frame.  With `sky_weight`
 *                               the same pass also gives `sky_opacity_loss` (:315-320): *loss_out = loss_weight · Σ w·alpha² /
 *                               max(Σw, 1), sums in double in a fixed order, and leaves 1 / max(Σw, 1) in scratch[0] for the
 *                               backward; a mask needs `loss_out` and `scratch`.  Without a mask neither is touched (both may
 *                               be NULL).  A mask of zeros gives exactly 0.
 * gsr_sky_composite_backward  : given `vpixels` (C,W,H) whose channels 0..2 hold the cotangent g of the composite (the loss
 *                               head's output; channels >= 3 hold whatever other terms added already): vsky (3,W,H) =
 *                               (1 - alpha) · g, and ADDS -(g · sky_rgb) [+ loss_weight · 2·w·alpha / max(Σw, 1) with a mask] onto
 *                               channel 4 of vpixels as ONE fp32 add; g · sky = (g0·s0 + g1·s1) + g2·s2, the mask term is
 *                               ((2·w)·alpha) · (loss_weight · scratch[0]), and the sum added is (-(g · sky)) + the mask term.
 *                               Channels 0..3 and >= 5 are not written (∂composite/∂image = 1).  `scratch` is the one the
 *                               forward filled for the same image and mask (NULL without a mask).  `image` is the SCENE frame,
 *                               not the composite, unless the composite was made in place (alpha is the same in both).
 *                               vpixels must not be the image.  A vpixels this was added onto must NOT go to gsr_backward
 *                               with GSR_GRADS_COLOR_COTANGENT. */
GSR_API size_t gsr_sky_scratch_bytes(int32_t W, int32_t H);
GSR_API int gsr_sky_composite_forward(int32_t W, int32_t H, int32_t C, const float* image, const float* sky_rgb,
                                      const float* sky_weight, float loss_weight, float* out, float* loss_out, void* scratch,
                                      void* stream);
GSR_API int gsr_sky_composite_backward(int32_t W, int32_t H, int32_t C, const float* image, const float* sky_rgb,
                                       const float* sky_weight, float loss_weight, float* vpixels, float* vsky,
                                       const void* scratch, void* stream);

/* The evaluation head: what `validate(trainer; quantize)` (src/training.jl:487-532) computes per test view, and the 8-bit
 * picture `gl_texture` / `to_image` (src/rasterizer.jl:155-182, scripts/render-views.jl) make of a frame.  New functions, no
 * struct change: GSR_ABI_VERSION stays.  `image` is the rasterizer's frame (C,W,H), channel fastest, C >= 3: channels 0..2 are
 * scored; `sky_rgb` (3,W,H) or NULL: when given, C >= 5 and the scored colour is image[c] + (1 - image[4]) · sky_rgb[c], a
 * product, then a sum (sky_dome.jl:246-250, training.jl:514-517) — the arithmetic of gsr_sky_composite_forward, so scoring
 * with `sky_rgb` equals scoring that function's output, bit for bit.  One arithmetic: every fp32 operation as written, IEEE
 * divisions, no contraction (gsr_ssim_precision does not apply).  All array pointers device; every argument is checked
 * before the device is touched; no float atomics: results are run-to-run bit-identical.
 *
 * gsr_eval_scratch_bytes : bytes of `scratch` for a W x H frame (72 per 54 x 32 strip of it); 8-byte aligned; 0 for W, H < 1.
 * gsr_eval_metrics       : exactly one of `target_f32` — (W,H,3) planar, as gsr_loss_l1_ssim takes it — and `target_u8` —
 *                          (3,W,H) bytes, channel fastest, as the dataset stores images (dataset.jl:253-260), converted in
 *                          the loads as (float)u · (1.0f/255.0f) (`Float32.(image) .* (1f0/255f0)`) — is non-NULL; neither
 *                          needs more alignment than its element size.  quantize != 0 applies `quantize8` (utils.jl:118)
 *                          after the composite: q(x) = floorf(fminf(fmaxf(x, 0), 1) · 255.0f + 0.5f) · (1.0f/255.0f), each
 *                          operation its own fp32 operation in that order; ±Inf clamp like any value, NaN is unspecified.
 *                          `ssim_map` (W,H,3) planar or NULL: the SSIM map of the scored colours, the train = false map of
 *                          fused_ssim.jl:34-238 (C1 = 0.01², C2 = 0.03², zero padding; symmetric pairs d = 1..5, centre tap
 *                          last), bit-identical to the CPU oracle; it must not be `image`.  `out`: 4 floats {mean SSIM, MSE
 *                          (utils.jl:107), PSNR, mean |x - y|} over the 3·W·H scored values.  Per value the map, d = x - y
 *                          and |d| are fp32, d² is (double)d · (double)d; the sums are double in a fixed order (csrc/eval.hip)
 *                          and each mean is (float)(Σ / n), rounded once.  PSNR = (float)(-10 · log10(Σd² / n)) in double;
 *                          the reference evaluates 20f0 · log10(1f0 / sqrt(mse)) on the host in Float32 (utils.jl:109):
 *                          the two agree to fp32 rounding, and mse = 0 gives +Inf in both.
 *                          GSR_E_INVALID_ARG: W or H < 1, C < 3, `sky_rgb` with C < 5, a frame of 2^32 elements or more (or
 *                          a row of 2^32 bytes or more), NULL image / out / scratch, both targets or neither, ssim_map ==
 *                          image, a scratch that is not 8-byte aligned.
 * gsr_frame_rgb8         : the 8-bit picture of the same colours: rgb8_out (3,W,H) bytes, channel fastest — the dataset's
 *                          own layout, so an exported frame can be fed back as `target_u8` — each (uint8) floorf(fminf(fmaxf(
 *                          x, 0), 1) · 255.0f + 0.5f), the integer inside q (one device function serves both entry
 *                          points).  flip_rows != 0 reverses the row order (`gl_texture`'s reverse!(…; dims=3)).  No alignment
 *                          is asked of rgb8_out.  Rejects what gsr_eval_metrics rejects of W, H, C, image and sky_rgb. */
GSR_API size_t gsr_eval_scratch_bytes(int32_t W, int32_t H);
GSR_API int gsr_eval_metrics(int32_t W, int32_t H, int32_t C, const float* image, const float* sky_rgb,
                             const float* target_f32, const uint8_t* target_u8, int32_t quantize, float* ssim_map,
                             float* out, void* scratch, void* stream);
GSR_API int gsr_frame_rgb8(int32_t W, int32_t H, int32_t C, const float* image, const float* sky_rgb, int32_t flip_rows,
                           uint8_t* rgb8_out, void* stream);

/* Geometry frames: the pictures the reference makes of the depth, alpha and normal channels of a frame — on the host, after
 * copying the frame out and sorting its depths — (scripts/render-views.jl:264-308,390-407 `depth_image` / `normal_image`;
 * src/rasterization/rasterizer.jl:163-198 `gl_depth` / `to_depth`; src/gui/worker.jl:688-726 `handle_pick!`).  New functions, no
 * struct change: GSR_ABI_VERSION stays.  `image` is the rasterizer's frame (C,W,H), channel fastest: 0..2 rgb, 3 depth, 4
 * alpha, 5..7 normal.  One arithmetic (csrc/frames.hip states it operation by operation): fp32 as written, IEEE divisions and
 * square roots, no contraction.  Per pixel: covered = alpha >= min_alpha (a NaN alpha is not covered), e = depth /
 * fmaxf(alpha, min_alpha).  All array pointers device unless said otherwise; every argument is checked before the device is
 * touched; integer atomics only: results are run-to-run bit-identical.
 *
 * gsr_frames_scratch_bytes : bytes of `scratch` for gsr_depth_scale on a W x H frame (32 832 + 4·W·H, rounded up to 8); 0 for
 *                            W, H < 1.
 * gsr_depth_scale          : the white level of `depth_image` (render-views.jl:272-277), left on the device.  C >= 5;
 *                            `percentile` in (0, 100].  stats_out, 16 bytes: {float scale; uint32 n; uint32 a_bits; uint32
 *                            b_bits}.  v = the covered e in ascending order (Julia's `sort`: -0.0 < +0.0; NaN unspecified),
 *                            n their number; Statistics.jl's definition 7 in double: p = percentile / 100, m = 1 - p,
 *                            aleph = fma((double)n, p, m), j = clamp(trunc(aleph), 1, n - 1), γ = clamp(aleph - j, 0, 1);
 *                            a = v[j], b = v[j+1] (1-based; n == 1: a = b = v[1]); d = b - a in fp32; q = (double)a + γ ·
 *                            (double)d, two double operations; scale = fmaxf((float)q, 1e-6f).  n == 0: scale = 1, a_bits =
 *                            b_bits = 0.  The selection is an exact radix select (11 + 11 + 10 key bits): one pass reads
 *                            depth and alpha of every pixel and writes a 4-byte key, two more passes read only the keys;
 *                            no host round trip between n and the rank.  This is a + γ·(b - a) as Statistics.jl evaluates
 *                            it for a Float32 vector and a Float64 p; newer Statistics.jl versions take (1-γ)a + γb when
 *                            a ≉ b, older ones n·p + m without the fma, and nobody has run Julia against this: n, a_bits
 *                            and b_bits are the pinned part.  `scratch`: 8-byte aligned, gsr_frames_scratch_bytes(W, H).
 * gsr_frame_depth16        : depth16_out (W,H) uint16, rows as the frame's rows, reversed with flip_rows != 0 (as
 *                            gsr_frame_rgb8); 2-byte aligned.  x = covered ? e : 0 with expected != 0 (C >= 5: `depth_image`),
 *                            x = depth with expected == 0 (C >= 4; with depth_max = 50 this is `to_depth` / `gl_depth`).
 *                            Exactly one of depth_max > 0 (a host float) and scale_dev (device pointer to the float
 *                            gsr_depth_scale wrote) is given.  inv = 1.0f / scale, one division; y = fminf(fmaxf(x · inv, 0),
 *                            1); word = (uint16) floorf(y · 65535.0f + 0.5f): gsr_frame_rgb8's quantiser form at 16 bits.
 *                            FixedPointNumbers' N0f16(y) rounds to nearest: the two can differ only on exact .5 ties.
 * gsr_frame_normal8        : `normal_image` (render-views.jl:291-308).  C >= 8; normal8_out (3,W,H) bytes, channel fastest,
 *                            any alignment.  n = N / fmaxf(alpha, min_alpha), three divisions; len = sqrtf((nx² + ny²) +
 *                            nz²); degenerate = len < 1e-6f || !covered; n = n / fmaxf(len, 1e-6f); a degenerate pixel is
 *                            (0,0,0).  R_c2w: nine HOST floats, column-major (transpose(camera.R)), or NULL; when given,
 *                            row i of R_c2w·n = (r[i]·x + r[i+3]·y) + r[i+6]·z and a degenerate pixel stays zero — the
 *                            reference multiplies through BLAS, whose order is not known: this order is ours.
 *                            byte = (uint8) floorf(fminf(fmaxf(c · 0.5f + 0.5f, 0), 1) · 255.0f + 0.5f), the device function
 *                            gsr_frame_rgb8 uses.
 * gsr_pick_point           : `handle_pick!`: the orbit target under a pixel.  C >= 4; px, py 1-based; 0 <= half_window <= 16;
 *                            out4: four device floats {x, y, z, count}.  Over the window [px-hw, px+hw] x [py-hw, py+hw]
 *                            clipped to the frame, z = (Σ of the raw depths > 1e-2f, in fp32 in a fixed order: csrc/frames.hip)
 *                            / count; p_cam = ((px - 0.5f - principal[0]·W)·z / fx, (py - 0.5f - principal[1]·H)·z / fy, z);
 *                            target = Rᵀ·p_cam + camera_center from the host fields of `cam` (the reference inverts the
 *                            4x4 pose; for a rigid pose that is the transpose).  count == 0 or a pixel outside the frame:
 *                            {0,0,0,0} and GSR_OK (the reference returns silently).
 * GSR_E_INVALID_ARG: W or H < 1; C below what the call needs; a frame of 2^32 elements or more; NULL image, output or `cam`,
 * NULL scratch or stats_out; percentile outside (0, 100] or NaN; min_alpha not > 0; both depth_max > 0 and scale_dev, or
 * neither; depth_max negative, NaN or Inf; half_window outside [0, 16]; a scratch that is not 8-byte aligned, a depth16_out
 * that is not 2-byte aligned. */
GSR_API size_t gsr_frames_scratch_bytes(int32_t W, int32_t H);
GSR_API int gsr_depth_scale(int32_t W, int32_t H, int32_t C, const float* image, float min_alpha, double percentile,
                            void* stats_out, void* scratch, void* stream);
GSR_API int gsr_frame_depth16(int32_t W, int32_t H, int32_t C, const float* image, int32_t expected, float min_alpha,
                              float depth_max, const float* scale_dev, int32_t flip_rows, uint16_t* depth16_out, void* stream);
GSR_API int gsr_frame_normal8(int32_t W, int32_t H, int32_t C, const float* image, float min_alpha, const float* R_c2w,
                              uint8_t* normal8_out, void* stream);
GSR_API int gsr_pick_point(int32_t W, int32_t H, int32_t C, const float* image, const gsr_camera* cam, int32_t px, int32_t py,
                           int32_t half_window, float* out4, void* stream);

/* The MCMC densification strategy of the reference on the device (src/mcmc.jl, `strategy = :mcmc`, src/strategy.jl:16): the
 * number of Gaussians only grows (up to max_cap), dead Gaussians are relocated onto alive ones sampled ∝ opacity with the
 * Eq. 9 opacity / scale correction, position noise keeps the chain exploring and an L1 on opacity and scale produces the
 * dead Gaussians to recycle.  The host keeps the reference's control flow (post_train_step! -> relocate_gaussians! ->
 * add_gaussians! -> inject_noise!, mcmc.jl:109-124); every per-Gaussian pass — in the reference a chain of device->host
 * copies, host loops and re-uploads (:135-258) — is one of these launches.  All array pointers device, caller-owned; arrays
 * in the reference's layouts (opacities (1,N), scales (scale_dims,N) with scale_dims 3, or 1 for an isotropic model,
 * rotations (4,N), points (3,N)), raw (pre-activation) unless said otherwise.  Rows are addressed 0-based.
 *
 * Two intended deviations from the reference:
 *  1. Randomness.  The reference draws from the host's `rand()` (mcmc.jl:224) and the device's `randn` (:310), which nothing
 *     can reproduce.  Here every random number is a pure function of (seed, index, draw) of the counter-based generator
 *     gsr_split_transform uses (a 32-bit integer mixer; uniforms and Box-Muller normals on top of it); a host restatement
 *     reproduces its integer part bit for bit.  The caller passes a different `seed` on every round / step.
 *  2. Multinomial sampling in integers.  The reference takes a float64 `cumsum` of the float32 opacities and
 *     `searchsortedfirst(cw, rand()·total)` (:220-225); a parallel scan cannot match a sequential float sum bit for bit, and
 *     one ulp flips a discrete choice.  Here the weight of row i is q_i = floor(sigmoid(opacity_i) · 2^30) as uint32 (0 for
 *     a dead row when relocating), prefix sums are uint64 — exact, independent of the order; below 2^51 at 2 M rows —, draw
 *     j takes r_j = mulhi64(h_j, total) with h_j 64 generator bits keyed by (seed, j), and selects the FIRST row whose
 *     inclusive prefix is > r_j.  With the strict inequality a zero-weight row is never selected, so one scan over all N
 *     rows replaces the reference's `alive[...]` indirection.  The distribution equals the reference's to 2^-30 per weight.
 *
 * gsr_mcmc_weights           : q[n], and unless `dead` is NULL dead[n] = (sigmoid(o) <= min_opacity) | (max_j scales_raw[j]
 *                              > log_max_scale) with q = 0 on dead rows (mcmc.jl:135-140); log_max_scale =
 *                              log(max_scale · extent) is evaluated by the host, as in the reference, so the compare needs
 *                              no device transcendental.  dead NULL: every row is weighted (add_gaussians!, :189-190).
 * gsr_mcmc_sample            : multinomial_sample (:220-225) + the multiplicities of split_sampled! (:237-240): scans q[n],
 *                              writes the m draws to sampled[m], zeroes counts[n] and counts the draws into it (integer
 *                              atomics: order-independent), and writes Σq to *total (a device 64-bit word).  total = 0
 *                              (the reference's `total > 0 || return Int[]`): sampled is not written, counts are zeros —
 *                              the host reads *total before it uses them.  m = 0: nothing is touched.  scratch:
 *                              gsr_mcmc_sample_scratch_bytes(n) bytes, 8-byte aligned.
 * gsr_mcmc_split_sampled     : split_sampled! (:232-260) in place: every row with counts[i] > 0 gets Eq. 9 with ratio =
 *                              clamp(counts[i] + 1, 1, n_max) applied to its raw opacity and raw scales — new opacity
 *                              inverse_sigmoid(new_o), new scale log(max(|coeff · exp(s)|, 1e-10)).  One thread per row: a
 *                              source drawn several times is rewritten once, from its own opacity before the rewrite.
 *                              binoms: the (n_max, n_max) table of mcmc_binom_coefficients (:79-90), row-major
 *                              binoms[n·n_max + k] = C(n, k)·(-1)^k/√(k+1), built once by the host.
 * gsr_mcmc_relocation_params : relocation_params (:266-280, Eq. 9 of the paper) on explicit arrays: activated opacities
 *                              o[m] and ratio[m] (clamped to [1, n_max]) -> new_o[m], coeff[m].  The device function
 *                              gsr_mcmc_split_sampled applies, exposed for tests: the reference's fp32 expression, summed
 *                              `i` outer, `k` inner.
 * gsr_mcmc_relocate_rows     : the row copies of relocate_gaussians! (:153-172), in place, for up to
 *                              GSR_COMPOSE_MAX_GROUPS arrays of n rows in one launch.  The array is groups[g].dst
 *                              (groups[g].src must be NULL or equal to it): x[dead_idx[j]] = x[sampled_idx[j]], j < m; for
 *                              new_zero groups (the twelve Adam moment arrays) rows dead_idx[j] AND sampled_idx[j] become 0
 *                              (`touched = union(sampled, dead)`).  In place is safe because dead ∩ sampled = ∅ and
 *                              dead_idx holds no row twice; an index >= n is skipped.
 * gsr_mcmc_inject_noise      : _inject_noise! (:306-325): points += Δ, Δ = lr / (1 + exp(min(100·sigmoid(o) - 0.5, 80))) ·
 *                              R·diag(min(exp(2s), 1e8))·Rᵀ·ξ, rescaled to length max_kick where longer; ξ = three normals
 *                              keyed by (seed, row).  One pass, 44 B read + 12 B written per Gaussian.  rotations must be
 *                              16-byte aligned.
 * gsr_mcmc_regularization    : regularization_loss (:104-107): opacity_reg · mean(sigmoid(o)) + scale_reg · mean(exp(s))
 *                              into *loss_out (device; 0 for n = 0).  Unless NULL, the gradient w.r.t. the ACTIVATED
 *                              values — the constants opacity_reg / n and scale_reg / (n · scale_dims) — is ADDED onto
 *                              vopacities (1,N) and vscales (3,N), the arrays gsr_backward wrote (scale_dims = 1: row 0
 *                              only — the prologue pullback sums the three tiled rows), exactly as gsr_flatten_loss does:
 *                              gsr_prologue_backward / gsr_trainer_tail_step then yield the raw gradients.  The fused
 *                              gsr_backward_trainer_tail cannot take it: steps with a non-zero regulariser run
 *                              gsr_backward + gsr_mcmc_regularization + gsr_trainer_tail_step.  Fixed summation order, no
 *                              float atomics.  scratch: gsr_mcmc_regularization_scratch_bytes(n) bytes (may be NULL for
 *                              n = 0). */
GSR_API int gsr_mcmc_weights(int64_t n, int32_t scale_dims, const float* opacities_raw, const float* scales_raw,
                             float min_opacity, float log_max_scale, uint32_t* q, uint8_t* dead, void* stream);
GSR_API size_t gsr_mcmc_sample_scratch_bytes(int64_t n);
GSR_API int gsr_mcmc_sample(int64_t n, const uint32_t* q, int64_t m, uint32_t seed, uint32_t* sampled, int32_t* counts,
                            uint64_t* total, void* scratch, size_t scratch_bytes, void* stream);
GSR_API int gsr_mcmc_split_sampled(int64_t n, int32_t scale_dims, const int32_t* counts, const float* binoms, int32_t n_max,
                                   float min_opacity, float* opacities_raw, float* scales_raw, void* stream);
GSR_API int gsr_mcmc_relocation_params(int64_t m, const float* o, const int32_t* ratio, const float* binoms, int32_t n_max,
                                       float min_opacity, float* new_o, float* coeff, void* stream);
GSR_API int gsr_mcmc_relocate_rows(const gsr_compose_group* groups, int32_t n_groups, int64_t n, const uint32_t* dead_idx,
                                   const uint32_t* sampled_idx, int64_t m, void* stream);
GSR_API int gsr_mcmc_inject_noise(int64_t n, int32_t scale_dims, float* points, const float* opacities_raw,
                                  const float* scales_raw, const float* rotations, float lr, float max_kick, uint32_t seed,
                                  void* stream);
GSR_API size_t gsr_mcmc_regularization_scratch_bytes(int64_t n);
GSR_API int gsr_mcmc_regularization(int64_t n, int32_t scale_dims, const float* opacities_raw, const float* scales_raw,
                                    float opacity_reg, float scale_reg, float* loss_out, float* vopacities, float* vscales,
                                    void* scratch, size_t scratch_bytes, void* stream);

/* New: the SH-coefficient gradient of a batch of views from the factored
 * per-view colour cotangents written by gsr_backward (gsr_grads.vcolors):
 *   vshs[:, k, i] = Σ_v basis_k(normalize(means[:, i] - camera_centers[:, v])) * vcolors_all[:, i, v]
 * — ∇spherical_harmonics! (spherical_harmonics.jl:32-37) of every view, summed in ascending view
 * order.  camera_centers: device (3,V); vcolors_all: device (3,N,V) (view slowest), e.g. the output
 * of an all-gather over the ranks; vshs: device (3,K,N), fully overwritten (bands above
 * sh_degree get zeros).  With V = 1 the result is bit-identical to gsr_backward's own vshs. */
GSR_API int gsr_sh_grad_from_views(int32_t n, int32_t n_coeffs, int32_t sh_degree, int32_t n_views,
                                   const float* camera_centers, const float* means, const float* vcolors_all,
                                   float* vshs, void* stream);

/* New in ABI 4 (SURVEY.md §8f-1 for the multi-GPU step; training.jl:768-779): gsr_sh_grad_from_views with the trainer tail in
 * place of the ∇shs store.  After the factored exchange — the 11·N small gradients all-reduced, the per-view colour
 * cotangents all-gathered — ONE pass rebuilds Σ_v basis(dir_v) x vc_v per Gaussian, keeps it on chip, and applies the
 * pullback of the functor prologue + the six NU.Adam updates + the activated copies of the next forward.  Equivalent to
 *     gsr_sh_grad_from_views(n, K, deg, V, centers, st->theta[0], vcolors_all, vshs, stream);
 *     gsr_trainer_tail_step(n, K-1, st->scale_dims, {small..., vshs}, st->theta, st->mu, st->nu, ..., stream);
 * with bit-identical θ, μ, ν and activated copies, without the 3K·N-float ∇shs ever being written or read.
 *   small : vmeans, vopacities, vscales, vrotations of the all-reduced block (w.r.t. the ACTIVATED opacity / scale);
 *           small->vshs is not read (may be NULL)
 *   st    : as for gsr_backward_trainer_tail (theta[0] = the points the view directions are taken from; vmeans2d and
 *           forward_generation are not used). */
GSR_API int gsr_sh_grad_from_views_tail(int32_t n, int32_t n_coeffs, int32_t sh_degree, int32_t n_views,
                                        const float* camera_centers, const float* vcolors_all,
                                        const gsr_tail_grads* small, const gsr_tail_state* st, void* stream);

/* New (no reference counterpart): sum the per-view gradient arena over
 * the ranks of an RCCL communicator (ncclComm_t passed as void*).  librccl is resolved
 * lazily with dlopen, so single-GPU users need not have it. */
GSR_API int gsr_allreduce_grads(void* nccl_comm, float* arena, size_t count, void* stream);

/* New (measurement): STREAM triad a = b + q*c over `count` floats — the
 * device-to-device bandwidth bench.py measures in the same run as the hot path and reports
 * next to the 8 TB/s data-sheet peak (12 bytes of HBM traffic per element). */
GSR_API int gsr_stream_triad(float* a, const float* b, const float* c, size_t count, float q, void* stream);

/* New (measurement; the reference has no profiling hooks): per-stage kernel
 * timing with HIP events recorded on the caller's stream around each launch.  While
 * enabled, every gsr_forward / gsr_backward / gsr_loss_l1_ssim appends one event pair per
 * stage; gsr_profile_read() waits for them and returns, per stage, the summed
 * milliseconds and the number of launches (arrays of gsr_profile_stage_count() entries). */
/* `on` is a bit set: 1 = HIP-event stage timing (above), 2 = one roctx range "gsr:<stage>" per stage around its
 * launches (lets `rocprofv3 --marker-trace --kernel-trace` slice a trace by stage; the roctx library
 * is resolved lazily with dlopen; GSR_ROCTX=1 in the environment enables the ranges on every handle). */
GSR_API int gsr_profile_enable(gsr_handle* h, int on);
/* Restrict the event pairs to the stages whose bit is set (bit i = stage i of gsr_profile_stage_name; default all).
 * An event record is a marker packet between two kernels: eight pairs per step cost ≈ 0.06 ms of a 1.8 ms step on
 * MI355X, so a benchmark times its dominant stage alone inside the timed region and surveys the rest outside it. */
GSR_API int gsr_profile_stages(gsr_handle* h, uint32_t stage_mask);
GSR_API int gsr_profile_stage_count(void);
GSR_API const char* gsr_profile_stage_name(int stage);
GSR_API int gsr_profile_read(gsr_handle* h, double* ms_sum, int* launches, int reset);
/* Time from each recorded launch of `stage` to the next one (begin event to begin event), in milliseconds, oldest
 * first: with one launch of the stage per step these are the per-step times of a run, from the event pairs that are
 * on the stream anyway (a separate per-step marker would be one more bubble).  Writes min(count-1, max_n) values,
 * *n_out = count-1 (0 when fewer than two launches are recorded).  Does not reset. */
GSR_API int gsr_profile_read_intervals(gsr_handle* h, int stage, double* ms_out, int max_n, int* n_out);

GSR_API const char* gsr_last_error_string(void);
GSR_API const char* gsr_version(void);   /* "gsr-hip <release> abi <GSR_ABI_VERSION> (gfx950)" */
GSR_API int gsr_abi_version(void);        /* GSR_ABI_VERSION the library was built from */
/* Binding self-check, to be called once by every binding right after it loads the library (the Python mirror and the
 * Julia binding do): the caller's GSR_ABI_VERSION and its sizeof of the six structs that cross gsr_create / gsr_forward
 * / gsr_backward, and (ABI 6) of gsr_tail_state, which grew late in ABI 5.  Any mismatch — a caller built against another header — is GSR_E_INVALID_ARG with a message naming the
 * struct, instead of mis-sized structs being read silently. */
GSR_API int gsr_check_abi(int abi_version, size_t sizeof_config, size_t sizeof_inputs, size_t sizeof_camera,
                          size_t sizeof_aux, size_t sizeof_stats, size_t sizeof_grads, size_t sizeof_tail_state);

#ifdef __cplusplus
}
#endif

/* The library's policies as GPU-free functions (bins capacity, binning mode and form, the form tuner's rule, the held
 * fused launch, the backward's list split) and the view-history state gsr_stats reports from. */
#include "gsr_policy.h"

#endif /* GSR_H */
