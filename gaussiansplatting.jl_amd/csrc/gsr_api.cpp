// C ABI of libgsr_hip.so (include/gsr.h), the part with a handle: the handle object with its grow-only scratch, argument
// validation, and the launch choreography of gsr_forward, the backward entry points and the loss head (the entry points that
// take no handle are gsr_ops.cpp's).  Mirrors the host side of the reference's
// `GaussianRasterizer` / `rasterize` / `∇rasterize` (src/rasterization/rasterizer.jl:5-90,
// 255-408, 416-550) — everything is enqueued on the caller's stream; the only host sync is
// the instance-count read-back (rasterizer.jl:337).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <new>

#include "gsr_kernels.h"
#include "adam_math.h"
#include "gsr_host.h"
#include "gsr_devbuf.h"
#include "gsr_profiler.h"
#include "gsr_host_wait.h"
#include "gsr_sizes.h"

using namespace gsr_host;

thread_local char gsr_host::g_err[512] = "";

namespace {

// The form tuner's clock (the RULE is gsr_policy.cpp's: which views are timed, what decides, when it starts over): one event
// pair per timed view around the view's first kernel, read without blocking a later view.
struct TunerEvents {
    hipEvent_t ev[2 * GSR_TUNER_TIMED_VIEWS] = {};
    bool create() {
        for (auto& e : ev)
            if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; return false; }
        return true;
    }
    void destroy() { for (auto& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } }
    // all timed views complete?  -> their first kernels' milliseconds.  "Not ready" is the expected answer most of the time
    // and is consumed here; any OTHER error stays for the caller's next HIPCHK (an unconditional hipGetLastError
    // swallowed unrelated sticky errors).
    bool read(float ms[GSR_TUNER_TIMED_VIEWS]) {
        for (int v = 0; v < GSR_TUNER_TIMED_VIEWS; v++) {
            const hipError_t q = hipEventQuery(ev[2 * v + 1]);
            if (q == hipErrorNotReady) { (void)hipGetLastError(); return false; }
            if (q != hipSuccess || hipEventElapsedTime(&ms[v], ev[2 * v], ev[2 * v + 1]) != hipSuccess) return false;
        }
        return true;
    }
};

constexpr int kHandleBufs = 34;  // rows of kBufs, the table of the handle's buffers below the handle (checked there)

bool valid_mode(int m) { return m == GSR_MODE_RGB || m == GSR_MODE_RGBD || m == GSR_MODE_RGBDN; }

}  // namespace

struct gsr_handle {
    gsr_config cfg;
    int grid_x, grid_y, n_tiles;
    // ImageState (states.jl:99-111) + tile bookkeeping
    DevBuf ranges, n_contrib, final_T, tile_count, tile_start, tile_order, totals;
    // GeometryState (states.jl:2-47), repacked as one 64-byte record per Gaussian
    DevBuf geo, gnormal, radii, bsum, bpre, bvis;
    DevBuf comp;  // add_blur's compensations (float per Gaussian): GSR_FLAG_ANTIALIASED handles only, never allocated otherwise
    // BinningState (states.jl:66-85): unsorted keys (per-tile bins of bin_cap slots), sorted ids, sorted splat stream
    // everything gsr_forward carries from one view to the next lives in `pol`, and every decision taken from it is a pure
    // function of gsr_policy.cpp (include/gsr_policy.h): bins capacity / compact mode, the binning form and its tuner, the held
    // fused launch, the backward's list split.  This file only executes them.
    gsr_policy_config pcfg;
    gsr_policy_state pol;
    TunerEvents tuner_ev;
    int last_form = 0;              // binning form the last view's preprocess ran in (gsr_stats.preprocess_form)
    bool last_compact = false;
    bool tile_count_dirty = false;  // counters not yet re-zeroed by the tile sort
    double wait_ema_us = 0.0;       // running average of the host's wait for the instance count (wait_totals)
    DevBuf bins, keys_compact, big_list, values_sorted, s0, s1, s2, s3, big_scratch, long_state;
    DevBuf overflow_fill;           // fill cursors of the scatter pass restricted to the lists beyond the bins' capacity
    // backward: per-instance gradient rows + instance position map; gstate.∇means_2d
    DevBuf rows, vmean2d;
    DevBuf sh_jac;  // d rgb / d dir per Gaussian (9 floats): written by the row-independent job of composite_bwd's launch, read by pergauss_bwd
    DevBuf pose_part;  // pose gradient: 12 partial sums per workgroup of pergauss_bwd, added in a fixed order by its finishing launch
    // loss-head scratch
    DevBuf d0, d1, d2, partial;
    uint32_t* host_totals = nullptr;  // pinned: the scan's totals (GsrTotal), [GSR_TOTAL_SEQ] = the forward's sequence number
    uint32_t* host_totals_dev = nullptr;  // the same words as the device addresses them
    uint32_t totals_seq = 0;
    hipStream_t aux_stream = nullptr;  // the four-wave backward of those tiles runs here, next to the main launch
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool fwd_valid = false, bwd_valid = false;
    bool fwd_only = false;         // the last forward was GSR_FORWARD_ONLY: no stream / ids / row storage behind it
    bool inputs_consumed = false;  // gsr_backward_trainer_tail updated the forward's inputs in place
    bool dropped_by_reserve = false;  // the forward is not live because gsr_reserve / gsr_drop_forward ended it (for the messages)
    uint64_t generation = 0;             // ordinal of the last gsr_forward (gsr_stats.generation)
    int32_t* radii_cur = nullptr;        // gstate.radii of the last forward: caller's (gsr_aux.radii) or h->radii
    float2* vmean2d_cur = nullptr;       // gstate.∇means_2d of the last backward: caller's (gsr_grads.vmeans2d) or h->vmean2d
    int last_n = 0;
    int64_t last_D = 0;
    int64_t last_slots = 0;
    // the cotangent the handle's loss head wrote, and for which forward (GSR_GRADS_COLOR_COTANGENT is honoured for it only)
    const float* loss_vpixels = nullptr;
    uint64_t loss_generation = 0;
    uint32_t reserved_regrowths = 0;  // reallocations made by gsr_reserve (not counted in gsr_stats.scratch_regrowths)
    DevBuf dbg_flag;
    Profiler prof;

    DevBuf* all[kHandleBufs];  // the buffers of kBufs, in its order (gsr_create)
    int n_all = 0;
    GuardDamage guard_damage;  // GSR_DEBUG_GUARD: the first damaged guard of any buffer of `all`, freed ones included
};

// gsr_ssim_precision: 0 = the contracted build of ssim.hip (default), 1 = its bit-exact twin.  GSR_SSIM_EXACT=1 in the
// environment starts a process in exact mode (A/B runs of unmodified callers).
// Process-wide DEFAULT only: a handle created with gsr_config.ssim_precision = 0 / 1 is pinned (ABI 5).
std::atomic<int> gsr_host::g_ssim_exact{[] { const char* e = getenv("GSR_SSIM_EXACT"); return e && e[0] == '1' ? 1 : 0; }()};

namespace {

// Every DevBuf of the handle, once: its name (what GSR_DEBUG_GUARD's check reports), whether gsr_release_scene_buffers frees
// it, whether GSR_DEBUG_FILL may fill it (DevBuf::fill_ok: read only as float data), and its guard word (DevBuf::guard_word:
// 1, or 0 for ids whose range may be {0}).
struct BufRow {
    DevBuf gsr_handle::*buf;
    const char* name;
    bool scene, fill_ok;
    uint32_t guard_word;
};
#define BUF(member, scene, fill_ok, guard_word) {&gsr_handle::member, #member, scene, fill_ok, guard_word}
constexpr BufRow kBufs[] = {
    BUF(ranges, false, false, 1u),
    BUF(n_contrib, false, false, 1u),
    BUF(final_T, false, true, 1u),        // final transmittance per pixel: a factor of the backward, never a bound (n_contrib is)
    BUF(tile_count, false, false, 1u),
    BUF(tile_start, false, false, 1u),
    BUF(tile_order, false, false, 0u),    // tile ids
    BUF(totals, false, false, 1u),
    BUF(geo, true, false, 1u),
    BUF(gnormal, true, true, 1u),         // per-Gaussian normals (float4): feature values of the :rgbdn stream
    BUF(radii, true, false, 1u),
    BUF(bsum, true, false, 1u),
    BUF(bpre, true, false, 1u),
    BUF(bvis, true, false, 1u),
    BUF(bins, true, false, 1u),
    BUF(values_sorted, true, false, 0u),  // Gaussian ids
    BUF(s0, true, false, 1u),
    BUF(s1, true, false, 1u),
    BUF(s2, true, false, 1u),
    BUF(s3, true, false, 1u),
    BUF(big_scratch, true, false, 1u),
    BUF(rows, true, true, 1u),            // GsrInst gradient rows (float4): summed by pergauss_bwd, copied out by gsr_buffer
    BUF(vmean2d, true, true, 1u),         // gstate.∇means_2d (float2): written for every Gaussian, read by gsr_update_stats behind radii > 0
    BUF(d0, false, true, 1u),             // SSIM loss head's ∂map/∂µ1 plane
    BUF(d1, false, true, 1u),             // ... ∂map/∂σ1²
    BUF(d2, false, true, 1u),             // ... ∂map/∂σ12
    BUF(partial, false, true, 1u),        // per-wave (Σ|x-y|, Σssim) pairs summed by the loss finisher
    BUF(keys_compact, true, false, 1u),
    BUF(big_list, false, false, 0u),      // tile ids of the tier lists
    BUF(long_state, false, true, 1u),     // (T, A) float2 per pixel and segment of the long-list backward
    BUF(overflow_fill, false, false, 1u),
    BUF(dbg_flag, false, false, 1u),
    BUF(pose_part, true, true, 1u),       // per-workgroup pose-gradient partials: every slot is stored (zeros included) before it is summed
    BUF(comp, true, true, 1u),            // compensations of an antialiased forward (float): stale where radii == 0, read behind radii > 0
    BUF(sh_jac, true, true, 1u),          // the backward's SH direction Jacobians (9 floats): written and read behind radii > 0 in one gsr_backward
};
#undef BUF
template <class Pred> constexpr int count_bufs(Pred pred) {
    int n = 0;
    for (const BufRow& r : kBufs) n += pred(r) ? 1 : 0;
    return n;
}
static_assert(sizeof(kBufs) / sizeof(kBufs[0]) == kHandleBufs, "gsr_handle::all holds one pointer per row");
static_assert(count_bufs([](const BufRow& r) { return r.scene; }) == 19, "the scene buffers");
static_assert(count_bufs([](const BufRow& r) { return r.fill_ok; }) == 12, "the GSR_DEBUG_FILL candidates");
static_assert(count_bufs([](const BufRow& r) { return r.guard_word == 0u; }) == 3, "the id buffers whose guard word is 0");

bool antialiased(const gsr_handle* h) { return (h->cfg.flags & GSR_FLAG_ANTIALIASED) != 0u; }

GsrCam make_cam(const gsr_handle* h, const gsr_camera* c) {
    GsrCam k;
    for (int r = 0; r < 3; r++)
        for (int col = 0; col < 3; col++) k.R[r * 3 + col] = c->R[col * 3 + r];
    for (int i = 0; i < 3; i++) { k.t[i] = c->t[i]; k.center[i] = c->camera_center[i]; }
    for (int i = 0; i < 2; i++) { k.focal[i] = c->focal[i]; k.principal[i] = c->principal[i]; }
    k.width = h->cfg.width; k.height = h->cfg.height;
    k.grid_x = h->grid_x; k.grid_y = h->grid_y;
    k.near_plane = h->cfg.near_plane; k.far_plane = h->cfg.far_plane;
    k.radius_clip = h->cfg.radius_clip; k.blur_eps = h->cfg.blur_eps;
    k.exact_cull = (h->cfg.flags & GSR_FLAG_REFERENCE_TILE_LISTS) ? 0 : 1;
    k.R_dev = c->R_dev; k.t_dev = c->t_dev;
    return k;
}

// the compensations of an antialiased handle's forward, else NULL: WHAT the per-Gaussian kernels dispatch on
float* comp_of(const gsr_handle* h) { return antialiased(h) ? h->comp.as<float>() : nullptr; }
GsrGeom geom_of(const gsr_handle* h) {
    return GsrGeom{h->geo.as<GsrGeoRec>(), h->gnormal.as<float4>(), h->radii_cur, h->bsum.as<uint32_t>(),
                   h->bpre.as<uint32_t>()};
}
GsrStream stream_of(const gsr_handle* h) {
    return GsrStream{h->s0.as<float4>(), h->s1.as<float4>(), h->s2.as<float4>(), h->s3.as<float4>()};
}
GsrInst inst_of(const gsr_handle* h) { return GsrInst{h->rows.as<float4>()}; }
GsrTiles tiles_of(const gsr_handle* h) {
    return GsrTiles{h->tile_start.as<uint32_t>(), h->tile_count.as<uint32_t>(), h->tile_order.as<uint32_t>(),
                    h->ranges.as<uint32_t>(), h->big_list.as<uint32_t>(), h->totals.as<uint32_t>(), h->n_tiles, h->grid_x};
}
// the handle's fixed-capacity bins (cap == 0: preprocess only counts)
GsrKeys bins_of(const gsr_handle* h, uint32_t cap) { return GsrKeys{h->bins.as<uint64_t>(), cap, nullptr}; }
GsrFrame frame_of(const gsr_handle* h, const float* background, float* image, const gsr_aux* aux,
                  const gsr_scores* scores = nullptr) {
    return GsrFrame{background, image, h->n_contrib.as<uint32_t>(), h->final_T.as<float>(), h->values_sorted.as<uint32_t>(),
                    aux ? aux->covisibilities : nullptr, aux ? aux->uncertainties : nullptr,
                    scores ? GsrScores{scores->max_weight, (unsigned long long*)scores->hits, (unsigned long long*)scores->weight_sum}
                           : GsrScores{nullptr, nullptr, nullptr}};
}

// gsr_preprocess_form: -1 by scene and grid size (default), 0 direct, 1 aggregating wherever its LDS fits; the same rule as
// gsr_ssim_precision's (g_ssim_exact, above): the process-wide default of the handles that do not say
std::atomic<int> g_preprocess_form{[] { const char* e = getenv("GSR_PREPROCESS_AGG"); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }()};
inline int ssim_exact_of(const gsr_handle* h) {
    return h->cfg.ssim_precision != GSR_DEFAULT ? (h->cfg.ssim_precision == GSR_SSIM_EXACT ? 1 : 0)
                                                : g_ssim_exact.load(std::memory_order_relaxed);
}
inline int preprocess_form_of(const gsr_handle* h) {  // -1 by scene and grid, 0 direct, 1 aggregating
    return h->cfg.preprocess_form != GSR_DEFAULT ? (h->cfg.preprocess_form == GSR_PREPROCESS_AGGREGATING ? 1 : 0)
                                                 : g_preprocess_form.load(std::memory_order_relaxed);
}

// Byte sizes of the buffers an n-Gaussian view on this handle touches (gsr_sizes.h: the one place they are written)
gsr_gaussian_bytes gaussian_bytes(const gsr_handle* h, int64_t n) {
    return gsr_sizes_per_gaussian((size_t)n, h->cfg.mode, gsr_pose_partial_floats(n), antialiased(h));
}

// gsr_stats' view-history block (ABI 6): the policy state's counters + the mechanism's own (buffer reallocations)
void fill_history(const gsr_handle* h, gsr_stats* st) {
    const gsr_policy_state& p = h->pol;
    st->bins_regrowths = p.bins_regrowths;
    st->compact_fallbacks = p.compact_fallbacks;
    st->tuner_rearms = p.tuner_rearms;
    uint32_t grows = 0;
    for (int i = 0; i < h->n_all; i++) grows += h->all[i]->regrowths;
    st->scratch_regrowths = grows - h->reserved_regrowths;  // (inside a view: what gsr_reserve reallocated is not counted)
    st->fused_relaunches = p.fused_relaunches;
    st->held_views = p.held_views;
    const bool decided = p.tuner.phase == GSR_TUNER_TIMED_VIEWS + 1;
    st->tuner_form = decided ? p.tuner.form : -1;
    st->tuner_ms[0] = decided ? p.tuner.ms[0] : 0.0f;
    st->tuner_ms[1] = decided ? p.tuner.ms[1] : 0.0f;
}

// GSR_GRADS_COLOR_COTANGENT (gsr.h): honoured for the cotangent this handle's loss head wrote for THIS forward, nothing else.
// GSR_CHECK_COLOR_COTANGENT=1 (debugging): also look at the buffer — every value of channels >= 3 must be exactly zero.
__global__ void nonzero_tail_kernel(const float* __restrict__ v, size_t n_pixels, int C, uint32_t* flag) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    bool bad = false;
    for (int c = 3; c < C; c++) bad |= v[p * C + c] != 0.0f;
    if (bad) atomicOr(flag, 1u);
}
int check_color_cotangent(gsr_handle* h, const float* vpixels, hipStream_t s) {
    if (h->cfg.mode <= 3) return GSR_OK;  // nothing above the colour channels
    if (vpixels != h->loss_vpixels || h->loss_generation != h->generation)
        return fail(GSR_E_INVALID_ARG, "GSR_GRADS_COLOR_COTANGENT is only valid for the cotangent gsr_loss_l1_ssim wrote for this "
                    "forward on this handle (its vpixels %p for forward #%llu; got %p for forward #%llu): a cotangent with depth / "
                    "alpha / normal terms must not set the flag", (const void*)h->loss_vpixels,
                    (unsigned long long)h->loss_generation, (const void*)vpixels, (unsigned long long)h->generation);
    const char* look = getenv("GSR_CHECK_COLOR_COTANGENT");  // (read per call: a debugging switch, flipped by tests in-process)
    if (!(look && look[0] == '1')) return GSR_OK;
    int rc = h->dbg_flag.ensure(4);
    if (rc) return rc;
    const size_t P = (size_t)h->cfg.width * h->cfg.height;
    uint32_t bad = 0;
    HIPCHK(hipMemsetAsync(h->dbg_flag.p, 0, 4, s));
    hipLaunchKernelGGL(nonzero_tail_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, vpixels, P, h->cfg.mode,
                       h->dbg_flag.as<uint32_t>());
    HIPCHK(hipMemcpyAsync(&bad, h->dbg_flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad) return fail(GSR_E_INVALID_ARG, "GSR_GRADS_COLOR_COTANGENT: vpixels holds non-zero values above the colour channels "
                         "(something was added to the loss head's cotangent in place)");
    return GSR_OK;
}

int check_inputs(const gsr_handle* h, const gsr_inputs* in, const gsr_camera* cam) {
    if (!h || !in || !cam) return fail(GSR_E_INVALID_ARG, "null handle / inputs / camera");
    if (in->n < 0) return fail(GSR_E_INVALID_ARG, "n = %d < 0", in->n);
    if (in->sh_degree < 0 || in->sh_degree > 3) return fail(GSR_E_INVALID_ARG, "sh_degree = %d not in 0..3", in->sh_degree);
    if (in->n_coeffs < (in->sh_degree + 1) * (in->sh_degree + 1) || in->n_coeffs > 16)
        return fail(GSR_E_INVALID_ARG, "n_coeffs = %d does not hold degree %d", in->n_coeffs, in->sh_degree);
    if (in->n > 0 && (!in->means || !in->shs || !in->opacities || !in->scales || !in->rotations))
        return fail(GSR_E_INVALID_ARG, "null input array");
    if (((uintptr_t)in->rotations & 15) != 0) return fail(GSR_E_INVALID_ARG, "rotations must be 16-byte aligned");
    if ((cam->R_dev == nullptr) != (cam->t_dev == nullptr))
        return fail(GSR_E_INVALID_ARG, "R_dev and t_dev must be given together");
    return GSR_OK;
}

}  // namespace

extern "C" {

const char* gsr_last_error_string(void) { return g_err; }
#define GSR_STR2(x) #x
#define GSR_STR(x) GSR_STR2(x)
const char* gsr_version(void) { return "gsr-hip 0.4 abi " GSR_STR(GSR_ABI_VERSION) " (gfx950)"; }
int gsr_abi_version(void) { return GSR_ABI_VERSION; }

int gsr_host_wait_policy(int spin_us, int yield_us, int sleep_us) {
    if (spin_us < 0 || yield_us < 0 || sleep_us < 0) return fail(GSR_E_INVALID_ARG, "negative wait time");
    if (spin_us > kWaitMaxUs || yield_us > kWaitMaxUs || sleep_us > kWaitMaxUs)
        return fail(GSR_E_INVALID_ARG, "wait times are at most %d us", kWaitMaxUs);
    WaitPolicy w;
    w.spin_us = spin_us; w.yield_us = yield_us; w.sleep_us = sleep_us;
    g_wait_packed.store(pack_wait(w), std::memory_order_relaxed);
    return GSR_OK;
}

int gsr_ssim_precision(int exact) {
    if (exact != 0 && exact != 1) return fail(GSR_E_INVALID_ARG, "gsr_ssim_precision: 0 (fast) or 1 (exact)");
    g_ssim_exact.store(exact, std::memory_order_relaxed);
    return GSR_OK;
}
int gsr_get_ssim_precision(void) { return g_ssim_exact.load(std::memory_order_relaxed); }

int gsr_preprocess_form(int form) {
    if (form < -1 || form > 1) return fail(GSR_E_INVALID_ARG, "gsr_preprocess_form: -1 (by size), 0 (direct) or 1 (aggregating)");
    g_preprocess_form.store(form, std::memory_order_relaxed);
    return GSR_OK;
}
int gsr_get_preprocess_form(void) { return g_preprocess_form.load(std::memory_order_relaxed); }

int gsr_check_abi(int abi_version, size_t sizeof_config, size_t sizeof_inputs, size_t sizeof_camera, size_t sizeof_aux,
                  size_t sizeof_stats, size_t sizeof_grads, size_t sizeof_tail_state) {
    if (abi_version != GSR_ABI_VERSION)
        return fail(GSR_E_INVALID_ARG, "binding was written for gsr ABI %d, this library is ABI %d", abi_version, GSR_ABI_VERSION);
    const struct { const char* name; size_t theirs, ours; } t[] = {
        {"gsr_config", sizeof_config, sizeof(gsr_config)}, {"gsr_inputs", sizeof_inputs, sizeof(gsr_inputs)},
        {"gsr_camera", sizeof_camera, sizeof(gsr_camera)}, {"gsr_aux", sizeof_aux, sizeof(gsr_aux)},
        {"gsr_stats", sizeof_stats, sizeof(gsr_stats)},    {"gsr_grads", sizeof_grads, sizeof(gsr_grads)},
        {"gsr_tail_state", sizeof_tail_state, sizeof(gsr_tail_state)}};
    for (const auto& e : t)
        if (e.theirs != e.ours)
            return fail(GSR_E_INVALID_ARG, "sizeof(%s) is %zu in the binding, %zu in the library", e.name, e.theirs, e.ours);
    return GSR_OK;
}

int gsr_create(const gsr_config* cfg, gsr_handle** out) {
    if (!cfg || !out) return fail(GSR_E_INVALID_ARG, "null config / out");
    if (cfg->width <= 0 || cfg->height <= 0) return fail(GSR_E_INVALID_ARG, "bad resolution %dx%d", cfg->width, cfg->height);
    if (!valid_mode(cfg->mode)) return fail(GSR_E_INVALID_ARG, "Invalid render mode: %d (3=rgb, 5=rgbd, 8=rgbdn)", cfg->mode);
    if (!(cfg->near_plane < cfg->far_plane)) return fail(GSR_E_INVALID_ARG, "near_plane >= far_plane");
    if (cfg->flags & GSR_FLAG_RETIRED_BIT0)
        return fail(GSR_E_INVALID_ARG, "flag bit 0x1 is retired (ABI 1's GSR_FLAG_EXACT_TILE_CULL): rebuild the caller against "
                                       "include/gsr.h ABI %d", GSR_ABI_VERSION);
    if (cfg->flags & ~(uint32_t)(GSR_FLAG_REFERENCE_TILE_LISTS | GSR_FLAG_ANTIALIASED)) return fail(GSR_E_INVALID_ARG, "unknown flags 0x%x", cfg->flags);
    if (cfg->ssim_precision < 0 || cfg->ssim_precision > GSR_SSIM_EXACT)
        return fail(GSR_E_INVALID_ARG, "gsr_config.ssim_precision = %d: GSR_DEFAULT (0), GSR_SSIM_FAST (1) or GSR_SSIM_EXACT (2)",
                    cfg->ssim_precision);
    if (cfg->preprocess_form < 0 || cfg->preprocess_form > GSR_PREPROCESS_AGGREGATING)
        return fail(GSR_E_INVALID_ARG, "gsr_config.preprocess_form = %d: GSR_DEFAULT (0), GSR_PREPROCESS_DIRECT (1) or "
                    "GSR_PREPROCESS_AGGREGATING (2)", cfg->preprocess_form);
    if (cfg->form_tuner < 0 || cfg->form_tuner > GSR_TUNER_ON)
        return fail(GSR_E_INVALID_ARG, "gsr_config.form_tuner = %d: GSR_DEFAULT (0), GSR_TUNER_OFF (1) or GSR_TUNER_ON (2)", cfg->form_tuner);
    if (cfg->grad_precision < 0 || cfg->grad_precision > GSR_GRAD_ACCURATE)
        return fail(GSR_E_INVALID_ARG, "gsr_config.grad_precision = %d: GSR_DEFAULT (0), GSR_GRAD_FP32_REFERENCE (1) or GSR_GRAD_ACCURATE (2)",
                    cfg->grad_precision);
    gsr_handle* h = new (std::nothrow) gsr_handle();
    if (!h) return fail(GSR_E_OOM, "host allocation failed");
    h->cfg = *cfg;
    h->grid_x = (cfg->width + GSR_TILE - 1) / GSR_TILE;
    h->grid_y = (cfg->height + GSR_TILE - 1) / GSR_TILE;
    // (8 192 tiles = 131 072 pixels wide: one row of the tile grid must fit the aggregating binning's LDS band, preprocess.hip)
    if (h->grid_x > 8192 || h->grid_y > 65535) { delete h; return fail(GSR_E_INVALID_ARG, "resolution too large"); }
    h->n_tiles = h->grid_x * h->grid_y;
    // the handle's policies: configuration (constructor fields, then the tuner's process default) and the view-history state
    gsr_policy_config_init(&h->pcfg, cfg->width, cfg->height, cfg->bins_budget_bytes, -1 /* resolved per view: process default */);
    gsr_policy_state_init(&h->pol);
    const char* tun = getenv("GSR_FORM_TUNER");  // the DEFAULT of handles that do not say (0 = off)
    h->pcfg.form_tuner = cfg->form_tuner == GSR_TUNER_ON ? 1 : cfg->form_tuner == GSR_TUNER_OFF ? 0 : !(tun && tun[0] == '0');
    for (const BufRow& r : kBufs) {
        DevBuf& b = h->*r.buf;
        b.name = r.name;
        b.fill_ok = r.fill_ok;
        b.guard_word = r.guard_word;
        b.damage = &h->guard_damage;
        h->all[h->n_all++] = &b;
    }
    const size_t P = (size_t)cfg->width * cfg->height, T = (size_t)h->n_tiles;
    int rc = GSR_OK;
    if ((rc = h->ranges.ensure(2 * T * 4)) || (rc = h->n_contrib.ensure(P * 4)) || (rc = h->final_T.ensure(P * 4)) ||
        (rc = h->tile_count.ensure((T + 2) * 4)) || (rc = h->tile_start.ensure((T + 1) * 4)) ||
        (rc = h->tile_order.ensure((T + 8) * 4)) || (rc = h->totals.ensure(GSR_TOTAL_WORDS * 4)) || (rc = h->big_list.ensure((3 * T + 1) * 4))) {
        gsr_destroy(h);
        return rc;
    }
    hipError_t e = hipHostMalloc((void**)&h->host_totals, GSR_TOTAL_WORDS * sizeof(uint32_t), hipHostMallocDefault);  // fine-grained
    if (e == hipSuccess) {
        memset(h->host_totals, 0, GSR_TOTAL_WORDS * sizeof(uint32_t));
        e = hipHostGetDevicePointer((void**)&h->host_totals_dev, h->host_totals, 0);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming);
    if (e != hipSuccess) {
        gsr_destroy(h);
        return fail(GSR_E_HIP, "pinned memory / stream / event creation failed: %s", hipGetErrorString(e));
    }
    (void)hipMemset(h->totals.p, 0, GSR_TOTAL_WORDS * 4);  // [GSR_TOTAL_SEQ]: the scan's ticket word
    (void)hipMemset(h->ranges.p, 0, 2 * T * 4);
    (void)hipMemset(h->tile_count.p, 0, (T + 2) * 4);
    *out = h;
    return GSR_OK;
}

int gsr_destroy(gsr_handle* h) {
    if (!h) return GSR_OK;
    for (int i = 0; i < h->n_all; i++) h->all[i]->release();
    if (h->host_totals) (void)hipHostFree(h->host_totals);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->aux_stream) (void)hipStreamDestroy(h->aux_stream);
    h->tuner_ev.destroy();
    h->prof.destroy();
    delete h;
    return GSR_OK;
}

// The handle after its last forward stopped being live (its buffers were released or reallocated, or the caller's state arrays
// were): no backward, no statistics, and the per-forward buffers of gsr_buffer report 0 bytes — nothing below reads what the
// forward left.  The policy state, the bins and the loss head's buffers are not part of it.
static void end_live_forward(gsr_handle* h) {
    h->fwd_valid = false;
    h->bwd_valid = false;
    h->radii_cur = nullptr;
    h->vmean2d_cur = nullptr;
    h->last_n = 0;
    h->last_D = 0;
    h->last_slots = 0;
}

int gsr_release_scene_buffers(gsr_handle* h) {
    if (!h) return fail(GSR_E_INVALID_ARG, "null handle");
    h->pol.bin_cap = 0;
    h->pol.compact_sticky = 0;
    for (const BufRow& r : kBufs) {
        if (!r.scene) continue;
        int rc = (h->*r.buf).release();
        if (rc) return rc;
    }
    end_live_forward(h);
    h->dropped_by_reserve = false;
    return GSR_OK;
}

int gsr_drop_forward(gsr_handle* h) {
    if (!h) return fail(GSR_E_INVALID_ARG, "null handle");
    h->dropped_by_reserve = h->dropped_by_reserve || h->fwd_valid;
    end_live_forward(h);
    return GSR_OK;
}

int gsr_reserve(gsr_handle* h, int64_t n_gaussians, int64_t n_instances) {
    if (!h) return fail(GSR_E_INVALID_ARG, "null handle");
    if (n_gaussians < 0 || n_instances < 0 || n_gaussians > 0x7FFFFFFFll || n_instances > 0xFFFFFFFFll)
        return fail(GSR_E_INVALID_ARG, "gsr_reserve: sizes out of range");
    const int C = h->cfg.mode;
    int rc = GSR_OK;
    struct Uncount {  // reallocations made here are the caller's choice of WHEN, not a forward's surprise: keep them out of the history
        gsr_handle* h;
        uint32_t before = 0;
        uint32_t sum() const { uint32_t g = 0; for (int i = 0; i < h->n_all; i++) g += h->all[i]->regrowths; return g; }
        explicit Uncount(gsr_handle* h_) : h(h_) { before = sum(); }
        // ... and a buffer that existed was freed (on the error paths too): whatever the last forward left in it is gone, and
        // so may be what radii_cur / vmean2d_cur point at.  The forward is no longer live: the backward entry points,
        // gsr_update_stats and gsr_copy_buffer fail with GSR_E_STATE until the next gsr_forward instead of reading fresh
        // allocations.  A call that reallocated nothing (sizes within capacity, first allocations) leaves the forward as it is.
        ~Uncount() {
            const uint32_t grown = sum() - before;
            h->reserved_regrowths += grown;
            if (grown > 0) {
                h->dropped_by_reserve = h->dropped_by_reserve || h->fwd_valid;
                end_live_forward(h);
            }
        }
    } uncount(h);
    if (n_gaussians > 0) {
        const gsr_gaussian_bytes b = gaussian_bytes(h, n_gaussians);
        if ((rc = h->geo.ensure(b.geo)) || (rc = h->radii.ensure(b.radii)) || (rc = h->bsum.ensure(b.block)) ||
            (rc = h->bpre.ensure(b.block)) || (rc = h->bvis.ensure(b.block)) || (rc = h->vmean2d.ensure(b.vmean2d)) ||
            (rc = h->pose_part.ensure(b.pose_part)) || (C > 5 && (rc = h->gnormal.ensure(b.gnormal))) ||
            (b.comp && (rc = h->comp.ensure(b.comp))))
            return rc;
    }
    if (n_instances > 0) {
        // (the gradient rows are indexed by Gaussian-major SLOT: one per emitted tile of a small rect, one per tile of a large one —
        //  at most ~1.5 x the instance count under exact culling: gsr_sizes_reserve_instances)
        const gsr_instance_bytes b = gsr_sizes_reserve_instances((uint64_t)n_instances, C);
        if ((rc = h->values_sorted.ensure(b.values_sorted)) || (rc = h->s0.ensure(b.stream)) || (rc = h->s1.ensure(b.stream)) ||
            (rc = h->s2.ensure(b.stream)) || (C > 3 && (rc = h->s3.ensure(b.s3))) || (rc = h->rows.ensure(b.rows)))
            return rc;
    }
    return GSR_OK;
}

int gsr_debug_check_guards(gsr_handle* h) {
    if (!h) return fail(GSR_E_INVALID_ARG, "null handle");
    for (int i = 0; i < h->n_all; i++)
        if (int rc = h->all[i]->check_guard()) return rc;
    const GuardDamage& d = h->guard_damage;
    if (d.set)
        return fail(GSR_E_STATE, "guard behind handle buffer '%s' is damaged: byte offset %zu past its capacity holds the word "
                                 "0x%08x (guard word 0x%08x)", d.name, d.offset, d.word, d.expect);
    return GSR_OK;
}

int64_t gsr_memory_usage(const gsr_handle* h) {
    if (!h) return 0;
    int64_t s = 0;
    for (int i = 0; i < h->n_all; i++) s += (int64_t)h->all[i]->cap;
    return s;
}

// What the stages of one gsr_forward share (the stages below, in the order gsr_forward lists them).
struct FwdView {
    hipStream_t s;
    int C, n;
    const gsr_inputs* in; float* image_out; const gsr_aux* aux; gsr_stats* stats;  // the caller's
    const gsr_scores* scores;  // gsr_forward_scored's, or NULL
    bool fwd_only;
    GsrCam k;
    gsr_view_plan plan;
    gsr_view_outcome oc;
    uint64_t cap_instances;  // what the per-instance buffers held when the view began
    bool spec;               // launches may go out behind the scan, before the host has the counts
    uint32_t seq;
    uint64_t D, D_slots;     // the scan's totals, read back: D_slots >= D; == D unless exact culling dropped tiles
    uint32_t max_tile, n_big, n_mid4, n_mid8, visible;  // visible: with the any-rect flag in bit 31
    size_t slab_stride;      // keys per merge slab of a list beyond the LDS sort (0: none)
};

// Argument checks and per-Gaussian scratch; a call that gets through them is the handle's forward number `generation`.
static int fwd_begin(gsr_handle* h, const gsr_inputs* in, const gsr_camera* cam, float* image_out, const gsr_aux* aux,
                     const gsr_scores* scores, void* stream_v, gsr_stats* stats, FwdView& v) {
    // (the scores' own checks first: they need no handle)
    if (scores && (scores->flags || scores->reserved))
        return fail(GSR_E_INVALID_ARG, "unknown gsr_scores.flags 0x%x / reserved 0x%x", scores->flags, scores->reserved);
    if (scores && ((uintptr_t)scores->max_weight % 4 || (uintptr_t)scores->hits % 8 || (uintptr_t)scores->weight_sum % 8))
        return fail(GSR_E_INVALID_ARG, "gsr_scores: max_weight must be 4-byte, hits and weight_sum 8-byte aligned");
    int rc = check_inputs(h, in, cam);
    if (rc) return rc;
    if (!image_out) return fail(GSR_E_INVALID_ARG, "null image_out");
    if (aux && ((aux->flags & ~(uint32_t)GSR_FORWARD_ONLY) || aux->reserved))
        return fail(GSR_E_INVALID_ARG, "unknown gsr_aux.flags 0x%x / reserved 0x%x", aux->flags, aux->reserved);
    // (no array asked for: the unscored kernels, as with scores == NULL)
    if (scores && !scores->max_weight && !scores->hits && !scores->weight_sum) scores = nullptr;
    v.in = in; v.image_out = image_out; v.aux = aux; v.stats = stats; v.scores = scores;
    v.fwd_only = aux && (aux->flags & GSR_FORWARD_ONLY);
    v.s = (hipStream_t)stream_v;
    v.C = h->cfg.mode; v.n = in->n;
    h->fwd_valid = false;
    h->bwd_valid = false;
    h->inputs_consumed = false;
    h->dropped_by_reserve = false;
    h->fwd_only = v.fwd_only;

    const gsr_gaussian_bytes b = gaussian_bytes(h, v.n);
    const bool own_radii = !(aux && aux->radii);
    // per-Gaussian scratch: grow-only with 25 % slack, like the per-instance buffers below — a training run's densification
    // adds 5-15 % of Gaussians per round (strategy.jl:78-105), and an exact fit made EVERY round's first view reallocate all
    // five (five hipFree + hipMalloc = device synchronisations: the slowest plain steps of the round-6 training protocol)
    const float nslack = 1.25f;
    if ((rc = h->geo.ensure(b.geo, nslack)) || (own_radii && (rc = h->radii.ensure(b.radii, nslack))) ||
        (rc = h->bsum.ensure(b.block, nslack)) || (rc = h->bpre.ensure(b.block, nslack)) ||
        (rc = h->bvis.ensure(b.block, nslack)) || (v.C > 5 && (rc = h->gnormal.ensure(b.gnormal, nslack))) ||
        (b.comp && (rc = h->comp.ensure(b.comp, nslack))))
        return rc;
    h->radii_cur = own_radii ? h->radii.as<int32_t>() : aux->radii;
    h->vmean2d_cur = nullptr;
    h->generation++;
    if (stats) stats->generation = h->generation;
    v.k = make_cam(h, cam);
    return GSR_OK;
}

// Sort + forward of every tile of up to 1024 instances, as ONE launch on stream fs.
static void launch_fused(gsr_handle* h, const FwdView& v, hipStream_t fs) {
    StageScope sc3(h->prof, ST_SORT_COMPOSITE_FWD, fs);
    gsr_launch_sort_composite_fwd(fs, v.C, v.k, tiles_of(h), bins_of(h, v.plan.bin_cap_view), geom_of(h), stream_of(h),
                                  frame_of(h, v.in->background, v.image_out, v.aux, v.scores), (uint32_t)v.cap_instances,
                                  /*keep_backward_state=*/!v.fwd_only);
    sc3.close();
}

// Plan and bin: the view's plan, preprocess, the scan, and what goes out behind the scan without waiting for the host.
static int fwd_plan_and_bin(gsr_handle* h, FwdView& v) {
    int rc;
    const hipStream_t s = v.s;
    const size_t T = (size_t)h->n_tiles;
    // Binning (SURVEY.md A.5-A.7 restated per tile).  FAST mode: every tile owns a fixed-capacity key bin and preprocess drops
    // the keys straight into them — no second pass over the instances; (T+1) x capacity x 8 B, so only while that stays within
    // the bins budget.  Otherwise — a scene with a few very deep tiles, or a view that overflowed small bins — the COMPACT mode
    // runs: preprocess only counts, the scan turns the counts into offsets, a scatter pass puts the keys at exact offsets (8 B
    // per instance whatever the skew).  WHICH of them, with what capacity, in which binning form: gsr_policy_begin_view.
    h->pcfg.preprocess_form = preprocess_form_of(h);  // the handle's pin, else the process default as of this call
    float timed_ms[GSR_TUNER_TIMED_VIEWS];
    const bool have_ms = h->pcfg.form_tuner && h->pol.tuner.phase == GSR_TUNER_TIMED_VIEWS && h->tuner_ev.read(timed_ms);
    gsr_policy_begin_view(&h->pcfg, &h->pol, v.n, have_ms ? timed_ms : nullptr, &v.plan);
    const uint32_t bin_cap_view = v.plan.bin_cap_view;
    const bool use_bins = bin_cap_view > 0;
    if (use_bins && (rc = h->bins.ensure((T + 1) * (size_t)bin_cap_view * 8))) return rc;
    // The tile counters are zero on entry: gsr_create clears them and the tile sort re-zeroes each
    // tile's counter as it consumes it (no memset kernel per view; the scan overwrites every total).
    // Only a pass that did not reach the sort (an error) leaves them dirty.
    if (h->tile_count_dirty) HIPCHK(hipMemsetAsync(h->tile_count.p, 0, (T + 2) * 4, s));
    h->tile_count_dirty = true;
    int timed = v.plan.timed_slot;
    if (timed >= 0 && !h->tuner_ev.create()) {  // no clock, no tuner on this handle (the plan's form is still a valid form)
        h->pcfg.form_tuner = 0;
        h->pol.tuner.phase = 0;
        timed = -1;
    }
    StageScope sc1(h->prof, ST_PREPROCESS, s);
    if (timed >= 0) HIPCHK(hipEventRecord(h->tuner_ev.ev[2 * timed], s));
    h->last_form = gsr_launch_preprocess(s, v.n, v.in->n_coeffs, v.in->sh_degree, v.C, v.in->means, v.in->scales,
                                         v.in->rotations, v.in->opacities, v.in->shs, v.k, geom_of(h), tiles_of(h),
                                         h->bvis.as<uint32_t>(), bins_of(h, bin_cap_view) /* 0: count only */,
                                         /*aggregating=*/v.plan.form != GSR_FORM_DIRECT, comp_of(h));
    if (timed >= 0) HIPCHK(hipEventRecord(h->tuner_ev.ev[2 * timed + 1], s));
    sc1.close();
    v.seq = ++h->totals_seq ? h->totals_seq : ++h->totals_seq;  // never 0
    StageScope sc2(h->prof, ST_SCAN, s);
    gsr_launch_tile_scan(s, tiles_of(h), geom_of(h), (v.n + 255) / 256, h->bvis.as<uint32_t>(), h->host_totals_dev, v.seq);
    sc2.close();
    HIPCHK(hipGetLastError());
    // the one host sync of the path: instance count D (reference: rasterizer.jl:337).  tile_scan stores the totals
    // and then this forward's sequence number into pinned host memory; no copy packet, no event on the stream.
    // Sort + forward of every tile of up to 1024 instances (nearly all of them) go out BEHIND the scan, as ONE launch,
    // without waiting for the host: the buffers have a capacity from earlier views (grow-only, 25 % slack), and the
    // kernel itself checks the scan's totals against it.  The host's wait (fwd_read_back) then overlaps that launch instead of
    // idling the GPU, and inside it the HBM-bound sort of one tile shares the CU with the VALU-bound compositing of others.
    uint64_t cap_instances = std::min(std::min(h->values_sorted.cap / 4, h->s0.cap / 16), std::min(h->s1.cap / 16, h->s2.cap / 16));
    if (v.C > 3) cap_instances = std::min<uint64_t>(cap_instances, h->s3.cap / 16);
    cap_instances = std::min<uint64_t>(cap_instances, 0xFFFFFFFFull);
    if (v.fwd_only) cap_instances = 0xFFFFFFFFull;  // nothing is stored per instance: no capacity to respect
    v.cap_instances = cap_instances;
    v.spec = use_bins && cap_instances > 0;
    // TIER TILES (lists beyond the fused launch's 1024 instances) are walked by their own launch, four single-wave workgroups per
    // tile, and that walk is a latency chain: 0.4 ms for one 32 k-instance tile and its neighbours, 0.15 ms for the few hundred
    // tiles of 1-4 k instances of a trained-like scene — it belongs BESIDE the fused launch, not behind it.  What does not work,
    // measured (tools/cu_mask_probe.hip, profiles/r05/experiments/long_list_chain.txt): queueing sorts + walk on a second stream
    // while the fused launch runs — it fills every wave slot and all LDS, and the sorts' workgroups (512-1024 threads, 64 KB)
    // never find four of its workgroups retiring on one CU together: the chain starts at the fused launch's tail, on any
    // stream, at any priority; CU-masked streams do give the chain CUs of its own (probe: done after 2.7 of 7.9 ms instead of
    // 9.0 of 9.0), but hipExtStreamCreateWithCUMask only makes streams that synchronise with the NULL stream — torch's default
    // — and every launch of the step then pays ~10 us of implicit cross-queue wait (+0.16 ms per step: more than it saved).
    // What does: the walk's workgroups are single waves, which slip into any retiring slot.  So when the previous view had tier
    // tiles the fused launch is HELD until the host has the counts and the tier sorts have run (mostly idle GPU: 0.04-0.2 ms),
    // and then goes out together with the walk, which takes the handle's second stream at raised wave priority.  Hot tile
    // (32 k) 2.08 -> 1.80 ms, trained-like 3 M / 1440p 2.19 -> 2.10, dense 4K 7.81 -> 7.70; a view without tier tiles is not
    // touched.  (gsr_policy_config.beside_max_tiles: hold only when the previous view had at most that many tier tiles; 0 = never.)
    const bool hold_fused = v.spec && v.plan.hold_fused;
    if (v.spec && !hold_fused) launch_fused(h, v, s);
    // A held fused launch waits for the tier sorts, and those for the host's read-back: 22-34 us of idle GPU per view (kernel
    // trace of the training protocol, profiles/r06/experiments/training_step_idle_time.txt).  The two mid tiers' sorts therefore
    // go out NOW, behind the scan, with grids guessed from the previous view and the scan's totals checked on the device
    // (gsr_launch_tile_sort_mid); what the guess missed — and every list beyond 8192, whose chain needs host-sized scratch — is
    // sorted after the read-back.  Not for forward-only renders (whose stream buffers are not sized by cap_instances).
    // (the guesses are the policy's: gsr_view_plan.spec_mid4 / spec_mid8; what is not launched is zeroed for gsr_policy_end_view)
    if (!(hold_fused && !v.fwd_only)) v.plan.spec_mid4 = v.plan.spec_mid8 = 0u;
    if (v.plan.spec_mid4 | v.plan.spec_mid8) {
        StageScope scs(h->prof, ST_SORT, s, /*extra=*/true);  // (the stage's time; the call after the read-back counts the launch)
        gsr_launch_tile_sort_mid(s, v.C, tiles_of(h), bins_of(h, bin_cap_view), v.plan.spec_mid4, v.plan.spec_mid8, geom_of(h),
                                 stream_of(h), h->values_sorted.as<uint32_t>(), (uint32_t)cap_instances);
        scs.close();
    }
    return GSR_OK;
}

// gsr_stats of the view, once the scan's counts and the policy's outcome are known
static void fill_view_stats(const gsr_handle* h, const FwdView& v, gsr_stats* st) {
    const bool hybrid = v.oc.binning == GSR_BINNING_OVERFLOW, compact = v.oc.binning == GSR_BINNING_COMPACT;
    st->n_rendered = (int64_t)v.D;
    st->n_visible = (int32_t)(v.visible & 0x7FFFFFFFu);
    st->max_tile_instances = (int32_t)v.max_tile;
    st->compact_binning = v.oc.binning;
    st->preprocess_form = h->last_form;
    st->bins_bytes = (int64_t)(compact ? v.D * 8 : (uint64_t)(h->n_tiles + 1) * v.plan.bin_cap_view * 8ull + (hybrid ? v.D * 8 : 0));
    st->bin_capacity = v.plan.bin_cap_view;
    st->tier_tiles[0] = v.n_mid4; st->tier_tiles[1] = v.n_mid8; st->tier_tiles[2] = v.n_big;
    st->reserved = 0;
    fill_history(h, st);  // (again at the end: the buffers this view grows are counted there)
}

// Read-back: the one host sync, then what this view turned out to be.
static int fwd_read_back(gsr_handle* h, FwdView& v) {
    int rc;
    if ((rc = wait_totals(h->host_totals + GSR_TOTAL_SEQ, &h->wait_ema_us, v.seq, v.s))) return rc;
    // What this view turned out to be — bins / overflow tiles / compact; whether the fused launch covers it; where the tier
    // walk goes; the bins' capacity for the next view — is gsr_policy_end_view's decision on the scan's counts.
    // OVERFLOW TILES (round 5): lists longer than the bins' capacity.  Their bins hold the first bin_cap_view arrivals only
    // (preprocess counted every instance); their complete key lists come from a scatter pass restricted to them
    // (fwd_sort_and_walk), and every sort takes a tile's keys from wherever they are complete.  The rest of the view stays on
    // the fast path.
    const uint32_t* t = h->host_totals;
    v.D = t[GSR_TOTAL_D]; v.D_slots = t[GSR_TOTAL_SLOTS]; v.max_tile = t[GSR_TOTAL_MAX_LIST];
    v.n_big = t[GSR_TOTAL_BIG]; v.n_mid4 = t[GSR_TOTAL_MID4]; v.n_mid8 = t[GSR_TOTAL_MID8]; v.visible = t[GSR_TOTAL_VISIBLE];
    gsr_policy_end_view(&h->pcfg, &h->pol, &v.plan, (int64_t)v.D, v.max_tile, v.n_mid4, v.n_mid8, v.n_big, v.cap_instances,
                        v.spec ? 1 : 0, &v.oc);
    h->last_n = v.n;
    h->last_D = (int64_t)v.D;
    h->last_slots = (int64_t)v.D_slots;
    h->last_compact = v.oc.binning == GSR_BINNING_COMPACT;
    if (v.stats) fill_view_stats(h, v, v.stats);
    return GSR_OK;
}

// Empty view (D == 0): nothing to sort or blend.
static int fwd_empty_view(gsr_handle* h, const FwdView& v) {
    const hipStream_t s = v.s;
    const size_t P = (size_t)h->cfg.width * h->cfg.height, T = (size_t)h->n_tiles;
    h->tile_count_dirty = false;  // every counter is zero
    if (v.k.exact_cull && (v.visible >> 31)) {
        // exact-cull mode dropped every instance (all of them invisible: opacities below 1/255) of a view the reference WOULD
        // have rendered (some rect holds a tile): its pixels blend nothing and show the background, as with the reference's
        // lists — the all-zero image below is the reference's answer to "no instance at all" only
        gsr_launch_fill_background(s, P, v.C, frame_of(h, v.in->background, v.image_out, v.aux));
    } else {
        // rasterizer.jl:283,338: all-zero image, background not applied
        HIPCHK(hipMemsetAsync(v.image_out, 0, P * v.C * 4, s));
        HIPCHK(hipMemsetAsync(h->n_contrib.p, 0, P * 4, s));
        HIPCHK(hipMemsetAsync(h->final_T.p, 0, P * 4, s));
    }
    HIPCHK(hipMemsetAsync(h->ranges.p, 0, 2 * T * 4, s));
    if (v.aux && v.aux->uncertainties) HIPCHK(hipMemsetAsync(v.aux->uncertainties, 0, P * 4, s));
    h->fwd_valid = true;
    return GSR_OK;
}

// Instance buffers: grow-only, sized by the counts just read.
static int fwd_instance_buffers(gsr_handle* h, FwdView& v) {
    int rc;
    const gsr_instance_bytes b = gsr_sizes_per_instance(v.D, v.D_slots, v.C);
    const float slack = 1.25f;  // instance count drifts slowly between training steps
    // forward-only and everything composited by the fused launch: no per-instance storage at all (the rare paths of
    // fwd_sort_and_walk — tier lists, compact binning — still hand their instances over through the stream)
    const bool need_stream = !(v.fwd_only && v.oc.fused_done && !v.oc.long_tiles);
    if (need_stream &&
        ((rc = h->values_sorted.ensure(b.values_sorted, slack)) ||
         (rc = h->s0.ensure(b.stream, slack)) || (rc = h->s1.ensure(b.stream, slack)) ||
         (rc = h->s2.ensure(b.stream, slack)) || (v.C > 3 && (rc = h->s3.ensure(b.s3, slack)))))
        return rc;
    if (!v.fwd_only && (rc = h->rows.ensure(b.rows, slack))) return rc;
    v.slab_stride = 0;
    if (v.n_big > 0) {  // lists beyond the LDS sort: two merge slabs per listed tile
        v.slab_stride = ((size_t)v.max_tile + 63) & ~(size_t)63;
        // (+ the plan of the multi-workgroup sort: 2 (n_big + 1) words behind the slabs)
        if ((rc = h->big_scratch.ensure((size_t)v.n_big * 2 * v.slab_stride * 8 + (size_t)(2 * v.n_big + 2) * 4 + 64))) return rc;
    }
    return GSR_OK;
}

// Sort and tier walk: whatever the launches behind the scan left of the view.
static int fwd_sort_and_walk(gsr_handle* h, const FwdView& v) {
    int rc;
    const hipStream_t s = v.s;
    const size_t T = (size_t)h->n_tiles;
    const float slack = 1.25f;
    const bool fused_done = v.oc.fused_done != 0, beside = v.oc.beside != 0;
    // (a held fused launch that this view gives no reason to hold any longer — no tier tiles after all, or too many — goes out
    // now; one that would only find its buffers too small — the kernel checks the same totals — is not launched at all: the
    // main sort pass then re-zeroes the counters and writes the ranges, as in every view without the fused launch)
    if (v.oc.launch_fused_now) launch_fused(h, v, s);
    if (fused_done && !v.oc.long_tiles) return GSR_OK;
    StageScope sc4(h->prof, ST_SORT, s);
    GsrKeys keys = bins_of(h, v.plan.bin_cap_view);
    if (v.oc.binning == GSR_BINNING_COMPACT) {
        // count -> scan -> scatter: the counters become the fill cursors of the scatter pass
        if ((rc = h->keys_compact.ensure(v.D * 8, slack))) return rc;
        HIPCHK(hipMemsetAsync(h->tile_count.p, 0, (T + 2) * 4, s));
        gsr_launch_emit_compact(s, v.n, v.k, geom_of(h), h->tile_start.as<uint32_t>(), h->tile_count.as<uint32_t>(),
                                h->keys_compact.as<uint64_t>(), v.max_tile, /*only_above=*/0u);
        keys = GsrKeys{h->keys_compact.as<uint64_t>(), 0u, nullptr};
    } else if (v.oc.binning == GSR_BINNING_OVERFLOW) {
        // the scatter pass restricted to the lists beyond the bins' capacity: their keys go to keys_compact at the offsets of
        // the compact layout (the buffer is sized as for it; only those segments are touched), with fill cursors of its own
        // (the tile counters belong to the fused launch, which re-zeroes them)
        if ((rc = h->keys_compact.ensure(v.D * 8, slack)) || (rc = h->overflow_fill.ensure((T + 2) * 4))) return rc;
        HIPCHK(hipMemsetAsync(h->overflow_fill.p, 0, (T + 2) * 4, s));
        gsr_launch_emit_compact(s, v.n, v.k, geom_of(h), h->tile_start.as<uint32_t>(), h->overflow_fill.as<uint32_t>(),
                                h->keys_compact.as<uint64_t>(), v.max_tile, /*only_above=*/keys.cap);
        keys.overflow = h->keys_compact.as<uint64_t>();
    }
    // (sorted_mid4 / sorted_mid8: what the speculative mid-tier sorts covered — gsr_policy_end_view: the kernels' own test, on
    // the same numbers)
    gsr_launch_tile_sort(s, v.C, /*main_pass=*/!fused_done, tiles_of(h), keys, v.n_mid4, v.n_mid8, v.n_big, v.oc.sorted_mid4,
                         v.oc.sorted_mid8, h->big_scratch.as<uint64_t>(), v.slab_stride, geom_of(h), stream_of(h),
                         h->values_sorted.as<uint32_t>());
    sc4.close();
    // the walk of the tier tiles: beside the held fused launch (second stream, first in the queue), else behind it
    const hipStream_t ws = beside ? h->aux_stream : s;
    if (beside) {
        HIPCHK(hipEventRecord(h->ev_fork, s));
        HIPCHK(hipStreamWaitEvent(h->aux_stream, h->ev_fork, 0));
    }
    StageScope sc5(h->prof, ST_COMPOSITE_FWD, ws);
    // after the fused launch only the tiles of the tier lists are left; otherwise every tile
    const GsrTierLists tiers{h->big_list.as<uint32_t>(), (uint32_t)h->n_tiles, v.n_big, v.n_mid8, v.n_mid4, beside ? 1u : 0u};
    gsr_launch_composite_fwd(ws, v.C, v.k, tiles_of(h), stream_of(h), frame_of(h, v.in->background, v.image_out, v.aux, v.scores),
                             fused_done ? &tiers : nullptr);
    sc5.close();
    if (beside) {
        HIPCHK(hipEventRecord(h->ev_join, h->aux_stream));
        launch_fused(h, v, s);
        HIPCHK(hipStreamWaitEvent(s, h->ev_join, 0));
    }
    return GSR_OK;
}

int gsr_forward(gsr_handle* h, const gsr_inputs* in, const gsr_camera* cam, float* image_out, const gsr_aux* aux,
                void* stream_v, gsr_stats* stats) {
    return gsr_forward_scored(h, in, cam, image_out, aux, nullptr, stream_v, stats);
}

// The forward, with or without gsr_scores (the scored kernels of composite.hip only where an array was asked for).
int gsr_forward_scored(gsr_handle* h, const gsr_inputs* in, const gsr_camera* cam, float* image_out, const gsr_aux* aux,
                       const gsr_scores* scores, void* stream_v, gsr_stats* stats) {
    FwdView v;
    int rc;
    if ((rc = fwd_begin(h, in, cam, image_out, aux, scores, stream_v, stats, v))) return rc;
    if ((rc = fwd_plan_and_bin(h, v))) return rc;
    if ((rc = fwd_read_back(h, v))) return rc;
    if (v.D == 0) return fwd_empty_view(h, v);
    if ((rc = fwd_instance_buffers(h, v))) return rc;
    if ((rc = fwd_sort_and_walk(h, v))) return rc;
    h->tile_count_dirty = false;  // the sort (fused or not) zeroed the counters
    HIPCHK(hipGetLastError());
    if (stats) fill_history(h, stats);
    h->fwd_valid = true;
    return GSR_OK;
}

// ∇render! of the last forward.  One wave walks a tile's list in the main launch; a list of tens of thousands of
// instances is then milliseconds of ONE wave (§8 of DESIGN.md).  As long as such tiles are too few to fill the GPU by
// themselves (at most one per CU), they are taken out of the main launch and walked by four waves each on the
// handle's second stream, forked from and joined back into the caller's stream.  The cut is a tier boundary of the
// scan (> 8192, > 4096 or > 1024 instances): the deepest tiers first, as many as fit the limit.  Four waves cost
// ~20 % more work per instance, so when long tiles are plentiful they stay with the main launch.
// job: the row-independent job for the tile-walk launch to carry, or NULL; *job_carried: whether it did (gsr_launch_composite_bwd).
static int launch_composite_bwd(gsr_handle* h, hipStream_t s, int C, const GsrCam& k, const float* background,
                                const float* vpixels, bool color_only, const GsrRowJob* job, bool* job_carried) {
    color_only = color_only && C > 3;
    // which tiers leave the main launch: gsr_policy_bwd_split (its limit: gsr_policy_config.bwd_split_max_tiles)
    gsr_bwd_split sp;
    gsr_policy_bwd_split(&h->pcfg, h->pol.tier_n[0], h->pol.tier_n[1], h->pol.tier_n[2], &sp);
    // (the accurate per-pixel arithmetic exists for the one-wave-per-tile kernel only: such a handle splits nothing)
    const bool accurate = h->cfg.grad_precision != GSR_DEFAULT;
    if (accurate) { sp.n_big = sp.n_mid8 = sp.n_mid4 = 0; sp.split_len = 0xFFFFFFFFu; }
    GsrTierLists tiers{h->big_list.as<uint32_t>(), (uint32_t)h->n_tiles, sp.n_big, sp.n_mid8, sp.n_mid4, sp.split_len};
    const uint32_t n = sp.n_big + sp.n_mid8 + sp.n_mid4;
    const GsrFrame frame = frame_of(h, background, nullptr, nullptr);
    if (n > 0) {
        // per (listed tile, list segment, pixel): the (m, c) of the segment — the first pass's hand-over to the second
        int rc = h->long_state.ensure((size_t)n * GSR_BWD_LONG_SEGS * 256 * 2 * sizeof(float));
        if (rc) return rc;
        HIPCHK(hipEventRecord(h->ev_fork, s));
        HIPCHK(hipStreamWaitEvent(h->aux_stream, h->ev_fork, 0));
        gsr_launch_composite_bwd_listed(h->aux_stream, C, k, tiles_of(h), tiers, stream_of(h), frame, vpixels, inst_of(h),
                                        h->long_state.as<float>());
        HIPCHK(hipEventRecord(h->ev_join, h->aux_stream));
    }
    *job_carried = gsr_launch_composite_bwd(s, C, k, tiles_of(h), stream_of(h), frame, vpixels, inst_of(h), job, tiers.split_len,
                                            color_only, accurate);
    if (n > 0) HIPCHK(hipStreamWaitEvent(s, h->ev_join, 0));
    return GSR_OK;
}

// What both backward entry points ask of the handle's last forward (`entry`: the entry point's name, for the messages).
static int check_backward_state(const gsr_handle* h, const gsr_inputs* in, const char* entry) {
    if (!h->fwd_valid && h->dropped_by_reserve)
        return fail(GSR_E_STATE, "%s: a gsr_reserve that reallocated scratch (or gsr_drop_forward) dropped the handle's last "
                    "forward; run gsr_forward again", entry);
    if (!h->fwd_valid || h->last_n != in->n)
        return fail(GSR_E_STATE, "%s without a matching gsr_forward on this handle", entry);
    if (h->fwd_only)
        return fail(GSR_E_STATE, "the handle's last forward was GSR_FORWARD_ONLY: it kept no backward state");
    if (h->inputs_consumed)
        return fail(GSR_E_STATE, "the inputs of the handle's last forward were updated in place by "
                    "gsr_backward_trainer_tail; run gsr_forward again");
    return GSR_OK;
}

// ... and what both do once their arguments are checked: ∇means_2d goes to the caller's array or the handle's scratch, a
// cotangent declared colour-only is checked where asked (GSR_CHECK_COLOR_COTANGENT), the compositing backward runs as its stage.
// grads: gsr_backward's gradient arrays — the row-independent job of the :rgb tile walk writes the zero rows of culled Gaussians
// into them and the SH direction Jacobians into the handle's sh_jac; NULL (the trainer tail): no job.  *job_carried: the per-
// Gaussian kernel behind may read sh_jac and leave those rows alone (false wherever no launch carried the job: an empty view,
// another mode or background, the accurate kernels, the factored SH gradient).
static int composite_bwd_stage(gsr_handle* h, hipStream_t s, const gsr_inputs* in, const gsr_camera* cam, const float* vpixels,
                               float* vmeans2d, uint32_t flags, GsrCam* k, const gsr_grads* grads, bool* job_carried) {
    int rc;
    *job_carried = false;
    if (!vmeans2d && (rc = h->vmean2d.ensure(gaussian_bytes(h, in->n).vmean2d, 1.25f))) return rc;
    h->vmean2d_cur = vmeans2d ? reinterpret_cast<float2*>(vmeans2d) : h->vmean2d.as<float2>();
    const bool color_only = (flags & GSR_GRADS_COLOR_COTANGENT) != 0u;
    if (color_only && (rc = check_color_cotangent(h, vpixels, s))) return rc;
    *k = make_cam(h, cam);
    GsrRowJob job{};
    // (the conditions of the one launch that carries it — composite_bwd_kernel_rgb_bg0 — so that no other backward allocates sh_jac.
    //  It grows here, with the slack of the forward's per-Gaussian scratch, not in gsr_reserve: what a reserve allocates per mode is
    //  pinned byte for byte by tests/test_gpu_handle_bytes.py, and most :rgb handles — a background, another precision — never use it)
    const bool bg_zero = in->background[0] == 0.0f && in->background[1] == 0.0f && in->background[2] == 0.0f;
    if (grads && grads->vshs && !grads->vcolors && h->cfg.mode == 3 && bg_zero && h->cfg.grad_precision == GSR_DEFAULT &&
        h->last_D > 0) {
        gsr_bwd_row_job rj;
        gsr_policy_bwd_row_job(&h->pcfg, in->n, &rj);
        if ((rc = h->sh_jac.ensure(gaussian_bytes(h, in->n).sh_jac, 1.25f))) return rc;
        job.n_wg = rj.n_wg; job.slice = rj.slice;
        job.n = in->n; job.K = in->n_coeffs; job.degree = in->sh_degree;
        job.means = in->means; job.shs = in->shs; job.radii = h->radii_cur;
        for (int c = 0; c < 3; c++) job.center[c] = k->center[c];
        job.jac = h->sh_jac.as<float>();
        job.vmeans = grads->vmeans; job.vshs = grads->vshs; job.vopac = grads->vopacities; job.vscales = grads->vscales;
        job.vrots = reinterpret_cast<float4*>(grads->vrotations);
    }
    StageScope sc(h->prof, ST_COMPOSITE_BWD, s);
    if (h->last_D > 0 &&
        (rc = launch_composite_bwd(h, s, h->cfg.mode, *k, in->background, vpixels, color_only, job.n_wg ? &job : nullptr, job_carried)))
        return rc;
    sc.close();
    return GSR_OK;
}

int gsr_backward(gsr_handle* h, const gsr_inputs* in, const gsr_camera* cam, const float* vpixels,
                 const gsr_grads* g, void* stream_v) {
    int rc = check_inputs(h, in, cam);
    if (rc) return rc;
    if (!vpixels || !g) return fail(GSR_E_INVALID_ARG, "null vpixels / grads");
    if ((rc = check_backward_state(h, in, "gsr_backward"))) return rc;
    if ((g->flags & ~GSR_GRADS_COLOR_COTANGENT) != 0u || g->reserved != 0u) return fail(GSR_E_INVALID_ARG, "unknown gsr_grads.flags / reserved bits");
    if (g->forward_generation != 0 && g->forward_generation != h->generation)
        return fail(GSR_E_STATE, "gsr_backward for forward #%llu, but the handle's last forward is #%llu (another "
                    "gsr_forward ran in between)", (unsigned long long)g->forward_generation,
                    (unsigned long long)h->generation);
    if (in->n > 0 && (!g->vmeans || (!g->vshs && !g->vcolors) || !g->vopacities || !g->vscales || !g->vrotations))
        return fail(GSR_E_INVALID_ARG, "null gradient buffer");
    if ((g->vR == nullptr) != (g->vt == nullptr)) return fail(GSR_E_INVALID_ARG, "vR and vt must be given together");
    if (((uintptr_t)g->vrotations & 15) != 0) return fail(GSR_E_INVALID_ARG, "vrotations must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream_v;
    const int C = h->cfg.mode, n = in->n;
    if (n == 0) return GSR_OK;
    // (nothing is cleared and nothing is accumulated into: composite_bwd writes the row of every emitted instance, pergauss_bwd
    // skips the slots of culled tiles, and the pose gradient goes through per-workgroup partials that are all stored, then summed
    // in a fixed order — the "zero_acc" stage stays in the table, empty)
    if (g->vR && (rc = h->pose_part.ensure(gaussian_bytes(h, n).pose_part, 1.25f))) return rc;
    GsrCam k;
    bool job_carried = false;
    if ((rc = composite_bwd_stage(h, s, in, cam, vpixels, g->vmeans2d, g->flags, &k, g, &job_carried))) return rc;
    StageScope sc8(h->prof, ST_PERGAUSS_BWD, s);
    gsr_launch_pergauss_bwd(s, n, in->n_coeffs, in->sh_degree, C, in->means, in->scales, in->rotations, in->shs, k,
                            geom_of(h), inst_of(h), h->vmean2d_cur, g->vmeans, g->vshs, g->vopacities,
                            g->vscales, g->vrotations, g->vR, g->vt, h->pose_part.as<float>(), g->vcolors,
                            /*fp32_chain=*/h->cfg.grad_precision == GSR_GRAD_FP32_REFERENCE,
                            antialiased(h) ? in->opacities : nullptr, comp_of(h), job_carried ? h->sh_jac.as<float>() : nullptr);
    sc8.close();
    HIPCHK(hipGetLastError());
    h->bwd_valid = true;
    return GSR_OK;
}

static int buffer_lookup(const gsr_handle* h, int which, const void** dev_ptr, size_t* bytes) {
    const size_t n = (size_t)h->last_n, P = (size_t)h->cfg.width * h->cfg.height, T = (size_t)h->n_tiles;
    // what the last forward's n Gaussians and D instances fill (a forward of no Gaussian: nothing, whatever it allocated)
    const gsr_gaussian_bytes gb = n ? gaussian_bytes(h, h->last_n) : gsr_gaussian_bytes{};
    const gsr_instance_bytes ib = gsr_sizes_per_instance((uint64_t)h->last_D, (uint64_t)h->last_slots, h->cfg.mode);
    const DevBuf* b = nullptr;
    size_t sz = 0;
    switch (which) {
        case GSR_BUF_RADII:  // handle-owned, or the caller's gsr_aux.radii of the last forward
            *dev_ptr = h->fwd_valid && n ? h->radii_cur : nullptr;
            *bytes = *dev_ptr ? gb.radii : 0;
            return GSR_OK;
        case GSR_BUF_GRAD_MEANS2D:
            *dev_ptr = h->bwd_valid && n ? h->vmean2d_cur : nullptr;
            *bytes = *dev_ptr ? gb.vmean2d : 0;
            return GSR_OK;
        case GSR_BUF_COMPENSATIONS:  // per-forward state like the radii; a handle without GSR_FLAG_ANTIALIASED has none
            *dev_ptr = h->fwd_valid && n && gb.comp && gb.comp <= h->comp.cap ? h->comp.p : nullptr;
            *bytes = *dev_ptr ? gb.comp : 0;
            return GSR_OK;
        case GSR_BUF_N_CONTRIB: b = &h->n_contrib; sz = P * 4; break;
        case GSR_BUF_FINAL_T: b = &h->final_T; sz = P * 4; break;
        case GSR_BUF_TILE_RANGES: b = &h->ranges; sz = 2 * T * 4; break;
        case GSR_BUF_VALUES_SORTED: b = &h->values_sorted; sz = h->fwd_only ? 0 : ib.values_sorted; break;
        case GSR_BUF_GEOM: b = &h->geo; sz = gb.geo; break;
        case GSR_BUF_NORMALS: b = &h->gnormal; sz = gb.gnormal; break;
        // (the rows as the backward packs them — 48 bytes per slot in :rgb mode — inside the 64 per slot of ib.rows)
        case GSR_BUF_GRAD_ROWS: b = &h->rows; sz = (size_t)h->last_slots * 16 * GSR_ROW_F4(h->cfg.mode); break;
        case GSR_BUF_INSTANCE_AUX: b = &h->s2; sz = h->fwd_only ? 0 : ib.stream; break;
        default: return fail(GSR_E_INVALID_ARG, "unknown buffer id %d", which);
    }
    if (sz > b->cap) sz = 0;  // not produced yet
    *dev_ptr = sz ? b->p : nullptr;
    *bytes = sz;
    return GSR_OK;
}

int gsr_buffer(const gsr_handle* h, int which, const void** dev_ptr, size_t* bytes) {
    if (!h || !dev_ptr || !bytes) return fail(GSR_E_INVALID_ARG, "null argument");
    return buffer_lookup(h, which, dev_ptr, bytes);
}

int gsr_copy_buffer(const gsr_handle* h, int which, void* dst, size_t bytes, void* stream) {
    if (!h || (!dst && bytes)) return fail(GSR_E_INVALID_ARG, "null argument");
    const void* src = nullptr;
    size_t have = 0;
    int rc = buffer_lookup(h, which, &src, &have);
    if (rc) return rc;
    if (bytes > have) return fail(GSR_E_STATE, "buffer %d holds %zu bytes, %zu requested (not produced yet?)", which, have, bytes);
    if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return GSR_OK;
}

int gsr_loss_l1_ssim(gsr_handle* h, const float* image, const float* target, float lambda_dssim, float* loss_out,
                     float* vpixels, void* stream) {
    if (!h || !image || !target || !loss_out || !vpixels) return fail(GSR_E_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int W = h->cfg.width, H = h->cfg.height, C = h->cfg.mode;
    const size_t P = (size_t)W * H;
    if (P * C > 0xFFFFFFFFull) return fail(GSR_E_INVALID_ARG, "image too large for the loss head");  // 32-bit offsets inside it
    // ONE decision for the forward and the pullback of this call, from the handle (ABI 5) or the process default
    const int exact = ssim_exact_of(h);
    int rc;
    if ((rc = h->d0.ensure(3 * P * 4)) || (rc = h->d1.ensure(3 * P * 4)) || (rc = h->d2.ensure(3 * P * 4)) ||
        (rc = h->partial.ensure((exact ? gsr_loss_partial_pairs_exact : gsr_loss_partial_pairs_fast)(W, H) * 2 * 4)))
        return rc;
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;  // fused_ssim.jl:374
    StageScope sc9(h->prof, ST_LOSS_FWD, s);
    (exact ? gsr_launch_loss_fwd_exact : gsr_launch_loss_fwd_fast)(s, W, H, C, image, target, C1, C2, h->d0.as<float>(),
                                                                          h->d1.as<float>(), h->d2.as<float>(), h->partial.as<float>());
    sc9.close();
    StageScope sc10(h->prof, ST_LOSS_BWD, s);
    (exact ? gsr_launch_loss_bwd_exact : gsr_launch_loss_bwd_fast)(s, W, H, C, image, target, lambda_dssim, h->d0.as<float>(),
                                                                          h->d1.as<float>(), h->d2.as<float>(), h->partial.as<float>(),
                                                                          loss_out, vpixels);
    sc10.close();
    HIPCHK(hipGetLastError());
    // the cotangent of this forward whose channels >= 3 are zeros by construction (GSR_GRADS_COLOR_COTANGENT)
    h->loss_vpixels = vpixels;
    h->loss_generation = h->generation;
    return GSR_OK;
}

int gsr_update_stats(gsr_handle* h, int32_t* max_radii, float* accum_grad_means2d, float* denom, void* stream) {
    if (!h || !max_radii || !accum_grad_means2d || !denom) return fail(GSR_E_INVALID_ARG, "null argument");
    if (!h->fwd_valid && h->dropped_by_reserve)
        return fail(GSR_E_STATE, "gsr_update_stats: a gsr_reserve that reallocated scratch (or gsr_drop_forward) dropped the "
                    "handle's last forward/backward pair");
    if (!h->fwd_valid || !h->bwd_valid) return fail(GSR_E_STATE, "gsr_update_stats needs a completed forward/backward pair");
    gsr_launch_update_stats((hipStream_t)stream, h->last_n, h->radii_cur, h->vmean2d_cur,
                            h->cfg.width, h->cfg.height, max_radii, accum_grad_means2d, denom);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_profile_enable(gsr_handle* h, int on) {
    if (!h) return fail(GSR_E_INVALID_ARG, "null handle");
    h->prof.on = (on & 1) != 0;      // bit 0: HIP-event stage timing
    h->prof.ranges = (on & 2) != 0;  // bit 1: roctx range per stage
    if (!h->prof.on) h->prof.clear();
    return GSR_OK;
}

int gsr_profile_stages(gsr_handle* h, uint32_t stage_mask) {
    if (!h) return fail(GSR_E_INVALID_ARG, "null handle");
    h->prof.mask = stage_mask;
    return GSR_OK;
}

int gsr_profile_stage_count(void) { return ST_COUNT; }
const char* gsr_profile_stage_name(int stage) { return stage >= 0 && stage < ST_COUNT ? kStageNames[stage] : ""; }

int gsr_profile_read(gsr_handle* h, double* ms_sum, int* launches, int reset) {
    if (!h || !ms_sum || !launches) return fail(GSR_E_INVALID_ARG, "null argument");
    for (int i = 0; i < ST_COUNT; i++) { ms_sum[i] = 0.0; launches[i] = 0; }
    for (auto& r : h->prof.recs) {
        float ms = 0.0f;
        HIPCHK(hipEventSynchronize(r.b));
        HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
        ms_sum[r.stage] += ms;
        if (!r.extra) launches[r.stage] += 1;
    }
    if (reset) h->prof.clear();
    return GSR_OK;
}

int gsr_profile_read_intervals(gsr_handle* h, int stage, double* ms_out, int max_n, int* n_out) {
    if (!h || !n_out || (max_n > 0 && !ms_out)) return fail(GSR_E_INVALID_ARG, "null argument");
    if (stage < 0 || stage >= ST_COUNT) return fail(GSR_E_INVALID_ARG, "unknown stage %d", stage);
    int n = 0;
    hipEvent_t prev = nullptr;
    for (auto& r : h->prof.recs) {
        if (r.stage != stage || r.extra) continue;
        if (prev) {
            if (n < max_n) {
                float ms = 0.0f;
                HIPCHK(hipEventSynchronize(r.a));
                HIPCHK(hipEventElapsedTime(&ms, prev, r.a));
                ms_out[n] = ms;
            }
            n++;
        }
        prev = r.a;
    }
    *n_out = n;
    return GSR_OK;
}

int gsr_backward_trainer_tail(gsr_handle* h, const gsr_inputs* in, const gsr_camera* cam, const float* vpixels,
                              const gsr_tail_state* st, void* stream_v) {
    int rc = check_inputs(h, in, cam);
    if (rc) return rc;
    if (!vpixels || !st) return fail(GSR_E_INVALID_ARG, "null vpixels / tail state");
    if ((rc = check_backward_state(h, in, "gsr_backward_trainer_tail"))) return rc;
    if ((st->flags & ~GSR_GRADS_COLOR_COTANGENT) != 0u || st->reserved != 0u) return fail(GSR_E_INVALID_ARG, "unknown gsr_tail_state.flags / reserved bits");
    if (st->forward_generation != 0 && st->forward_generation != h->generation)
        return fail(GSR_E_STATE, "gsr_backward_trainer_tail for forward #%llu, but the handle's last forward is #%llu",
                    (unsigned long long)st->forward_generation, (unsigned long long)h->generation);
    if (st->scale_dims != 1 && st->scale_dims != 3) return fail(GSR_E_INVALID_ARG, "scale_dims must be 1 or 3");
    const int n = in->n, K = in->n_coeffs;
    if (n == 0) return GSR_OK;
    float lr_t[6];
    if ((rc = tail_lr_t(st->theta, st->mu, st->nu, st->lr, st->current_step, st->beta1, st->beta2, /*rest_empty=*/K == 1, lr_t)))
        return rc;
    // the kernel reads its inputs through the trainer's arrays and updates them in place
    if (in->means != st->theta[0] || in->rotations != st->theta[5] || in->shs != st->shs ||
        in->opacities != st->opacities_act || in->scales != st->scales_act)
        return fail(GSR_E_INVALID_ARG, "the inputs of the fused step must be the trainer's own arrays (means == theta[0], "
                    "rotations == theta[5], shs / opacities / scales == the activated copies)");
    if (((uintptr_t)st->theta[5] & 15) != 0) return fail(GSR_E_INVALID_ARG, "rotations must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream_v;
    const int C = h->cfg.mode;
    GsrCam k;
    bool no_job = false;
    if ((rc = composite_bwd_stage(h, s, in, cam, vpixels, st->vmeans2d, st->flags, &k, nullptr, &no_job))) return rc;
    StageScope sc12(h->prof, ST_PERGAUSS_BWD, s);
    const gsr::TailState S = gsr_make_tail_state(st->theta, st->mu, st->nu, lr_t, st->beta1, st->beta2, st->eps,
                                                 st->scale_dims, st->shs, st->opacities_act, st->scales_act);
    gsr_launch_pergauss_bwd_tail(s, n, K, in->sh_degree, C, k, geom_of(h), inst_of(h), h->vmean2d_cur, S,
                                 /*fp32_chain=*/h->cfg.grad_precision == GSR_GRAD_FP32_REFERENCE, comp_of(h));
    sc12.close();
    HIPCHK(hipGetLastError());
    h->bwd_valid = true;
    // the forward's inputs no longer exist (updated in place): a second backward on this forward would differentiate
    // the wrong parameters (the forward's own outputs — radii, tile lists, image — stay readable)
    h->inputs_consumed = true;
    return GSR_OK;
}

}  // extern "C"
