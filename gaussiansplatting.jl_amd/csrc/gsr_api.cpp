// C ABI of libgsr_hip.so (include/gsr.h): handle object with grow-only scratch, argument
// validation, kernel orchestration.  Mirrors the host side of the reference's
// `GaussianRasterizer` / `rasterize` / `∇rasterize` (src/rasterization/rasterizer.jl:5-90,
// 255-408, 416-550) — everything is enqueued on the caller's stream; the only host sync is
// the instance-count read-back (rasterizer.jl:337).
#include "../../include/gsr.h"

#include <dlfcn.h>
#include <math.h>
#include <sched.h>
#include <time.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "gsr_kernels.h"
#include "adam_math.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail(e_ == hipErrorOutOfMemory ? GSR_E_OOM : GSR_E_HIP, "%s failed: %s (%s:%d)", #expr,   \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                          \
    } while (0)

// GSR_DEBUG_FILL=nan | big (debugging, read at every allocation): each new allocation of a buffer marked `fill_ok` is filled
// with the 32-bit word 0xFFFFFFFF (a NaN) or 0x7F7F7F7F (3.4e38, finite: NaN hides behind comparisons), so that a kernel
// that reads a float it never wrote shows up in the result instead of reading the zeros of fresh pages.  0 = unset.
uint32_t debug_fill_word() {
    const char* e = getenv("GSR_DEBUG_FILL");
    if (!e) return 0u;
    if (!strcmp(e, "nan")) return 0xFFFFFFFFu;
    if (!strcmp(e, "big")) return 0x7F7F7F7Fu;
    return 0u;
}

// GSR_DEBUG_GUARD=1 (debugging, read at every allocation): every handle buffer is allocated kGuardBytes longer than asked for and
// the extra bytes — right behind `cap`, which stays what it would have been, so that nothing the library derives from a
// capacity moves — are filled with a guard word.  gsr_debug_check_guards (and every free of such a buffer) compares them: a
// kernel that stores past the end of a handle buffer is named instead of silently corrupting the neighbouring allocation.
bool debug_guard_on() {
    const char* e = getenv("GSR_DEBUG_GUARD");
    return e && e[0] == '1' && !e[1];
}
constexpr size_t kGuardBytes = 4096;
struct GuardDamage {  // the first damaged guard seen on a handle (remembered across the free of its buffer)
    bool set = false;
    const char* name = "";
    size_t offset = 0;   // bytes past cap
    uint32_t word = 0;   // what was found there
    uint32_t expect = 0;
};

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
    uint32_t regrowths = 0;  // reallocations of a buffer that already existed (each is a device synchronisation)
    // GSR_DEBUG_FILL may fill it: floats only, none of which ever becomes an address, a loop bound or a branch that leaves the
    // allocation (set in gsr_create; index / key / count / mask buffers never are: garbage there is a wild address)
    bool fill_ok = false;
    // GSR_DEBUG_GUARD: the name the check reports; whether THIS allocation carries a guard; the word of a buffer that is not
    // fill_ok (those get 0x7F7F7F7F).  By the rule above an index / count buffer's guard holds a small valid value: 1 — one
    // instance, offset 1, tile-list range [1, 1), radius 1, a 64-bit key of tile 0 — and unlike 0 it differs from what a
    // stray clear would leave.  The three buffers whose words are ids that need not have a second element (tile ids of a
    // one-tile image, Gaussian ids of a one-Gaussian scene) get 0 (set in gsr_create).
    const char* name = "?";
    bool guarded = false;
    uint32_t guard_word = 1u;
    GuardDamage* damage = nullptr;
    uint32_t guard_value() const { return fill_ok ? 0x7F7F7F7Fu : guard_word; }
    // Compares the guard with its word (synchronises the device); the first difference is remembered in *damage.
    int check_guard() {
        if (!p || !guarded || !damage) return GSR_OK;
        static thread_local uint32_t host[kGuardBytes / 4];
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(host, (const char*)p + cap, kGuardBytes, hipMemcpyDeviceToHost));
        const uint32_t w = guard_value();
        for (size_t i = 0; i < kGuardBytes / 4; i++) {
            if (host[i] != w) {
                if (!damage->set) *damage = GuardDamage{true, name, i * 4, host[i], w};
                break;
            }
        }
        return GSR_OK;
    }
    // grow-only, like the reference's scratch (rasterizer.jl:275-278,340-343)
    int ensure(size_t bytes, float slack = 1.0f) {
        if (bytes <= cap) return GSR_OK;
        size_t want = (size_t)((double)bytes * slack);
        if (p) {
            // REgrowth of a buffer that is given slack (the per-Gaussian and per-instance scratch of a scene that changes): at
            // least half again of what is there — the views of a batch differ by a few per cent in their instance count, and a
            // training run grows; 288 GB of HBM are there to be used, a hipFree + hipMalloc synchronises the device
            if (slack > 1.0f) want = std::max(want, cap + cap / 2);
            regrowths++;
            if (int rc = check_guard()) return rc;
            HIPCHK(hipFree(p));
            p = nullptr;
            cap = 0;
            guarded = false;
        }
        want = (want + 255) & ~(size_t)255;
        const bool guard = debug_guard_on();
        HIPCHK(hipMalloc(&p, want + (guard ? kGuardBytes : 0)));
        cap = want;
        guarded = guard;
        bool wrote = false;
        if (fill_ok) {
            if (const uint32_t w = debug_fill_word()) {
                // synchronised: the library's kernels also run on its own non-blocking aux_stream
                HIPCHK(hipMemsetD32((hipDeviceptr_t)p, (int)w, want / 4));
                wrote = true;
            }
        }
        if (guard) {
            HIPCHK(hipMemsetD32((hipDeviceptr_t)((char*)p + want), (int)guard_value(), kGuardBytes / 4));
            wrote = true;
        }
        if (wrote) HIPCHK(hipDeviceSynchronize());
        return GSR_OK;
    }
    int release() {
        if (p) {
            if (int rc = check_guard()) return rc;
            HIPCHK(hipFree(p));
        }
        p = nullptr;
        cap = 0;
        guarded = false;
        return GSR_OK;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Optional per-stage timing with HIP events on the caller's stream (gsr_profile_*).
enum Stage { ST_PREPROCESS, ST_SCAN, ST_SORT, ST_COMPOSITE_FWD, ST_LOSS_FWD, ST_LOSS_BWD, ST_ZERO_ACC,
             ST_COMPOSITE_BWD, ST_PERGAUSS_BWD, ST_SORT_COMPOSITE_FWD, ST_COUNT };
// "sort_composite_fwd": the fused launch (sort + forward of every tile of up to 1024 instances); "tile_sort" and
// "composite_fwd" then only hold the tier launches of longer lists, or the whole passes when the fused launch does not apply
const char* const kStageNames[ST_COUNT] = {"preprocess", "tile_scan", "tile_sort", "composite_fwd",
                                           "loss_fwd", "loss_bwd", "zero_acc", "composite_bwd", "pergauss_bwd",
                                           "sort_composite_fwd"};
// roctx ranges per stage: resolved lazily from the ROCm tools library, only when asked for
// (GSR_ROCTX=1 in the environment, or gsr_profile_enable(h, 2 | ...)); rocprofv3 --marker-trace then
// slices the kernel trace by stage without kernel-name matching.
struct Roctx {
    typedef int (*push_fn)(const char*);
    typedef int (*pop_fn)(void);
    push_fn push = nullptr;
    pop_fn pop = nullptr;
    bool tried = false;
    bool load() {
        if (tried) return push != nullptr;
        tried = true;
        const char* names[] = {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"};
        for (const char* n : names) {
            void* lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (!lib) continue;
            push = (push_fn)dlsym(lib, "roctxRangePushA");
            pop = (pop_fn)dlsym(lib, "roctxRangePop");
            if (push && pop) return true;
            push = nullptr; pop = nullptr;
        }
        return false;
    }
};
Roctx g_roctx;
bool roctx_env() {
    static const bool on = [] { const char* e = getenv("GSR_ROCTX"); return e && e[0] == '1'; }();
    return on;
}

struct Profiler {
    bool on = false;      // HIP-event timing per stage
    bool ranges = false;  // roctx range per stage
    bool in_range = false;
    bool rec_open = false;
    uint32_t mask = ~0u;  // stages that get an event pair (gsr_profile_stages)
    struct Rec { int stage; hipEvent_t a, b; bool extra; };  // extra: a second launch group of a stage inside ONE call (time, not count)
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        // timing-only events: no system-scope fence (cache write-back + invalidate) when the marker retires — the bubble an
        // event record leaves between two kernels is what the timed region pays for its one profiled stage
        (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
        return e;
    }
    void begin(int stage, hipStream_t s, bool extra = false);
    void end(hipStream_t s) {
        if (in_range) { g_roctx.pop(); in_range = false; }
        if (!rec_open) return;
        rec_open = false;
        (void)hipEventRecord(recs.back().b, s);
    }
    // error path: a stage that was begun but whose launch failed — close the roctx range and DROP the half-recorded
    // pair (its end event was never recorded: gsr_profile_read would fail or mis-time on it)
    void abort() {
        if (in_range) { g_roctx.pop(); in_range = false; }
        if (!rec_open) return;
        rec_open = false;
        pool.push_back(recs.back().a);
        pool.push_back(recs.back().b);
        recs.pop_back();
    }
    void clear() {
        for (auto& r : recs) { pool.push_back(r.a); pool.push_back(r.b); }
        recs.clear();
    }
    void destroy() {
        clear();
        for (auto e : pool) (void)hipEventDestroy(e);
        pool.clear();
    }
};

void Profiler::begin(int stage, hipStream_t s, bool extra) {
    if ((ranges || roctx_env()) && g_roctx.load()) {
        char name[48];
        snprintf(name, sizeof name, "gsr:%s", kStageNames[stage]);
        g_roctx.push(name);
        in_range = true;
    }
    if (!on || !((mask >> stage) & 1u)) return;
    Rec r{stage, get(), get(), extra};
    (void)hipEventRecord(r.a, s);
    recs.push_back(r);
    rec_open = true;
}

// One profiled stage: begun by the constructor, ended by close(); a scope left WITHOUT close() — an early `return rc`
// or a HIPCHK between the two — aborts the stage instead of leaving a pushed roctx range and an open record behind.
struct StageScope {
    Profiler& p;
    hipStream_t s;
    bool open = true;
    StageScope(Profiler& prof, int stage, hipStream_t stream, bool extra = false) : p(prof), s(stream) { p.begin(stage, s, extra); }
    void close() { if (open) { p.end(s); open = false; } }
    ~StageScope() { if (open) p.abort(); }
    StageScope(const StageScope&) = delete;
    StageScope& operator=(const StageScope&) = delete;
};

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

bool valid_mode(int m) { return m == GSR_MODE_RGB || m == GSR_MODE_RGBD || m == GSR_MODE_RGBDN; }

}  // namespace

struct gsr_handle {
    gsr_config cfg;
    int grid_x, grid_y, n_tiles;
    // ImageState (states.jl:99-111) + tile bookkeeping
    DevBuf ranges, n_contrib, final_T, tile_count, tile_start, tile_order, totals;
    // GeometryState (states.jl:2-47), repacked as one 64-byte record per Gaussian
    DevBuf geo, gnormal, radii, bsum, bpre, bvis;
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

    DevBuf* all[40];
    int n_all = 0;
    GuardDamage guard_damage;  // GSR_DEBUG_GUARD: the first damaged guard of any buffer of `all`, freed ones included
};

namespace {

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
GsrFrame frame_of(const gsr_handle* h, const float* background, float* image, const gsr_aux* aux) {
    return GsrFrame{background, image, h->n_contrib.as<uint32_t>(), h->final_T.as<float>(), h->values_sorted.as<uint32_t>(),
                    aux ? aux->covisibilities : nullptr, aux ? aux->uncertainties : nullptr};
}

// CPU relax hint inside the spin phase: x86 `pause`, AArch64 `yield`, nothing elsewhere (the host side builds on any arch).
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#endif
}

// Host wait policy of the forward's single read-back (gsr_host_wait_policy), process-wide.
//   DEFAULT (sleep_us == 0): spin for spin_us microseconds, then poll with sched_yield() between looks at the word.  Any
//   other runnable thread — RCCL's proxy threads on an 8-rank host — gets the core at once, no timer is involved, and
//   the step time is a pure spin's (config 2: 0.2123-0.2137 ms, config 3: 1.494 ms per step over 200 steps, all three
//   policies within noise of each other: tools/host_wait_ab.sh).
//   OPT-IN (sleep_us > 0): the thread SLEEPS through the expected wait (a running average of this handle's previous
//   waits: the host runs ahead of the GPU, so the wait is as long as the work still queued in front of the scan, about
//   the same every step) except for its last spin_us microseconds — in doubling pieces of 50, 100, 200 ... us with a look
//   at the word after each, so that the first forward after the caller synchronised (GPU idle: a short wait) costs one
//   small piece; a wake-up that finds the word already written is not a sample (an average fed with its own oversleeps
//   ratchets upwards and starves the GPU) but shrinks the estimate; after the expected time + spin_us: sched_yield() for
//   yield_us, then sleeps of sleep_us.  Same step time on a quiet host, a fraction of the CPU time; NOT the default
//   because a late timer wake-up (observed on one box of the pool: one step of twenty 3 ms late) lands in the step time.
struct WaitPolicy { int spin_us = 30, yield_us = 0, sleep_us = 0; };
// the three values live in ONE atomic word (21 bits each): a forward on another thread reads the old or the new policy,
// never a mix of the two (round-4 verdict, weak #9)
constexpr int kWaitMaxUs = (1 << 21) - 1;
inline uint64_t pack_wait(const WaitPolicy& w) {
    return (uint64_t)w.spin_us | ((uint64_t)w.yield_us << 21) | ((uint64_t)w.sleep_us << 42);
}
std::atomic<uint64_t> g_wait_packed{pack_wait(WaitPolicy{})};
inline WaitPolicy load_wait() {
    const uint64_t v = g_wait_packed.load(std::memory_order_relaxed);
    WaitPolicy w;
    w.spin_us = (int)(v & kWaitMaxUs); w.yield_us = (int)((v >> 21) & kWaitMaxUs); w.sleep_us = (int)((v >> 42) & kWaitMaxUs);
    return w;
}

// gsr_ssim_precision: 0 = the contracted build of ssim.hip (default), 1 = its bit-exact twin.  GSR_SSIM_EXACT=1 in the
// environment starts a process in exact mode (A/B runs of unmodified callers).
// Process-wide DEFAULT only: a handle created with gsr_config.ssim_precision = 0 / 1 is pinned (ABI 5).
std::atomic<int> g_ssim_exact{[] { const char* e = getenv("GSR_SSIM_EXACT"); return e && e[0] == '1' ? 1 : 0; }()};
// gsr_preprocess_form: -1 by scene and grid size (default), 0 direct, 1 aggregating wherever its LDS fits; the same rule
std::atomic<int> g_preprocess_form{[] { const char* e = getenv("GSR_PREPROCESS_AGG"); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }()};
inline int ssim_exact_of(const gsr_handle* h) {
    return h->cfg.ssim_precision != GSR_DEFAULT ? (h->cfg.ssim_precision == GSR_SSIM_EXACT ? 1 : 0)
                                                : g_ssim_exact.load(std::memory_order_relaxed);
}
inline int preprocess_form_of(const gsr_handle* h) {  // -1 by scene and grid, 0 direct, 1 aggregating
    return h->cfg.preprocess_form != GSR_DEFAULT ? (h->cfg.preprocess_form == GSR_PREPROCESS_AGGREGATING ? 1 : 0)
                                                 : g_preprocess_form.load(std::memory_order_relaxed);
}

// Wait until tile_scan of forward `seq` has published its totals (a word of pinned host memory).
// A wait that lasts longer than any sane queue depth (50 ms) starts polling the stream, so that a failed launch or a
// faulted kernel ends with an error instead of hanging the caller — not earlier: hipStreamQuery puts a marker packet on
// the stream, and a marker between two kernels is a 5 us bubble (rocprofv3 kernel trace, tools/gap_report.py).
int wait_totals(gsr_handle* h, uint32_t seq, hipStream_t s) {
    using clk = std::chrono::steady_clock;
    volatile uint32_t* word = h->host_totals + GSR_TOTAL_SEQ;
    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return GSR_OK;
    const auto t0 = clk::now();
    const double expect_us = h->wait_ema_us;
    const WaitPolicy g_wait = load_wait();  // one consistent snapshot for this wait
    if (g_wait.sleep_us > 0 && expect_us > (double)g_wait.spin_us + 50.0) {  // sleeping enabled and worth it
        // ... in doubling pieces (50, 100, 200, ... us) with a look at the word after each: the expectation comes from
        // steps in which the host ran ahead of the GPU; the first forward after the caller synchronised finds the GPU
        // idle and its wait is only preprocess + scan long — the small first pieces bound what that costs.
        double remaining = expect_us - (double)g_wait.spin_us, piece = 50.0;
        while (remaining > 0.0) {
            const long ns = (long)((remaining < piece ? remaining : piece) * 1000.0);
            struct timespec ts = {ns / 1000000000L, ns % 1000000000L};
            nanosleep(&ts, nullptr);
            if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) {
                // Overslept (or woke exactly on time): how long the wait really was is unknown — only that it was no
                // longer than this.  NOT a sample of the average (an average fed with its own oversleeps ratchets upwards
                // and starves the GPU): the estimate shrinks instead, so that the next wake-up comes early enough to see
                // the word arrive.
                const double slept = std::chrono::duration<double, std::micro>(clk::now() - t0).count();
                h->wait_ema_us = 0.85 * (slept < expect_us ? slept : expect_us);
                return GSR_OK;
            }
            remaining = expect_us - (double)g_wait.spin_us - std::chrono::duration<double, std::micro>(clk::now() - t0).count();
            piece *= 2.0;
        }
    }
    const auto t_spin = t0 + std::chrono::microseconds((g_wait.sleep_us > 0 ? (long)expect_us : 0L) + g_wait.spin_us);
    const auto t_yield = t_spin + std::chrono::microseconds(g_wait.yield_us);
    auto next_poll = t0 + std::chrono::milliseconds(50);
    int rc = GSR_OK;
    for (;;) {
        bool done = false;
        for (int i = 0; i < 64 && !done; i++) {
            done = __atomic_load_n(word, __ATOMIC_ACQUIRE) == seq;
            if (!done) cpu_relax();
        }
        const auto now = clk::now();
        if (done) {
            const double us = std::chrono::duration<double, std::micro>(now - t0).count();
            h->wait_ema_us = h->wait_ema_us == 0.0 ? us : 0.75 * h->wait_ema_us + 0.25 * us;
            return GSR_OK;
        }
        if (now >= t_spin) {
            if (now < t_yield || g_wait.sleep_us <= 0) {
                sched_yield();
            } else {
                struct timespec ts = {0, (long)g_wait.sleep_us * 1000L};
                nanosleep(&ts, nullptr);
            }
        }
        if (now < next_poll) continue;
        next_poll = now + std::chrono::milliseconds(50);
        const hipError_t q = hipStreamQuery(s);
        if (q == hipSuccess) {  // everything enqueued has finished: the word is there, or it never will be
            if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return GSR_OK;
            rc = fail(GSR_E_HIP, "tile scan finished without publishing its totals");
            break;
        }
        if (q != hipErrorNotReady) { rc = fail(GSR_E_HIP, "HIP error while waiting for the tile scan: %s", hipGetErrorString(q)); break; }
    }
    h->wait_ema_us = 0.0;
    return rc;
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
    if (cfg->flags & ~(uint32_t)GSR_FLAG_REFERENCE_TILE_LISTS) return fail(GSR_E_INVALID_ARG, "unknown flags 0x%x", cfg->flags);
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
    // (8 192 tiles = 131 072 pixels wide: one row of the tile grid must fit the aggregating binning's LDS band, pergauss.hip)
    if (h->grid_x > 8192 || h->grid_y > 65535) { delete h; return fail(GSR_E_INVALID_ARG, "resolution too large"); }
    h->n_tiles = h->grid_x * h->grid_y;
    // the handle's policies: configuration (constructor fields, then the tuner's process default) and the view-history state
    gsr_policy_config_init(&h->pcfg, cfg->width, cfg->height, cfg->bins_budget_bytes, -1 /* resolved per view: process default */);
    gsr_policy_state_init(&h->pol);
    const char* tun = getenv("GSR_FORM_TUNER");  // the DEFAULT of handles that do not say (0 = off)
    h->pcfg.form_tuner = cfg->form_tuner == GSR_TUNER_ON ? 1 : cfg->form_tuner == GSR_TUNER_OFF ? 0 : !(tun && tun[0] == '0');
    DevBuf* list[] = {&h->ranges, &h->n_contrib, &h->final_T, &h->tile_count, &h->tile_start, &h->tile_order, &h->totals,
                      &h->geo, &h->gnormal, &h->radii, &h->bsum, &h->bpre, &h->bvis, &h->bins, &h->values_sorted, &h->s0,
                      &h->s1, &h->s2, &h->s3, &h->big_scratch, &h->rows, &h->vmean2d, &h->d0, &h->d1,
                      &h->d2, &h->partial, &h->keys_compact, &h->big_list, &h->long_state, &h->overflow_fill, &h->dbg_flag, &h->pose_part};
    static const char* const names[] = {"ranges", "n_contrib", "final_T", "tile_count", "tile_start", "tile_order", "totals",
                                        "geo", "gnormal", "radii", "bsum", "bpre", "bvis", "bins", "values_sorted", "s0",
                                        "s1", "s2", "s3", "big_scratch", "rows", "vmean2d", "d0", "d1",
                                        "d2", "partial", "keys_compact", "big_list", "long_state", "overflow_fill", "dbg_flag", "pose_part"};
    static_assert(sizeof(names) / sizeof(names[0]) == sizeof(list) / sizeof(list[0]), "one name per buffer");
    for (DevBuf* b : list) {
        b->name = names[h->n_all];
        b->damage = &h->guard_damage;
        h->all[h->n_all++] = b;
    }
    // GSR_DEBUG_GUARD words (DevBuf::guard_word): ids whose range may be {0} get 0
    h->tile_order.guard_word = 0u;     // tile ids
    h->big_list.guard_word = 0u;       // tile ids of the tier lists
    h->values_sorted.guard_word = 0u;  // Gaussian ids
    // GSR_DEBUG_FILL candidates (DevBuf::fill_ok), each read only as float data:
    h->rows.fill_ok = true;        // GsrInst gradient rows (float4): summed by pergauss_bwd, copied out by gsr_buffer
    h->vmean2d.fill_ok = true;     // gstate.∇means_2d (float2): written for every Gaussian, read by gsr_update_stats behind radii > 0
    h->final_T.fill_ok = true;     // final transmittance per pixel: a factor of the backward, never a bound (n_contrib is)
    h->gnormal.fill_ok = true;     // per-Gaussian normals (float4): feature values of the :rgbdn stream
    h->d0.fill_ok = true;          // SSIM loss head's ∂map/∂µ1 plane
    h->d1.fill_ok = true;          // ... ∂map/∂σ1²
    h->d2.fill_ok = true;          // ... ∂map/∂σ12
    h->partial.fill_ok = true;     // per-wave (Σ|x-y|, Σssim) pairs summed by the loss finisher
    h->pose_part.fill_ok = true;   // per-workgroup pose-gradient partials: every slot is stored (zeros included) before it is summed
    h->long_state.fill_ok = true;  // (T, A) float2 per pixel and segment of the long-list backward
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
    DevBuf* scene[] = {&h->geo, &h->gnormal, &h->radii, &h->bsum, &h->bpre, &h->bvis, &h->bins, &h->values_sorted, &h->s0, &h->s1,
                       &h->s2, &h->s3, &h->big_scratch, &h->rows, &h->vmean2d, &h->pose_part, &h->keys_compact};
    h->pol.bin_cap = 0;
    h->pol.compact_sticky = 0;
    for (DevBuf* b : scene) {
        int rc = b->release();
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
        const size_t nn = (size_t)n_gaussians, nb = (nn + 255) / 256 + 1;
        if ((rc = h->geo.ensure(nn * 64)) || (rc = h->radii.ensure(nn * 4)) || (rc = h->bsum.ensure(nb * 4)) ||
            (rc = h->bpre.ensure(nb * 4)) || (rc = h->bvis.ensure(nb * 4)) || (rc = h->vmean2d.ensure(nn * 8)) ||
            (rc = h->pose_part.ensure(gsr_pose_partial_floats(n_gaussians) * 4)) ||
            (C > 5 && (rc = h->gnormal.ensure(nn * 16))))
            return rc;
    }
    if (n_instances > 0) {
        const size_t D = (size_t)n_instances;
        // (the gradient rows are indexed by Gaussian-major SLOT: one per emitted tile of a small rect, one per tile of a large one —
        //  at most ~1.5 x the instance count under exact culling)
        if ((rc = h->values_sorted.ensure(D * 4)) || (rc = h->s0.ensure(D * 16)) || (rc = h->s1.ensure(D * 16)) ||
            (rc = h->s2.ensure(D * 16)) || (C > 3 && (rc = h->s3.ensure(D * 16))) || (rc = h->rows.ensure(D * 64 + D * 32)))
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
                     void* stream_v, gsr_stats* stats, FwdView& v) {
    int rc = check_inputs(h, in, cam);
    if (rc) return rc;
    if (!image_out) return fail(GSR_E_INVALID_ARG, "null image_out");
    if (aux && ((aux->flags & ~(uint32_t)GSR_FORWARD_ONLY) || aux->reserved))
        return fail(GSR_E_INVALID_ARG, "unknown gsr_aux.flags 0x%x / reserved 0x%x", aux->flags, aux->reserved);
    v.in = in; v.image_out = image_out; v.aux = aux; v.stats = stats;
    v.fwd_only = aux && (aux->flags & GSR_FORWARD_ONLY);
    v.s = (hipStream_t)stream_v;
    v.C = h->cfg.mode; v.n = in->n;
    h->fwd_valid = false;
    h->bwd_valid = false;
    h->inputs_consumed = false;
    h->dropped_by_reserve = false;
    h->fwd_only = v.fwd_only;

    const size_t nn = v.n > 0 ? (size_t)v.n : 1;
    const int n_blocks = (v.n + 255) / 256;
    const bool own_radii = !(aux && aux->radii);
    // per-Gaussian scratch: grow-only with 25 % slack, like the per-instance buffers below — a training run's densification
    // adds 5-15 % of Gaussians per round (strategy.jl:78-105), and an exact fit made EVERY round's first view reallocate all
    // five (five hipFree + hipMalloc = device synchronisations: the slowest plain steps of the round-6 training protocol)
    const float nslack = 1.25f;
    if ((rc = h->geo.ensure(nn * 64, nslack)) || (own_radii && (rc = h->radii.ensure(nn * 4, nslack))) ||
        (rc = h->bsum.ensure((size_t)(n_blocks + 1) * 4, nslack)) || (rc = h->bpre.ensure((size_t)(n_blocks + 1) * 4, nslack)) ||
        (rc = h->bvis.ensure((size_t)(n_blocks + 1) * 4, nslack)) || (v.C > 5 && (rc = h->gnormal.ensure(nn * 16, nslack))))
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
                                  frame_of(h, v.in->background, v.image_out, v.aux), (uint32_t)v.cap_instances,
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
                                         /*aggregating=*/v.plan.form != GSR_FORM_DIRECT);
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
    if ((rc = wait_totals(h, v.seq, v.s))) return rc;
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
    const uint64_t D = v.D;
    const float slack = 1.25f;  // instance count drifts slowly between training steps
    // forward-only and everything composited by the fused launch: no per-instance storage at all (the rare paths of
    // fwd_sort_and_walk — tier lists, compact binning — still hand their instances over through the stream)
    const bool need_stream = !(v.fwd_only && v.oc.fused_done && !v.oc.long_tiles);
    if (need_stream &&
        ((rc = h->values_sorted.ensure(D * 4, slack)) ||
         (rc = h->s0.ensure(D * 16, slack)) || (rc = h->s1.ensure(D * 16, slack)) ||
         (rc = h->s2.ensure(D * 16, slack)) || (v.C > 3 && (rc = h->s3.ensure(D * 16, slack)))))
        return rc;
    if (!v.fwd_only && (rc = h->rows.ensure(v.D_slots * 64, slack))) return rc;
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
    gsr_launch_composite_fwd(ws, v.C, v.k, tiles_of(h), stream_of(h), frame_of(h, v.in->background, v.image_out, v.aux),
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
    FwdView v;
    int rc;
    if ((rc = fwd_begin(h, in, cam, image_out, aux, stream_v, stats, v))) return rc;
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
static int launch_composite_bwd(gsr_handle* h, hipStream_t s, int C, const GsrCam& k, const float* background,
                                const float* vpixels, bool color_only) {
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
    gsr_launch_composite_bwd(s, C, k, tiles_of(h), stream_of(h), frame, vpixels, inst_of(h), tiers.split_len, color_only, accurate);
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
static int composite_bwd_stage(gsr_handle* h, hipStream_t s, const gsr_inputs* in, const gsr_camera* cam, const float* vpixels,
                               float* vmeans2d, uint32_t flags, GsrCam* k) {
    int rc;
    if (!vmeans2d && (rc = h->vmean2d.ensure((size_t)in->n * 8, 1.25f))) return rc;
    h->vmean2d_cur = vmeans2d ? reinterpret_cast<float2*>(vmeans2d) : h->vmean2d.as<float2>();
    const bool color_only = (flags & GSR_GRADS_COLOR_COTANGENT) != 0u;
    if (color_only && (rc = check_color_cotangent(h, vpixels, s))) return rc;
    *k = make_cam(h, cam);
    StageScope sc(h->prof, ST_COMPOSITE_BWD, s);
    if (h->last_D > 0 && (rc = launch_composite_bwd(h, s, h->cfg.mode, *k, in->background, vpixels, color_only))) return rc;
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
    if (g->vR && (rc = h->pose_part.ensure(gsr_pose_partial_floats(n) * 4, 1.25f))) return rc;
    GsrCam k;
    if ((rc = composite_bwd_stage(h, s, in, cam, vpixels, g->vmeans2d, g->flags, &k))) return rc;
    StageScope sc8(h->prof, ST_PERGAUSS_BWD, s);
    gsr_launch_pergauss_bwd(s, n, in->n_coeffs, in->sh_degree, C, in->means, in->scales, in->rotations, in->shs, k,
                            geom_of(h), inst_of(h), h->vmean2d_cur, g->vmeans, g->vshs, g->vopacities,
                            g->vscales, g->vrotations, g->vR, g->vt, h->pose_part.as<float>(), g->vcolors,
                            /*fp32_chain=*/h->cfg.grad_precision == GSR_GRAD_FP32_REFERENCE);
    sc8.close();
    HIPCHK(hipGetLastError());
    h->bwd_valid = true;
    return GSR_OK;
}

static int buffer_lookup(const gsr_handle* h, int which, const void** dev_ptr, size_t* bytes) {
    const size_t n = (size_t)h->last_n, P = (size_t)h->cfg.width * h->cfg.height, T = (size_t)h->n_tiles;
    const size_t D = (size_t)h->last_D;
    const DevBuf* b = nullptr;
    size_t sz = 0;
    switch (which) {
        case GSR_BUF_RADII:  // handle-owned, or the caller's gsr_aux.radii of the last forward
            *dev_ptr = h->fwd_valid && n ? h->radii_cur : nullptr;
            *bytes = *dev_ptr ? n * 4 : 0;
            return GSR_OK;
        case GSR_BUF_GRAD_MEANS2D:
            *dev_ptr = h->bwd_valid && n ? h->vmean2d_cur : nullptr;
            *bytes = *dev_ptr ? n * 8 : 0;
            return GSR_OK;
        case GSR_BUF_N_CONTRIB: b = &h->n_contrib; sz = P * 4; break;
        case GSR_BUF_FINAL_T: b = &h->final_T; sz = P * 4; break;
        case GSR_BUF_TILE_RANGES: b = &h->ranges; sz = 2 * T * 4; break;
        case GSR_BUF_VALUES_SORTED: b = &h->values_sorted; sz = h->fwd_only ? 0 : D * 4; break;
        case GSR_BUF_GEOM: b = &h->geo; sz = n * 64; break;
        case GSR_BUF_NORMALS: b = &h->gnormal; sz = h->cfg.mode > 5 ? n * 16 : 0; break;
        case GSR_BUF_GRAD_ROWS: b = &h->rows; sz = (size_t)h->last_slots * 16 * GSR_ROW_F4(h->cfg.mode); break;
        case GSR_BUF_INSTANCE_AUX: b = &h->s2; sz = h->fwd_only ? 0 : D * 16; break;
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

int gsr_ssim_forward(int W, int H, int CH, int B, const float* img, const float* ref, float C1, float C2, int train,
                     float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream) {
    if (W <= 0 || H <= 0 || CH <= 0 || B <= 0) return fail(GSR_E_INVALID_ARG, "bad SSIM shape");
    if (!img || !ref || !ssim_map) return fail(GSR_E_INVALID_ARG, "null SSIM array");
    if (train && (!dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12)) return fail(GSR_E_INVALID_ARG, "train needs the 3 partial maps");
    if ((size_t)CH * B > 65535) return fail(GSR_E_INVALID_ARG, "CH*B too large");
    if ((size_t)W * H > 0xFFFFFFFFull) return fail(GSR_E_INVALID_ARG, "SSIM plane too large");  // 32-bit offsets inside a plane
    (g_ssim_exact.load(std::memory_order_relaxed) ? gsr_launch_ssim_fwd_exact : gsr_launch_ssim_fwd_fast)((hipStream_t)stream, W, H, CH, B, img, ref, C1, C2, train,
                                                                          ssim_map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_ssim_backward(int W, int H, int CH, int B, const float* img, const float* ref, const float* dL_dmap,
                      const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg,
                      void* stream) {
    if (W <= 0 || H <= 0 || CH <= 0 || B <= 0) return fail(GSR_E_INVALID_ARG, "bad SSIM shape");
    if (!img || !ref || !dL_dmap || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg)
        return fail(GSR_E_INVALID_ARG, "null SSIM array");
    if ((size_t)CH * B > 65535) return fail(GSR_E_INVALID_ARG, "CH*B too large");
    if ((size_t)W * H > 0xFFFFFFFFull) return fail(GSR_E_INVALID_ARG, "SSIM plane too large");  // 32-bit offsets inside a plane
    (g_ssim_exact.load(std::memory_order_relaxed) ? gsr_launch_ssim_bwd_exact : gsr_launch_ssim_bwd_fast)((hipStream_t)stream, W, H, CH, B, img, ref, dL_dmap, dm_dmu1,
                                                                          dm_dsigma1_sq, dm_dsigma12, dL_dimg);
    HIPCHK(hipGetLastError());
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

int gsr_prologue_forward(int32_t n, int32_t k_rest, int32_t scale_dims, const float* sh_color,
                         const float* sh_remainder, const float* opacities, const float* scales, float* shs,
                         float* opacities_act, float* scales_act, void* stream) {
    if (n < 0 || k_rest < 0 || (scale_dims != 1 && scale_dims != 3))
        return fail(GSR_E_INVALID_ARG, "bad sizes: n=%d k_rest=%d scale_dims=%d", n, k_rest, scale_dims);
    if (n == 0) return GSR_OK;
    if (!sh_color || (k_rest > 0 && !sh_remainder) || !opacities || !scales || !shs || !opacities_act || !scales_act)
        return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_prologue_fwd((hipStream_t)stream, n, k_rest, scale_dims, sh_color, sh_remainder, opacities, scales, shs,
                            opacities_act, scales_act);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_prologue_backward(int32_t n, int32_t k_rest, int32_t scale_dims, const float* opacities_act,
                          const float* scales_act, const float* vshs, const float* vopacities_act,
                          const float* vscales_act, float* v_sh_color, float* v_sh_remainder, float* v_opacities,
                          float* v_scales, void* stream) {
    if (n < 0 || k_rest < 0 || (scale_dims != 1 && scale_dims != 3))
        return fail(GSR_E_INVALID_ARG, "bad sizes: n=%d k_rest=%d scale_dims=%d", n, k_rest, scale_dims);
    if (n == 0) return GSR_OK;
    if (!opacities_act || !scales_act || !vshs || !vopacities_act || !vscales_act || !v_sh_color ||
        (k_rest > 0 && !v_sh_remainder) || !v_opacities || !v_scales)
        return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_prologue_bwd((hipStream_t)stream, n, k_rest, scale_dims, opacities_act, scales_act, vshs, vopacities_act,
                            vscales_act, v_sh_color, v_sh_remainder, v_opacities, v_scales);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

// Adam's step size with both debiasing factors folded in (Kingma & Ba §2); current_step counts from 1
static float adam_lr_t(float lr, float beta1, float beta2, uint32_t current_step) {
    const float t = (float)current_step;
    return lr * sqrtf(1.0f - powf(beta2, t)) / (1.0f - powf(beta1, t));
}

// lr_t of the trainer's six groups, after checking their arrays and counters; rest_empty: the scene has no features_rest
// (group 2), whose arrays are then not looked at (training.jl:770)
static int tail_lr_t(float* const theta[6], float* const mu[6], float* const nu[6], const float lr[6],
                     const uint32_t current_step[6], float beta1, float beta2, bool rest_empty, float lr_t[6]) {
    for (int g = 0; g < 6; g++) {
        if (g == 2 && rest_empty) { lr_t[g] = 0.0f; continue; }
        if (!theta[g] || !mu[g] || !nu[g]) return fail(GSR_E_INVALID_ARG, "group %d: null array", g);
        if (current_step[g] == 0) return fail(GSR_E_INVALID_ARG, "group %d: current_step counts from 1", g);
        lr_t[g] = adam_lr_t(lr[g], beta1, beta2, current_step[g]);
    }
    return GSR_OK;
}

int gsr_adam_step(const gsr_adam_group* groups, int32_t n_groups, float beta1, float beta2, float eps, void* stream) {
    if (n_groups < 0 || n_groups > GSR_ADAM_MAX_GROUPS || (n_groups > 0 && !groups))
        return fail(GSR_E_INVALID_ARG, "n_groups must be in [0, %d]", GSR_ADAM_MAX_GROUPS);
    float* theta[GSR_ADAM_MAX_GROUPS]; const float* grad[GSR_ADAM_MAX_GROUPS];
    float* mu[GSR_ADAM_MAX_GROUPS]; float* nu[GSR_ADAM_MAX_GROUPS];
    long long count[GSR_ADAM_MAX_GROUPS]; float lr_t[GSR_ADAM_MAX_GROUPS];
    int m = 0;
    for (int g = 0; g < n_groups; g++) {
        const gsr_adam_group& a = groups[g];
        if (a.count < 0) return fail(GSR_E_INVALID_ARG, "group %d: negative count", g);
        if (a.count == 0) continue;  // training.jl:770 `isempty(θᵢ) && continue`
        if (!a.theta || !a.grad || !a.mu || !a.nu) return fail(GSR_E_INVALID_ARG, "group %d: null array", g);
        if (a.current_step == 0) return fail(GSR_E_INVALID_ARG, "group %d: current_step counts from 1", g);
        theta[m] = a.theta; grad[m] = a.grad; mu[m] = a.mu; nu[m] = a.nu; count[m] = a.count;
        lr_t[m] = adam_lr_t(a.lr, beta1, beta2, a.current_step);
        m++;
    }
    if (m == 0) return GSR_OK;
    gsr_launch_adam((hipStream_t)stream, m, theta, grad, mu, nu, count, lr_t, beta1, beta2, eps);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_trainer_tail_step(int32_t n, int32_t k_rest, int32_t scale_dims, const gsr_tail_grads* grads,
                          float* const theta[6], float* const mu[6], float* const nu[6], const float lr[6],
                          const uint32_t current_step[6], float beta1, float beta2, float eps, float* shs,
                          float* opacities_act, float* scales_act, void* stream) {
    if (n < 0 || k_rest < 0 || (scale_dims != 1 && scale_dims != 3))
        return fail(GSR_E_INVALID_ARG, "bad sizes: n=%d k_rest=%d scale_dims=%d", n, k_rest, scale_dims);
    if (n == 0) return GSR_OK;
    if (!grads || !theta || !mu || !nu || !lr || !current_step || !shs || !opacities_act || !scales_act)
        return fail(GSR_E_INVALID_ARG, "null argument");
    if (!grads->vmeans || !grads->vshs || !grads->vopacities || !grads->vscales || !grads->vrotations)
        return fail(GSR_E_INVALID_ARG, "null gradient");
    float lr_t[6];
    int rc = tail_lr_t(theta, mu, nu, lr, current_step, beta1, beta2, /*rest_empty=*/k_rest == 0, lr_t);
    if (rc) return rc;
    const float* gr[5] = {grads->vmeans, grads->vshs, grads->vopacities, grads->vscales, grads->vrotations};
    gsr_launch_trainer_tail((hipStream_t)stream, n, k_rest, scale_dims, gr, theta, mu, nu, lr_t, beta1, beta2, eps, shs,
                            opacities_act, scales_act);
    HIPCHK(hipGetLastError());
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
    if ((rc = composite_bwd_stage(h, s, in, cam, vpixels, st->vmeans2d, st->flags, &k))) return rc;
    StageScope sc12(h->prof, ST_PERGAUSS_BWD, s);
    const gsr::TailState S = gsr_make_tail_state(st->theta, st->mu, st->nu, lr_t, st->beta1, st->beta2, st->eps,
                                                 st->scale_dims, st->shs, st->opacities_act, st->scales_act);
    gsr_launch_pergauss_bwd_tail(s, n, K, in->sh_degree, C, k, geom_of(h), inst_of(h), h->vmean2d_cur, S,
                                 /*fp32_chain=*/h->cfg.grad_precision == GSR_GRAD_FP32_REFERENCE);
    sc12.close();
    HIPCHK(hipGetLastError());
    h->bwd_valid = true;
    // the forward's inputs no longer exist (updated in place): a second backward on this forward would differentiate
    // the wrong parameters (the forward's own outputs — radii, tile lists, image — stay readable)
    h->inputs_consumed = true;
    return GSR_OK;
}

size_t gsr_mask_findall_scratch_bytes(int64_t n) { return n > 0 ? gsr_findall_scratch_bytes(n) : sizeof(uint32_t); }

int gsr_mask_findall(const uint8_t* mask, int64_t n, uint32_t* indices, uint32_t* count_out, void* scratch,
                     void* stream) {
    if (n < 0 || n > 0xFFFFFFFFll) return fail(GSR_E_INVALID_ARG, "n out of range");
    if (!count_out || (n > 0 && (!mask || !indices || !scratch))) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_findall((hipStream_t)stream, n, mask, indices, count_out, (uint32_t*)scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_gather_rows(const gsr_gather_group* groups, int32_t n_groups, const uint32_t* indices, int64_t count,
                    void* stream) {
    if (n_groups < 0 || n_groups > GSR_ADAM_MAX_GROUPS || (n_groups > 0 && !groups))
        return fail(GSR_E_INVALID_ARG, "n_groups must be in [0, %d]", GSR_ADAM_MAX_GROUPS);
    if (count < 0) return fail(GSR_E_INVALID_ARG, "negative count");
    if (count == 0 || n_groups == 0) return GSR_OK;
    if (!indices) return fail(GSR_E_INVALID_ARG, "null indices");
    const void* src[GSR_ADAM_MAX_GROUPS]; void* dst[GSR_ADAM_MAX_GROUPS]; int rw[GSR_ADAM_MAX_GROUPS];
    int m = 0;
    for (int g = 0; g < n_groups; g++) {
        if (groups[g].row_words < 0) return fail(GSR_E_INVALID_ARG, "group %d: negative row_words", g);
        if (groups[g].row_words == 0) continue;  // e.g. an empty features_rest (densification.jl:40-41)
        if (!groups[g].src || !groups[g].dst) return fail(GSR_E_INVALID_ARG, "group %d: null array", g);
        src[m] = groups[g].src; dst[m] = groups[g].dst; rw[m] = groups[g].row_words; m++;
    }
    if (m == 0) return GSR_OK;
    gsr_launch_gather_rows((hipStream_t)stream, m, src, dst, rw, indices, count);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

// ---- bilateral grid (bilateral.hip; src/bilateral_grid.jl) ----
namespace {
constexpr int kBilateralMaxGz = 64;         // LDS of the pullback: gz x 4 waves x 48 floats
constexpr int kBilateralMaxSlab = 16384;    // floats of one (image, coefficient) slab staged in LDS by the TV passes

int check_bilateral_grid(int32_t gx, int32_t gy, int32_t gz) {
    if (gx < 1 || gy < 1 || gz < 1) return fail(GSR_E_INVALID_ARG, "grid size (%d, %d, %d): every side must be >= 1", gx, gy, gz);
    if (gz > kBilateralMaxGz) return fail(GSR_E_INVALID_ARG, "grid size (%d, %d, %d): gz must be <= %d", gx, gy, gz, kBilateralMaxGz);
    if ((int64_t)gx * gy * gz > kBilateralMaxSlab)
        return fail(GSR_E_INVALID_ARG, "grid size (%d, %d, %d): gx*gy*gz must be <= %d", gx, gy, gz, kBilateralMaxSlab);
    return GSR_OK;
}
int check_bilateral_image(int32_t W, int32_t H, int32_t C) {
    if (W < 1 || H < 1 || (int64_t)W * H > 0x7FFFFFFF) return fail(GSR_E_INVALID_ARG, "image size %d x %d", W, H);
    if (C != 3 && C != 5 && C != 8) return fail(GSR_E_INVALID_ARG, "C = %d: the image has 3, 5 or 8 channels", C);
    return GSR_OK;
}
// the constants of the TV prior, once, on the host: the standalone TV and the fused tail read the same floats
gsr::BilateralTv bilateral_tv_consts(int32_t n, int32_t gx, int32_t gy, int32_t gz, float weight) {
    gsr::BilateralTv tv;
    tv.weight = weight;
    tv.nx = (float)std::max<int64_t>(1, (int64_t)(gx - 1) * gy * gz);   // bilateral_grid.jl:115-117
    tv.ny = (float)std::max<int64_t>(1, (int64_t)gx * (gy - 1) * gz);
    tv.nz = (float)std::max<int64_t>(1, (int64_t)gx * gy * (gz - 1));
    tv.n12 = 12.0f * (float)n;
    tv.rx = 2.0f / (tv.nx * tv.n12);
    tv.ry = 2.0f / (tv.ny * tv.n12);
    tv.rz = 2.0f / (tv.nz * tv.n12);
    return tv;
}
}  // namespace

size_t gsr_bilateral_scratch_bytes(int32_t W, int32_t H, int32_t gx, int32_t gy, int32_t gz) {
    if (W < 1 || H < 1 || gx < 1 || gy < 1 || gz < 1) return 0;
    return gsr_bilateral_partial_bytes(W, H, gx, gy, gz);
}

size_t gsr_bilateral_tv_scratch_bytes(int32_t n_images) {
    return n_images < 1 ? 0 : (size_t)n_images * 12 * 3 * sizeof(float);
}

int gsr_bilateral_slice_forward(int32_t W, int32_t H, int32_t C, const float* image, const float* grid, int32_t gx,
                                int32_t gy, int32_t gz, float* out, void* stream) {
    int rc;
    if ((rc = check_bilateral_image(W, H, C)) || (rc = check_bilateral_grid(gx, gy, gz))) return rc;
    if (!image || !grid || !out) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_bilateral_fwd((hipStream_t)stream, W, H, C, image, grid, gx, gy, gz, out);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_bilateral_slice_backward(int32_t W, int32_t H, int32_t C, const float* image, const float* grid, int32_t gx,
                                 int32_t gy, int32_t gz, const float* vout, float* vimage, float* vgrid, void* scratch,
                                 size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_bilateral_image(W, H, C)) || (rc = check_bilateral_grid(gx, gy, gz))) return rc;
    if (!image || !grid || !vout || !vimage || !vgrid || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    const size_t need = gsr_bilateral_scratch_bytes(W, H, gx, gy, gz);
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "scratch of %zu bytes, the pullback needs %zu", scratch_bytes, need);
    gsr_launch_bilateral_bwd((hipStream_t)stream, W, H, C, image, grid, gx, gy, gz, vout, vimage, vgrid, (float*)scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_bilateral_tv(int32_t n_images, int32_t gx, int32_t gy, int32_t gz, const float* grids, float weight,
                     float* loss_out, float* grad_out, void* scratch, size_t scratch_bytes, void* stream) {
    int rc;
    if (n_images < 1) return fail(GSR_E_INVALID_ARG, "n_images = %d", n_images);
    if ((rc = check_bilateral_grid(gx, gy, gz))) return rc;
    if (!grids || !loss_out || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    const size_t need = gsr_bilateral_tv_scratch_bytes(n_images);
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "scratch of %zu bytes, the TV needs %zu", scratch_bytes, need);
    gsr_launch_bilateral_tv((hipStream_t)stream, n_images, gx, gy, gz, grids, bilateral_tv_consts(n_images, gx, gy, gz, weight),
                            loss_out, grad_out, (float*)scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_bilateral_adam_tail(int32_t n_images, int32_t gx, int32_t gy, int32_t gz, float* grids, float* mu, float* nu,
                            const float* vgrid_view, int32_t view, float tv_weight, float lr, uint32_t current_step,
                            float beta1, float beta2, float eps, float* tv_loss_out, void* scratch, size_t scratch_bytes,
                            void* stream) {
    int rc;
    if (n_images < 1) return fail(GSR_E_INVALID_ARG, "n_images = %d", n_images);
    if ((rc = check_bilateral_grid(gx, gy, gz))) return rc;
    if (view < 0 || view >= n_images) return fail(GSR_E_INVALID_ARG, "view %d of %d images", view, n_images);
    if (!grids || !mu || !nu || !vgrid_view || !tv_loss_out || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    if (current_step == 0) return fail(GSR_E_INVALID_ARG, "current_step counts from 1");
    const size_t need = gsr_bilateral_tv_scratch_bytes(n_images);
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "scratch of %zu bytes, the tail needs %zu", scratch_bytes, need);
    const float lr_t = adam_lr_t(lr, beta1, beta2, current_step);
    const gsr::AdamHyper h{lr_t, beta1, beta2, 1.0f - beta1, 1.0f - beta2, eps};
    gsr_launch_bilateral_adam_tail((hipStream_t)stream, n_images, gx, gy, gz, grids, mu, nu, vgrid_view, view,
                                   bilateral_tv_consts(n_images, gx, gy, gz, tv_weight), h, tv_loss_out, (float*)scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

// ---- geometry regularisation (geometry.hip; src/geometry_regularization.jl) ----
namespace {
int check_normal_loss_frame(int32_t W, int32_t H, int32_t C) {
    if (W < 1 || H < 1 || (int64_t)W * H > 0x7FFFFFFF / 8) return fail(GSR_E_INVALID_ARG, "image size %d x %d", W, H);
    if (C != 8) return fail(GSR_E_INVALID_ARG, "C = %d: the depth-normal loss reads a :rgbdn frame (8 channels)", C);
    return GSR_OK;
}
int check_normal_loss_camera(const gsr_camera* cam) {
    if (!cam) return fail(GSR_E_INVALID_ARG, "null camera");
    if (!(cam->focal[0] > 0.0f) || !(cam->focal[1] > 0.0f)) return fail(GSR_E_INVALID_ARG, "focal lengths must be positive");
    return GSR_OK;
}
}  // namespace

size_t gsr_normal_loss_scratch_bytes(int32_t W, int32_t H) {
    if (W < 1 || H < 1) return 0;
    return gsr_normal_loss_scratch_floats(W, H) * sizeof(float);
}

int gsr_normal_loss_forward(int32_t W, int32_t H, int32_t C, const float* image, const gsr_camera* cam, float weight,
                            float* loss_out, float* stats_out, float* weights_out, void* scratch, size_t scratch_bytes,
                            void* stream) {
    int rc;
    if ((rc = check_normal_loss_frame(W, H, C)) || (rc = check_normal_loss_camera(cam))) return rc;
    if (!image || !loss_out || !stats_out || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    const size_t need = gsr_normal_loss_scratch_bytes(W, H);
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "scratch of %zu bytes, the depth-normal loss needs %zu", scratch_bytes, need);
    gsr_launch_normal_loss_fwd((hipStream_t)stream, W, H, image, cam->focal, cam->principal, weight, loss_out, stats_out,
                               weights_out, (float*)scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_normal_loss_backward(int32_t W, int32_t H, int32_t C, const float* image, const gsr_camera* cam, float weight,
                             float* vpixels, const void* scratch, size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_normal_loss_frame(W, H, C)) || (rc = check_normal_loss_camera(cam))) return rc;
    if (!image || !vpixels || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    if (image == vpixels) return fail(GSR_E_INVALID_ARG, "vpixels must not be the image");
    const size_t need = gsr_normal_loss_scratch_bytes(W, H);
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "scratch of %zu bytes, the depth-normal loss needs %zu", scratch_bytes, need);
    gsr_launch_normal_loss_bwd((hipStream_t)stream, W, H, image, cam->focal, cam->principal, weight, vpixels,
                               (const float*)scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

size_t gsr_flatten_loss_scratch_bytes(int32_t n) { return gsr_flatten_loss_scratch_floats(n) * sizeof(float); }

int gsr_flatten_loss(int32_t n, int32_t scale_dims, const float* scales_raw, float weight, float* loss_out, float* vscales,
                     void* scratch, size_t scratch_bytes, void* stream) {
    if (n < 0) return fail(GSR_E_INVALID_ARG, "negative n");
    if (scale_dims != 1 && scale_dims != 3) return fail(GSR_E_INVALID_ARG, "scale_dims = %d: 1 (isotropic) or 3", scale_dims);
    if (!loss_out || (n > 0 && (!scales_raw || !scratch))) return fail(GSR_E_INVALID_ARG, "null array");
    const size_t need = gsr_flatten_loss_scratch_bytes(n);
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "scratch of %zu bytes, the flatten loss needs %zu", scratch_bytes, need);
    gsr_launch_flatten_loss((hipStream_t)stream, n, scale_dims, scales_raw, weight, loss_out, vscales, (float*)scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

// ---- anchored depth supervision (depth.hip; src/depth_supervision.jl) ----
namespace {
int check_depth_loss_args(int32_t W, int32_t H, int32_t C, const gsr_depth_anchor* anchor, float qstep) {
    if (W < 1 || H < 1 || (int64_t)W * H > 0x7FFFFFFF / 8) return fail(GSR_E_INVALID_ARG, "image size %d x %d", W, H);
    if (C != 5 && C != 8) return fail(GSR_E_INVALID_ARG, "C = %d: the depth loss reads a :rgbd (5) or :rgbdn (8) frame", C);
    if (!anchor) return fail(GSR_E_INVALID_ARG, "null anchor");
    if (!std::isfinite(anchor->a) || !std::isfinite(anchor->b) || !(anchor->floor > 0.0f) || !std::isfinite(anchor->floor) ||
        !(anchor->p_far >= 0.0f) || !std::isfinite(anchor->p_far))
        return fail(GSR_E_INVALID_ARG, "anchor: a and b must be finite, floor > 0, p_far >= 0");
    if (!(qstep >= 0.0f) || !std::isfinite(qstep)) return fail(GSR_E_INVALID_ARG, "qstep must be finite and >= 0");
    return GSR_OK;
}
}  // namespace

size_t gsr_depth_loss_scratch_bytes(int32_t W, int32_t H) {
    if (W < 1 || H < 1) return 0;
    return gsr_depth_loss_scratch_size(W, H);
}

int gsr_depth_target(int32_t W, int32_t H, const float* prior, const gsr_depth_anchor* anchor, float qstep, float* target_out,
                     float* half_band_out, uint8_t* flags_out, void* stream) {
    int rc;
    if ((rc = check_depth_loss_args(W, H, 5, anchor, qstep))) return rc;
    if (!prior) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_depth_target((hipStream_t)stream, W, H, prior, &anchor->a, qstep, target_out, half_band_out, flags_out);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_depth_loss_forward(int32_t W, int32_t H, int32_t C, const float* image, const float* prior, const gsr_depth_anchor* anchor,
                           float qstep, float lambda_grad, float weight, float* loss_out, float* stats_out, float* target_out,
                           float* half_band_out, uint8_t* flags_out, void* scratch, size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_depth_loss_args(W, H, C, anchor, qstep))) return rc;
    if (!image || !prior || !loss_out || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    if ((uintptr_t)scratch % 16) return fail(GSR_E_INVALID_ARG, "scratch must be 16-byte aligned");
    const size_t need = gsr_depth_loss_scratch_bytes(W, H);
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "scratch of %zu bytes, the depth loss needs %zu", scratch_bytes, need);
    gsr_launch_depth_loss_fwd((hipStream_t)stream, W, H, C, image, prior, &anchor->a, qstep, lambda_grad, weight, loss_out,
                              stats_out, target_out, half_band_out, flags_out, scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_depth_loss_backward(int32_t W, int32_t H, int32_t C, const float* image, const float* prior, const gsr_depth_anchor* anchor,
                            float qstep, float lambda_grad, float weight, float* vpixels, const void* scratch, size_t scratch_bytes,
                            void* stream) {
    int rc;
    if ((rc = check_depth_loss_args(W, H, C, anchor, qstep))) return rc;
    if (!image || !prior || !vpixels || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    if (image == vpixels) return fail(GSR_E_INVALID_ARG, "vpixels must not be the image");
    if ((uintptr_t)scratch % 16) return fail(GSR_E_INVALID_ARG, "scratch must be 16-byte aligned");
    const size_t need = gsr_depth_loss_scratch_bytes(W, H);
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "scratch of %zu bytes, the depth loss needs %zu", scratch_bytes, need);
    // prior, anchor and qstep are the forward's: what they determine per pixel is in the records the forward left in scratch
    gsr_launch_depth_loss_bwd((hipStream_t)stream, W, H, C, image, lambda_grad, weight, vpixels, scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

// ---- sky dome: composite, sky-mask loss and their pullback (sky.hip; src/sky_dome.jl) ----
namespace {
int check_sky_args(int32_t W, int32_t H, int32_t C, const void* image, const void* sky_rgb) {
    if (W < 1 || H < 1 || (int64_t)W * H > 0x7FFFFFFF / 8) return fail(GSR_E_INVALID_ARG, "image size %d x %d", W, H);
    if (C != 5 && C != 8)
        return fail(GSR_E_INVALID_ARG, "C = %d: the sky composite reads the alpha row of a :rgbd (5) or :rgbdn (8) frame", C);
    if (!image || !sky_rgb) return fail(GSR_E_INVALID_ARG, "null array");
    return GSR_OK;
}
}  // namespace

size_t gsr_sky_scratch_bytes(int32_t W, int32_t H) {
    if (W < 1 || H < 1) return 0;
    return gsr_sky_scratch_size(W, H);
}

int gsr_sky_composite_forward(int32_t W, int32_t H, int32_t C, const float* image, const float* sky_rgb, const float* sky_weight,
                              float loss_weight, float* out, float* loss_out, void* scratch, void* stream) {
    int rc;
    if ((rc = check_sky_args(W, H, C, image, sky_rgb))) return rc;
    if (!out) return fail(GSR_E_INVALID_ARG, "null array");
    if (sky_weight && (!loss_out || !scratch)) return fail(GSR_E_INVALID_ARG, "a sky mask needs loss_out and scratch");
    if (sky_weight && (uintptr_t)scratch % 8) return fail(GSR_E_INVALID_ARG, "scratch must be 8-byte aligned");
    gsr_launch_sky_composite_fwd((hipStream_t)stream, W, H, C, image, sky_rgb, sky_weight, loss_weight, out, loss_out, scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_sky_composite_backward(int32_t W, int32_t H, int32_t C, const float* image, const float* sky_rgb, const float* sky_weight,
                               float loss_weight, float* vpixels, float* vsky, const void* scratch, void* stream) {
    int rc;
    if ((rc = check_sky_args(W, H, C, image, sky_rgb))) return rc;
    if (!vpixels || !vsky) return fail(GSR_E_INVALID_ARG, "null array");
    if (image == vpixels) return fail(GSR_E_INVALID_ARG, "vpixels must not be the image");
    if (sky_weight && !scratch) return fail(GSR_E_INVALID_ARG, "a sky mask needs the scratch its forward filled");
    if (sky_weight && (uintptr_t)scratch % 8) return fail(GSR_E_INVALID_ARG, "scratch must be 8-byte aligned");
    gsr_launch_sky_composite_bwd((hipStream_t)stream, W, H, C, image, sky_rgb, sky_weight, loss_weight, vpixels, vsky, scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

// ---- evaluation head: 8-bit SSIM / MSE / PSNR / L1 and the RGB8 export (eval.hip; training.jl:487-532) ----
namespace {
int check_eval_frame(int32_t W, int32_t H, int32_t C, const void* image, const void* sky_rgb) {
    if (W < 1 || H < 1) return fail(GSR_E_INVALID_ARG, "image size %d x %d", W, H);
    if (C < 3) return fail(GSR_E_INVALID_ARG, "C = %d: a frame has at least the 3 colour channels", C);
    if (sky_rgb && C < 5) return fail(GSR_E_INVALID_ARG, "C = %d: a sky frame needs the alpha row of a :rgbd / :rgbdn frame (C >= 5)", C);
    // 32-bit element offsets inside the frame, 32-bit byte offsets inside a row
    if ((uint64_t)W * (uint64_t)H * (uint64_t)C > 0xFFFFFFFFull || (uint64_t)W * (uint64_t)C * 4 > 0xFFFFFFFFull)
        return fail(GSR_E_INVALID_ARG, "frame too large: %d x %d x %d is 2^32 elements or more", C, W, H);
    if (!image) return fail(GSR_E_INVALID_ARG, "null image");
    return GSR_OK;
}
}  // namespace

size_t gsr_eval_scratch_bytes(int32_t W, int32_t H) {
    if (W < 1 || H < 1) return 0;
    return gsr_eval_scratch_size(W, H);
}

int gsr_eval_metrics(int32_t W, int32_t H, int32_t C, const float* image, const float* sky_rgb, const float* target_f32,
                     const uint8_t* target_u8, int32_t quantize, float* ssim_map, float* out, void* scratch, void* stream) {
    int rc;
    if ((rc = check_eval_frame(W, H, C, image, sky_rgb))) return rc;
    if (!out || !scratch) return fail(GSR_E_INVALID_ARG, "null out or scratch");
    if ((target_f32 != nullptr) == (target_u8 != nullptr))
        return fail(GSR_E_INVALID_ARG, "exactly one of target_f32 and target_u8: %s given", target_f32 ? "both" : "neither");
    if (ssim_map == image) return fail(GSR_E_INVALID_ARG, "ssim_map must not be the image");
    if ((uintptr_t)scratch % 8) return fail(GSR_E_INVALID_ARG, "scratch must be 8-byte aligned");
    gsr_launch_eval_metrics((hipStream_t)stream, W, H, C, image, sky_rgb, target_f32, target_u8, quantize != 0, ssim_map, out,
                            scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_frame_rgb8(int32_t W, int32_t H, int32_t C, const float* image, const float* sky_rgb, int32_t flip_rows,
                   uint8_t* rgb8_out, void* stream) {
    int rc;
    if ((rc = check_eval_frame(W, H, C, image, sky_rgb))) return rc;
    if (!rgb8_out) return fail(GSR_E_INVALID_ARG, "null rgb8_out");
    gsr_launch_frame_rgb8((hipStream_t)stream, W, H, C, image, sky_rgb, flip_rows != 0, rgb8_out);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_densify_grad_mean(int64_t n, const float* accum, const float* denom, float* grad_out, void* stream) {
    if (n < 0) return fail(GSR_E_INVALID_ARG, "negative n");
    if (n == 0) return GSR_OK;
    if (!accum || !denom || !grad_out) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_grad_mean((hipStream_t)stream, n, accum, denom, grad_out);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_densify_mask(int32_t kind, int64_t n, int64_t n_grad, const float* grad, const float* scales, int32_t scale_dims,
                     const float* opacities, const int32_t* max_radii, float grad_threshold, float gamma, float min_opacity,
                     int32_t max_screen_size, uint8_t* mask, void* stream) {
    if (kind < GSR_DENSIFY_CLONE || kind > GSR_DENSIFY_PRUNE) return fail(GSR_E_INVALID_ARG, "unknown mask kind %d", kind);
    if (n < 0 || n_grad < 0 || n_grad > n) return fail(GSR_E_INVALID_ARG, "bad sizes: n=%lld n_grad=%lld", (long long)n, (long long)n_grad);
    if (scale_dims != 1 && scale_dims != 3) return fail(GSR_E_INVALID_ARG, "scale_dims must be 1 or 3");
    if (n == 0) return GSR_OK;
    if (!mask) return fail(GSR_E_INVALID_ARG, "null mask");
    if (kind != GSR_DENSIFY_PRUNE && (!scales || (n_grad > 0 && !grad))) return fail(GSR_E_INVALID_ARG, "null array");
    if (kind == GSR_DENSIFY_PRUNE && (!opacities || (max_screen_size > 0 && (!max_radii || !scales))))
        return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_densify_mask((hipStream_t)stream, kind, n, n_grad, grad, scales, scale_dims, opacities, max_radii, grad_threshold,
                            gamma, min_opacity, max_screen_size, mask);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_compose_rows(const gsr_compose_group* groups, int32_t n_groups, const uint32_t* keep_idx, int64_t n_keep,
                     const uint32_t* sel_idx, int64_t n_sel, int32_t reps, void* stream) {
    if (n_groups < 0 || n_groups > GSR_COMPOSE_MAX_GROUPS || (n_groups > 0 && !groups))
        return fail(GSR_E_INVALID_ARG, "n_groups must be in [0, %d]", GSR_COMPOSE_MAX_GROUPS);
    if (n_keep < 0 || n_sel < 0 || reps < 0) return fail(GSR_E_INVALID_ARG, "negative count");
    if (n_sel > 0 && reps > 0 && !sel_idx) return fail(GSR_E_INVALID_ARG, "null sel_idx");
    if (n_keep + n_sel * reps == 0 || n_groups == 0) return GSR_OK;
    const void* src[GSR_COMPOSE_MAX_GROUPS]; void* dst[GSR_COMPOSE_MAX_GROUPS];
    int rw[GSR_COMPOSE_MAX_GROUPS], nz[GSR_COMPOSE_MAX_GROUPS];
    int m = 0;
    for (int g = 0; g < n_groups; g++) {
        if (groups[g].row_words < 0) return fail(GSR_E_INVALID_ARG, "group %d: negative row_words", g);
        if (groups[g].row_words == 0) continue;  // an empty features_rest (densification.jl:40-41,196-201)
        if (!groups[g].dst || (!groups[g].src && (n_keep > 0 || !groups[g].new_zero)))
            return fail(GSR_E_INVALID_ARG, "group %d: null array", g);
        src[m] = groups[g].src; dst[m] = groups[g].dst; rw[m] = groups[g].row_words; nz[m] = groups[g].new_zero ? 1 : 0; m++;
    }
    if (m == 0) return GSR_OK;
    gsr_launch_compose_rows((hipStream_t)stream, m, src, dst, rw, nz, keep_idx, n_keep, sel_idx, reps > 0 ? n_sel : 0, reps > 0 ? reps : 1);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_split_transform(int64_t n_new, int32_t scale_dims, float* points, const float* rotations, float* scales, uint32_t seed,
                        void* stream) {
    if (n_new < 0 || (scale_dims != 1 && scale_dims != 3)) return fail(GSR_E_INVALID_ARG, "bad sizes");
    if (n_new == 0) return GSR_OK;  // densification.jl:94 `if n_new_points > 0`
    if (!points || !rotations || !scales) return fail(GSR_E_INVALID_ARG, "null array");
    if (((uintptr_t)rotations & 15) != 0) return fail(GSR_E_INVALID_ARG, "rotations must be 16-byte aligned");
    gsr_launch_split_transform((hipStream_t)stream, n_new, scale_dims, points, rotations, scales, seed);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_reset_opacity(int64_t n, float* opacities, void* stream) {
    if (n < 0) return fail(GSR_E_INVALID_ARG, "negative n");
    if (n == 0) return GSR_OK;
    if (!opacities) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_reset_opacity((hipStream_t)stream, n, opacities);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

// ---- the MCMC strategy (mcmc.hip; src/mcmc.jl) ----
static int check_mcmc_rows(int64_t n, int32_t scale_dims) {
    if (n < 0) return fail(GSR_E_INVALID_ARG, "negative n");
    if (scale_dims != 1 && scale_dims != 3) return fail(GSR_E_INVALID_ARG, "scale_dims = %d: 1 (isotropic) or 3", scale_dims);
    return GSR_OK;
}

int gsr_mcmc_weights(int64_t n, int32_t scale_dims, const float* opacities_raw, const float* scales_raw, float min_opacity,
                     float log_max_scale, uint32_t* q, uint8_t* dead, void* stream) {
    int rc;
    if ((rc = check_mcmc_rows(n, scale_dims))) return rc;
    if (n == 0) return GSR_OK;
    if (!opacities_raw || !q || (dead && !scales_raw)) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_mcmc_weights((hipStream_t)stream, n, scale_dims, opacities_raw, scales_raw, min_opacity, log_max_scale, q, dead);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

size_t gsr_mcmc_sample_scratch_bytes(int64_t n) { return gsr_mcmc_sample_scratch_words(n) * sizeof(uint64_t); }

int gsr_mcmc_sample(int64_t n, const uint32_t* q, int64_t m, uint32_t seed, uint32_t* sampled, int32_t* counts, uint64_t* total,
                    void* scratch, size_t scratch_bytes, void* stream) {
    if (n < 0 || m < 0) return fail(GSR_E_INVALID_ARG, "negative count: n=%lld m=%lld", (long long)n, (long long)m);
    if (n > 0xFFFFFFFFll || m > 0xFFFFFFFFll) return fail(GSR_E_INVALID_ARG, "rows and draws are indexed with 32 bits");
    if (m == 0) return GSR_OK;
    if (!total) return fail(GSR_E_INVALID_ARG, "null total");
    if (n > 0 && (!q || !sampled || !counts || !scratch)) return fail(GSR_E_INVALID_ARG, "null array");
    const size_t need = gsr_mcmc_sample_scratch_bytes(n);
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "scratch of %zu bytes, the sampler needs %zu", scratch_bytes, need);
    if ((((uintptr_t)scratch | (uintptr_t)total) & 7) != 0) return fail(GSR_E_INVALID_ARG, "scratch and total must be 8-byte aligned");
    gsr_launch_mcmc_sample((hipStream_t)stream, n, q, m, seed, sampled, counts, reinterpret_cast<unsigned long long*>(total),
                           reinterpret_cast<unsigned long long*>(scratch));
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_mcmc_split_sampled(int64_t n, int32_t scale_dims, const int32_t* counts, const float* binoms, int32_t n_max,
                           float min_opacity, float* opacities_raw, float* scales_raw, void* stream) {
    int rc;
    if ((rc = check_mcmc_rows(n, scale_dims))) return rc;
    if (n_max < 1) return fail(GSR_E_INVALID_ARG, "n_max = %d: at least 1", n_max);
    if (n == 0) return GSR_OK;
    if (!counts || !binoms || !opacities_raw || !scales_raw) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_mcmc_split_sampled((hipStream_t)stream, n, scale_dims, counts, binoms, n_max, min_opacity, opacities_raw, scales_raw);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_mcmc_relocation_params(int64_t m, const float* o, const int32_t* ratio, const float* binoms, int32_t n_max,
                               float min_opacity, float* new_o, float* coeff, void* stream) {
    if (m < 0) return fail(GSR_E_INVALID_ARG, "negative m");
    if (n_max < 1) return fail(GSR_E_INVALID_ARG, "n_max = %d: at least 1", n_max);
    if (m == 0) return GSR_OK;
    if (!o || !ratio || !binoms || !new_o || !coeff) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_mcmc_relocation_params((hipStream_t)stream, m, o, ratio, binoms, n_max, min_opacity, new_o, coeff);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_mcmc_relocate_rows(const gsr_compose_group* groups, int32_t n_groups, int64_t n, const uint32_t* dead_idx,
                           const uint32_t* sampled_idx, int64_t m, void* stream) {
    if (n_groups < 0 || n_groups > GSR_COMPOSE_MAX_GROUPS || (n_groups > 0 && !groups))
        return fail(GSR_E_INVALID_ARG, "n_groups must be in [0, %d]", GSR_COMPOSE_MAX_GROUPS);
    if (n < 0 || m < 0) return fail(GSR_E_INVALID_ARG, "negative count");
    if (m == 0 || n == 0 || n_groups == 0) return GSR_OK;
    if (!dead_idx || !sampled_idx) return fail(GSR_E_INVALID_ARG, "null index vector");
    void* x[GSR_COMPOSE_MAX_GROUPS];
    int rw[GSR_COMPOSE_MAX_GROUPS], nz[GSR_COMPOSE_MAX_GROUPS];
    int k = 0;
    for (int g = 0; g < n_groups; g++) {
        if (groups[g].row_words < 0) return fail(GSR_E_INVALID_ARG, "group %d: negative row_words", g);
        if (groups[g].row_words == 0) continue;  // an empty features_rest
        if (!groups[g].dst) return fail(GSR_E_INVALID_ARG, "group %d: null array", g);
        if (groups[g].src && groups[g].src != groups[g].dst) return fail(GSR_E_INVALID_ARG, "group %d: the relocation is in place (src must be NULL or dst)", g);
        x[k] = groups[g].dst; rw[k] = groups[g].row_words; nz[k] = groups[g].new_zero ? 1 : 0; k++;
    }
    if (k == 0) return GSR_OK;
    gsr_launch_mcmc_relocate_rows((hipStream_t)stream, k, x, rw, nz, n, dead_idx, sampled_idx, m);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_mcmc_inject_noise(int64_t n, int32_t scale_dims, float* points, const float* opacities_raw, const float* scales_raw,
                          const float* rotations, float lr, float max_kick, uint32_t seed, void* stream) {
    int rc;
    if ((rc = check_mcmc_rows(n, scale_dims))) return rc;
    if (n == 0) return GSR_OK;  // mcmc.jl:292
    if (!points || !opacities_raw || !scales_raw || !rotations) return fail(GSR_E_INVALID_ARG, "null array");
    if (((uintptr_t)rotations & 15) != 0) return fail(GSR_E_INVALID_ARG, "rotations must be 16-byte aligned");
    gsr_launch_mcmc_inject_noise((hipStream_t)stream, n, scale_dims, points, opacities_raw, scales_raw, rotations, lr, max_kick, seed);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

size_t gsr_mcmc_regularization_scratch_bytes(int64_t n) { return gsr_mcmc_regularization_scratch_floats(n) * sizeof(float); }

int gsr_mcmc_regularization(int64_t n, int32_t scale_dims, const float* opacities_raw, const float* scales_raw, float opacity_reg,
                            float scale_reg, float* loss_out, float* vopacities, float* vscales, void* scratch,
                            size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_mcmc_rows(n, scale_dims))) return rc;
    if (!loss_out || (n > 0 && (!opacities_raw || !scales_raw || !scratch))) return fail(GSR_E_INVALID_ARG, "null array");
    const size_t need = gsr_mcmc_regularization_scratch_bytes(n);
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "scratch of %zu bytes, the regulariser needs %zu", scratch_bytes, need);
    gsr_launch_mcmc_regularization((hipStream_t)stream, n, scale_dims, opacities_raw, scales_raw, opacity_reg, scale_reg, loss_out,
                                   vopacities, vscales, (float*)scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_morton_codes(int64_t n, const float* points, const float* box_lo, const float* box_hi, uint64_t* codes, void* stream) {
    if (n < 0) return fail(GSR_E_INVALID_ARG, "negative n");
    if (n == 0) return GSR_OK;
    if (!points || !box_lo || !box_hi || !codes) return fail(GSR_E_INVALID_ARG, "null array");
    float inv[3];
    for (int k = 0; k < 3; k++) {
        const float e = box_hi[k] - box_lo[k];
        if (!(e >= 0.0f)) return fail(GSR_E_INVALID_ARG, "gsr_morton_codes: box_hi < box_lo (or NaN)");
        inv[k] = e > 0.0f ? 1.0f / e : 0.0f;
    }
    gsr_launch_morton_codes((hipStream_t)stream, n, points, box_lo, inv, reinterpret_cast<unsigned long long*>(codes));
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

// ---- a model from a point cloud: exact 3-NN initial scales (knn.hip; dataset.jl:236-249 `compute_scales`) ----
size_t gsr_knn_scratch_bytes(int64_t n) {
    if (n <= 0 || n > 0x7FFFFFFFll) return 0;
    return gsr_knn_scratch_size(n);
}

int gsr_knn_scales(int64_t n, const float* points, const int32_t* order, float point_size, int32_t scale_dims, float* scales_out,
                   float* dist2_out, void* scratch, size_t scratch_bytes, void* stream) {
    if (n < 0) return fail(GSR_E_INVALID_ARG, "gsr_knn_scales: negative n");
    if (n == 0) return GSR_OK;
    if (n <= 3)  // the reference's knn(kdtree, xyz, 3 + 1) throws there
        return fail(GSR_E_INVALID_ARG, "gsr_knn_scales: n = %lld: three neighbours need at least 4 points", (long long)n);
    if (n > 0x7FFFFFFFll) return fail(GSR_E_INVALID_ARG, "gsr_knn_scales: n = %lld: rows are indexed with 31 bits", (long long)n);
    if (scale_dims != 1 && scale_dims != 3) return fail(GSR_E_INVALID_ARG, "gsr_knn_scales: scale_dims = %d: 1 (isotropic) or 3", scale_dims);
    if (!(point_size > 0.0f)) return fail(GSR_E_INVALID_ARG, "gsr_knn_scales: point_size = %g must be positive", (double)point_size);
    if (!points || !scales_out || !scratch) return fail(GSR_E_INVALID_ARG, "gsr_knn_scales: null points, scales_out or scratch");
    const size_t need = gsr_knn_scratch_bytes(n);
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "gsr_knn_scales: scratch_bytes = %zu, the search needs %zu", scratch_bytes, need);
    if ((uintptr_t)scratch % 16) return fail(GSR_E_INVALID_ARG, "gsr_knn_scales: scratch must be 16-byte aligned");
    gsr_launch_knn_scales((hipStream_t)stream, n, points, order, point_size, scale_dims, scales_out, dist2_out, scratch);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_count_nonfinite(const float* const* arrays, const int32_t* row_words, int32_t n_groups, int64_t n_rows, uint32_t* counts,
                        uint32_t* first_bad, void* stream) {
    if (n_groups < 0 || n_groups > GSR_ADAM_MAX_GROUPS || (n_groups > 0 && (!arrays || !row_words)))
        return fail(GSR_E_INVALID_ARG, "n_groups must be in [0, %d]", GSR_ADAM_MAX_GROUPS);
    if (n_rows < 0) return fail(GSR_E_INVALID_ARG, "negative n_rows");
    if (n_groups == 0) return GSR_OK;
    if (!counts || !first_bad) return fail(GSR_E_INVALID_ARG, "null output");
    const float* src[GSR_ADAM_MAX_GROUPS]; int rw[GSR_ADAM_MAX_GROUPS];
    for (int g = 0; g < n_groups; g++) {
        if (row_words[g] < 0) return fail(GSR_E_INVALID_ARG, "group %d: negative row_words", g);
        if (row_words[g] > 0 && n_rows > 0 && !arrays[g]) return fail(GSR_E_INVALID_ARG, "group %d: null array", g);
        src[g] = arrays[g]; rw[g] = row_words[g];
    }
    gsr_launch_nonfinite_scan((hipStream_t)stream, n_groups, src, rw, n_rows, counts, first_bad);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

static int ply_rows(bool pack, int64_t n, int32_t k_rest, const float* points, const float* dc, const float* rest,
                    const float* opac, const float* scales, const float* rots, const float* rows, void* stream) {
    if (n < 0 || k_rest < 0) return fail(GSR_E_INVALID_ARG, "bad sizes: n=%lld k_rest=%d", (long long)n, k_rest);
    if (n == 0) return GSR_OK;
    if (!points || !dc || (k_rest > 0 && !rest) || !opac || !scales || !rots || !rows) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_ply_rows((hipStream_t)stream, pack, n, k_rest, const_cast<float*>(points), const_cast<float*>(dc),
                        const_cast<float*>(rest), const_cast<float*>(opac), const_cast<float*>(scales), const_cast<float*>(rots),
                        const_cast<float*>(rows));
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_ply_pack_rows(int64_t n, int32_t k_rest, const float* points, const float* features_dc, const float* features_rest,
                      const float* opacities, const float* scales, const float* rotations, float* rows, void* stream) {
    return ply_rows(true, n, k_rest, points, features_dc, features_rest, opacities, scales, rotations, rows, stream);
}

int gsr_ply_unpack_rows(int64_t n, int32_t k_rest, const float* rows, float* points, float* features_dc, float* features_rest,
                        float* opacities, float* scales, float* rotations, void* stream) {
    return ply_rows(false, n, k_rest, points, features_dc, features_rest, opacities, scales, rotations, rows, stream);
}

int gsr_sh_grad_from_views(int32_t n, int32_t n_coeffs, int32_t sh_degree, int32_t n_views, const float* camera_centers,
                           const float* means, const float* vcolors_all, float* vshs, void* stream) {
    if (n < 0 || n_views < 1 || sh_degree < 0 || sh_degree > 3 || n_coeffs < (sh_degree + 1) * (sh_degree + 1))
        return fail(GSR_E_INVALID_ARG, "bad sizes: n=%d views=%d degree=%d K=%d", n, n_views, sh_degree, n_coeffs);
    if (n == 0) return GSR_OK;
    if (!camera_centers || !means || !vcolors_all || !vshs) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_sh_grad_views((hipStream_t)stream, n, n_coeffs, sh_degree, n_views, camera_centers, means, vcolors_all, vshs);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_sh_grad_from_views_tail(int32_t n, int32_t n_coeffs, int32_t sh_degree, int32_t n_views, const float* camera_centers,
                                const float* vcolors_all, const gsr_tail_grads* small, const gsr_tail_state* st, void* stream) {
    if (n < 0 || n_views < 1 || sh_degree < 0 || sh_degree > 3 || n_coeffs < (sh_degree + 1) * (sh_degree + 1) || n_coeffs > 16)
        return fail(GSR_E_INVALID_ARG, "bad sizes: n=%d views=%d degree=%d K=%d", n, n_views, sh_degree, n_coeffs);
    if (n == 0) return GSR_OK;
    if (!camera_centers || !vcolors_all || !small || !st) return fail(GSR_E_INVALID_ARG, "null argument");
    if (!small->vmeans || !small->vopacities || !small->vscales || !small->vrotations)
        return fail(GSR_E_INVALID_ARG, "null gradient (vmeans / vopacities / vscales / vrotations; vshs is not read)");
    if (st->scale_dims != 1 && st->scale_dims != 3) return fail(GSR_E_INVALID_ARG, "scale_dims must be 1 or 3");
    if (!st->shs || !st->opacities_act || !st->scales_act) return fail(GSR_E_INVALID_ARG, "null activated copy");
    float lr_t[6];
    int rc = tail_lr_t(st->theta, st->mu, st->nu, st->lr, st->current_step, st->beta1, st->beta2, /*rest_empty=*/n_coeffs == 1, lr_t);
    if (rc) return rc;
    const gsr::TailState S = gsr_make_tail_state(st->theta, st->mu, st->nu, lr_t, st->beta1, st->beta2, st->eps,
                                                 st->scale_dims, st->shs, st->opacities_act, st->scales_act);
    gsr_launch_sh_views_tail((hipStream_t)stream, n, n_coeffs, sh_degree, n_views, camera_centers, vcolors_all, small->vmeans,
                             small->vopacities, small->vscales, small->vrotations, S);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_stream_triad(float* a, const float* b, const float* c, size_t count, float q, void* stream) {
    if (!a || !b || !c) return fail(GSR_E_INVALID_ARG, "null array");
    if (count % 4 != 0 || (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) != 0)
        return fail(GSR_E_INVALID_ARG, "count must be a multiple of 4 and the arrays 16-byte aligned");
    gsr_launch_triad((hipStream_t)stream, count / 4, a, b, c, q);
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

int gsr_allreduce_grads(void* nccl_comm, float* arena, size_t count, void* stream) {
    typedef int (*allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
    static allreduce_fn fn = nullptr;
    if (!nccl_comm || !arena) return fail(GSR_E_INVALID_ARG, "null communicator / arena");
    if (!fn) {
        void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) return fail(GSR_E_HIP, "cannot load librccl.so: %s", dlerror());
        fn = (allreduce_fn)dlsym(lib, "ncclAllReduce");
        if (!fn) return fail(GSR_E_HIP, "ncclAllReduce not found in librccl.so");
    }
    const int ncclFloat32 = 7, ncclSum = 0;
    int r = fn(arena, arena, count, ncclFloat32, ncclSum, nccl_comm, (hipStream_t)stream);
    if (r != 0) return fail(GSR_E_HIP, "ncclAllReduce failed with code %d", r);
    return GSR_OK;
}

}  // extern "C"
