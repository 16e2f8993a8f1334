// Optional per-stage timing with HIP events on the caller's stream (gsr_profile_*), and roctx ranges per stage.
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace gsr_host {

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
inline Roctx g_roctx;
inline bool roctx_env() {
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

inline void Profiler::begin(int stage, hipStream_t s, bool extra) {
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

}  // namespace gsr_host
