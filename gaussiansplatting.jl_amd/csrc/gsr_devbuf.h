// The handle's device buffers: grow-only allocations (DevBuf) and the two debugging aids every allocation consults, the fill of
// fresh float buffers (GSR_DEBUG_FILL) and the guard behind each buffer (GSR_DEBUG_GUARD).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gsr_host.h"

namespace gsr_host {

// GSR_DEBUG_FILL=nan | big (debugging, read at every allocation): each new allocation of a buffer marked `fill_ok` is filled
// with the 32-bit word 0xFFFFFFFF (a NaN) or 0x7F7F7F7F (3.4e38, finite: NaN hides behind comparisons), so that a kernel
// that reads a float it never wrote shows up in the result instead of reading the zeros of fresh pages.  0 = unset.
inline uint32_t debug_fill_word() {
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
inline bool debug_guard_on() {
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
    // allocation (gsr_api.cpp's table of the handle's buffers; index / key / count / mask buffers never are: garbage there is a wild address)
    bool fill_ok = false;
    // GSR_DEBUG_GUARD: the name the check reports; whether THIS allocation carries a guard; the word of a buffer that is not
    // fill_ok (those get 0x7F7F7F7F).  By the rule above an index / count buffer's guard holds a small valid value: 1 — one
    // instance, offset 1, tile-list range [1, 1), radius 1, a 64-bit key of tile 0 — and unlike 0 it differs from what a
    // stray clear would leave.  The three buffers whose words are ids that need not have a second element (tile ids of a
    // one-tile image, Gaussian ids of a one-Gaussian scene) get 0 (the same table).
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

}  // namespace gsr_host
