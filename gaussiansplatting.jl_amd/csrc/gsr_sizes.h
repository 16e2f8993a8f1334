// Byte sizes of the handle's per-Gaussian and per-instance buffers, written once: gsr_reserve, the forward, the backward and
// gsr_buffer all take them from here, so that a reserve sizes exactly what the next view asks for.  Plain host C++ (no HIP
// header): tests/test_sizes.py builds it with g++ alone.  Slack is not part of a size: it is an argument of DevBuf::ensure.
#pragma once
#include <cstddef>
#include <cstdint>

struct gsr_gaussian_bytes {
    size_t geo;        // one 64-byte record per Gaussian
    size_t radii;      // int32
    size_t block;      // bsum, bpre, bvis — each: one word per block of 256 Gaussians, and one more
    size_t gnormal;    // float4, :rgbdn only
    size_t vmean2d;    // float2 (the backward's)
    size_t pose_part;  // the backward's pose-gradient partials
    size_t comp;       // float: add_blur's compensations, antialiased handles only
    size_t sh_jac;     // 9 floats: d rgb / d dir of the backward's row-independent job, :rgb only; grown by that backward, not by gsr_reserve
};

// n Gaussians in a C-channel mode; pose_partial_floats: pergauss.hip's gsr_pose_partial_floats(n).  The forward's arrays hold
// at least one element (a view of no Gaussian still launches over them).  antialiased: a GSR_FLAG_ANTIALIASED handle.
inline gsr_gaussian_bytes gsr_sizes_per_gaussian(size_t n, int C, size_t pose_partial_floats, bool antialiased = false) {
    const size_t nn = n > 0 ? n : 1;
    gsr_gaussian_bytes b;
    b.geo = nn * 64;
    b.radii = nn * 4;
    b.block = ((n + 255) / 256 + 1) * 4;
    b.gnormal = C > 5 ? nn * 16 : 0;
    b.vmean2d = n * 8;
    b.pose_part = pose_partial_floats * 4;
    b.comp = antialiased ? nn * 4 : 0;
    b.sh_jac = C == 3 ? n * 36 : 0;
    return b;
}

struct gsr_instance_bytes {
    size_t values_sorted;  // Gaussian id per instance
    size_t stream;         // s0, s1, s2 — each: one float4 per instance
    size_t s3;             // a fourth float4 in the modes beyond :rgb
    size_t rows;           // the backward's gradient rows: 64 bytes per SLOT
};

// D instances in D_slots gradient-row slots (Gaussian-major: one per emitted tile of a small rect, one per tile of a large one)
inline gsr_instance_bytes gsr_sizes_per_instance(uint64_t D, uint64_t D_slots, int C) {
    gsr_instance_bytes b;
    b.values_sorted = (size_t)D * 4;
    b.stream = (size_t)D * 16;
    b.s3 = C > 3 ? (size_t)D * 16 : 0;
    b.rows = (size_t)D_slots * 64;
    return b;
}

// ... as gsr_reserve sizes them before a view's slot count is known: at most ~1.5 slots per instance under exact culling.
// (the forward's expression at D_slots = 1.5 D, taken at 3 D and halved so that an odd D loses nothing: D * 96 exactly)
inline gsr_instance_bytes gsr_sizes_reserve_instances(uint64_t D, int C) {
    gsr_instance_bytes b = gsr_sizes_per_instance(D, 3 * D, C);
    b.rows /= 2;
    return b;
}
