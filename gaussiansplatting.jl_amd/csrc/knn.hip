// Initial scales of a model built from a point cloud: the EXACT three nearest neighbours of every point and the
// reference's scale from them (src/dataset.jl:236-249 `compute_scales`: KDTree, knn(…, 3 + 1), log of the root mean
// squared distance to the three that are not the point itself).  DESIGN.md §17.
//
// Two passes over a caller-given permutation `order` (a Morton order makes the cull effective; ANY permutation gives the
// same bits):
//   gather : slot p of the scratch receives point order[p] as float4 (x, y, z, row as bits); every 64 consecutive slots —
//            a GROUP — get one axis-aligned box.
//   search : one wave per group, one query per lane.  The wave scans its own group, then the other groups outward
//            (g-1, g+1, g-2, …), 64 candidate groups per step: lane l tests candidate l's box against the wave's box and
//            the wave's largest third-best distance, a ballot turns the survivors into a work list (composite.hip's
//            pattern), and a surviving group's points are read at wave-uniform addresses.
//            Before a survivor is visited every lane tests its own point against the box: a visit costs 64 such tests.
// Exactness of the cull: the box-to-box (and point-to-box) lower bound is the fp32 expression of d2 itself — (dx*dx + dy*dy) + dz*dz, no
// contraction (-ffp-contract=off) — on clamped per-axis gaps.  For a query q of the wave's box and a point p of the
// candidate's box, |q.x - p.x| >= gap.x in the reals, fp32 subtraction, multiplication and addition are monotone, hence
// bound <= d2(q, p) in fp32; a group is skipped only when bound >= every lane's third-best, where no point of it could
// replace anything (a candidate replaces only if d2 < third-best).  With every distance 0 everything is culled.
// Every loop's trip count is fixed by n (the work list's by its 64 bits); no float atomics: one lane owns one output row.
#include "gsr_kernels.h"

namespace {

constexpr int KNN_GROUP = 64;  // points per group = lanes per wave

__device__ __forceinline__ float wave_min_all(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float wave_max_all(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

__device__ __forceinline__ bool finite_(float v) { return fabsf(v) <= 3.4028234664e38f; }

// boxes: six arrays of G floats — lo.x, lo.y, lo.z, hi.x, hi.y, hi.z.  fminf / fmaxf drop a NaN coordinate; a group of
// nothing but NaNs keeps lo = +inf, hi = -inf, whose bound against anything is +inf: never visited.
__global__ __launch_bounds__(256) void knn_gather_kernel(long long n, int G, const float* __restrict__ points,
                                                         const int32_t* __restrict__ order, float4* __restrict__ pts,
                                                         float* __restrict__ boxes) {
    const int lane = threadIdx.x & 63;
    const int g = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (g >= G) return;  // (whole waves leave: no barrier below)
    const long long p = (long long)g * KNN_GROUP + lane;
    const float inf = __builtin_inff();
    float lx = inf, ly = inf, lz = inf, hx = -inf, hy = -inf, hz = -inf;
    if (p < n) {
        long long j = order ? (long long)order[p] : p;
        j = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);  // a bad permutation gives wrong numbers, never a read outside `points`
        const float x = points[3 * j], y = points[3 * j + 1], z = points[3 * j + 2];
        pts[p] = make_float4(x, y, z, __int_as_float((int)j));
        lx = hx = x; ly = hy = y; lz = hz = z;
    }
    lx = wave_min_all(lx); ly = wave_min_all(ly); lz = wave_min_all(lz);
    hx = wave_max_all(hx); hy = wave_max_all(hy); hz = wave_max_all(hz);
    if (lane == 0) {
        boxes[g] = lx; boxes[(size_t)G + g] = ly; boxes[2 * (size_t)G + g] = lz;
        boxes[3 * (size_t)G + g] = hx; boxes[4 * (size_t)G + g] = hy; boxes[5 * (size_t)G + g] = hz;
    }
}

// The sorted triple b0 <= b1 <= b2 of a lane takes in d: m = min(d, b2) is never a NaN (a NaN d — a non-finite
// coordinate — is dropped there), and the three smallest of {b0, b1, b2, d} are those of {b0, b1, m}.
__device__ __forceinline__ void take(float d, float& b0, float& b1, float& b2) {
    const float m = fminf(d, b2);
    b2 = fmaxf(b1, m);
    b1 = fmaxf(b0, fminf(b1, m));
    b0 = fminf(b0, m);
}

// `cnt` points at a wave-uniform address against the lane's query.  SELF: the wave's own group, slot == lane is the
// query itself — excluded by INDEX, not by d2 > 0: a duplicate at distance 0 is a neighbour.
template <bool SELF>
__device__ __forceinline__ void visit_point(const float4 c, int k, int lane, float qx, float qy, float qz, float& b0, float& b1,
                                            float& b2) {
    const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
    float d = (dx * dx + dy * dy) + dz * dz;
    if (SELF) d = k == lane ? __builtin_inff() : d;
    take(d, b0, b1, b2);
}
// (eight points per trip: their loads — scalar, the address is the wave's — are issued together, not one wait per point;
// fetching the next eight under these measured 1-5 % slower: 106 SGPRs and a wait in the middle of the trip)
template <bool SELF>
__device__ __forceinline__ void visit_group(const float4* __restrict__ grp, int cnt, int lane, float qx, float qy, float qz,
                                            float& b0, float& b1, float& b2) {
    int k = 0;
    for (; k + 8 <= cnt; k += 8) {
        float4 c[8];
#pragma unroll
        for (int u = 0; u < 8; u++) c[u] = grp[k + u];
#pragma unroll
        for (int u = 0; u < 8; u++) visit_point<SELF>(c[u], k + u, lane, qx, qy, qz, b0, b1, b2);
    }
    for (; k < cnt; k++) visit_point<SELF>(grp[k], k, lane, qx, qy, qz, b0, b1, b2);
}

__global__ __launch_bounds__(256) void knn_search_kernel(long long n, int G, const float4* __restrict__ pts,
                                                         const float* __restrict__ boxes, float point_size, int scale_dims,
                                                         float* __restrict__ scales_out, float* __restrict__ dist2_out) {
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (g >= G) return;
    const long long p = (long long)g * KNN_GROUP + lane;
    const bool valid = p < n;
    const long long left = n - (long long)g * KNN_GROUP;
    const int cnt_g = left < KNN_GROUP ? (int)left : KNN_GROUP;
    const float inf = __builtin_inff();
    const float4 q = valid ? pts[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // a query with a non-finite coordinate (its row is unspecified) must not hold the wave's cull radius at +inf
    const bool active = valid && finite_(q.x) && finite_(q.y) && finite_(q.z);
    float b0 = inf, b1 = inf, b2 = inf;
    visit_group<true>(pts + (size_t)g * KNN_GROUP, cnt_g, lane, q.x, q.y, q.z, b0, b1, b2);

    const size_t sG = (size_t)G;
    const float wlx = boxes[g], wly = boxes[sG + g], wlz = boxes[2 * sG + g];
    const float whx = boxes[3 * sG + g], why = boxes[4 * sG + g], whz = boxes[5 * sG + g];
    // candidate m = 0, 1, 2, …  is group g-1, g+1, g-2, g+2, …; the farther end of the array is |offset| <= G-1 away
    const long long n_cand = 2 * ((long long)G - 1);
    for (long long m0 = 0; m0 < n_cand; m0 += 64) {
        const long long m = m0 + lane;
        const long long off = (m >> 1) + 1;
        const long long cl = (m & 1) ? (long long)g + off : (long long)g - off;
        const bool in = m < n_cand && cl >= 0 && cl < (long long)G;
        const int c = in ? (int)cl : g;
        const float gx = fmaxf(fmaxf(boxes[c] - whx, wlx - boxes[3 * sG + c]), 0.0f);
        const float gy = fmaxf(fmaxf(boxes[sG + c] - why, wly - boxes[4 * sG + c]), 0.0f);
        const float gz = fmaxf(fmaxf(boxes[2 * sG + c] - whz, wlz - boxes[5 * sG + c]), 0.0f);
        const float bound = (gx * gx + gy * gy) + gz * gz;
        const float wmax = wave_max_all(active ? b2 : 0.0f);
        unsigned long long wl = __builtin_amdgcn_ballot_w64(in && bound < wmax);
        for (int s = 0; s < 64 && wl != 0ull; s++) {
            const int j = __builtin_ctzll(wl);
            wl &= wl - 1;
            // the third-bests have shrunk since the ballot: test again, against every lane's own
            const float bc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bound), j));
            if (__builtin_amdgcn_ballot_w64(active && bc < b2) == 0ull) continue;
            const int cj = __builtin_amdgcn_readlane(c, j);
            // ... and each lane's own POINT against the box (the wave's box is wide where its points are sparse — the
            // far outliers of a cloud —, and a visit costs 64 of these tests): the same expression on the point's gaps
            const float px = fmaxf(fmaxf(boxes[cj] - q.x, q.x - boxes[3 * sG + cj]), 0.0f);
            const float py = fmaxf(fmaxf(boxes[sG + cj] - q.y, q.y - boxes[4 * sG + cj]), 0.0f);
            const float pz = fmaxf(fmaxf(boxes[2 * sG + cj] - q.z, q.z - boxes[5 * sG + cj]), 0.0f);
            const float pb = (px * px + py * py) + pz * pz;
            if (__builtin_amdgcn_ballot_w64(active && pb < b2) == 0ull) continue;
            const long long lc = n - (long long)cj * KNN_GROUP;
            visit_group<false>(pts + (size_t)cj * KNN_GROUP, lc < KNN_GROUP ? (int)lc : KNN_GROUP, lane, q.x, q.y, q.z, b0, b1, b2);
        }
    }
    if (!valid) return;
    const long long row = (long long)__float_as_int(q.w);  // (clamped into [0, n) by the gather)
    if (dist2_out) {
        dist2_out[3 * row] = b0; dist2_out[3 * row + 1] = b1; dist2_out[3 * row + 2] = b2;
    }
    // mean(d[2:end] .^ 2) of the tree's DISTANCES, then log(sqrt(max(1f-7, md) * point_size))   (dataset.jl:245-246)
    const float q0 = sqrtf(b0) * sqrtf(b0), q1 = sqrtf(b1) * sqrtf(b1), q2 = sqrtf(b2) * sqrtf(b2);
    const float md = ((q0 + q1) + q2) / 3.0f;
    const float s = logf(sqrtf(fmaxf(1e-7f, md) * point_size));
    if (scale_dims == 3) {
        scales_out[3 * row] = s; scales_out[3 * row + 1] = s; scales_out[3 * row + 2] = s;
    } else {
        scales_out[row] = ((s + s) + s) / 3.0f;  // isotropic: mean(scales; dims=1) (gaussians.jl:53)
    }
}

}  // namespace

static inline long long knn_groups(long long n) { return (n + KNN_GROUP - 1) / KNN_GROUP; }

// scratch: n float4 (the gathered points), then 6 floats per group (the boxes); 16-byte aligned
size_t gsr_knn_scratch_size(long long n) {
    if (n <= 0) return 0;
    return (size_t)n * sizeof(float4) + (size_t)knn_groups(n) * 6 * sizeof(float);
}

void gsr_launch_knn_scales(hipStream_t s, long long n, const float* points, const int32_t* order, float point_size,
                           int scale_dims, float* scales_out, float* dist2_out, void* scratch) {
    if (n <= 0) return;
    const int G = (int)knn_groups(n);
    float4* pts = reinterpret_cast<float4*>(scratch);
    float* boxes = reinterpret_cast<float*>(pts + n);
    const unsigned blocks = (unsigned)((G + 3) / 4);
    hipLaunchKernelGGL(knn_gather_kernel, dim3(blocks), dim3(256), 0, s, n, G, points, order, pts, boxes);
    hipLaunchKernelGGL(knn_search_kernel, dim3(blocks), dim3(256), 0, s, n, G, pts, boxes, point_size, scale_dims, scales_out,
                       dist2_out);
}
