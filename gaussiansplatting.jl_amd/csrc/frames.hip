// Geometry frames: what the reference makes of the depth, alpha and normal channels of a frame on the HOST
// (scripts/render-views.jl:264-308,390-407 `depth_image` / `normal_image`; src/rasterization/rasterizer.jl:163-198 `gl_depth` /
// `to_depth`; src/gui/worker.jl:688-726 `handle_pick!`), on the device: no frame is copied out, no depth is sorted on the host.
// Compiled with -ffp-contract=off: every fp32 / fp64 operation below is its own operation, in the order written, divisions
// and square roots are IEEE.  `image` is the rasterizer's (C,W,H) frame, channel fastest: 3 depth, 4 alpha, 5..7 normal.
//
// Per pixel (fp32):  covered = alpha >= min_alpha (a NaN alpha is not covered);  e = depth / fmaxf(alpha, min_alpha), ONE division.
//
// gsr_depth_scale — the white level of `depth_image` (render-views.jl:272-277), an EXACT percentile left on the device.
//   key(e) = bits(e) ^ (sign ? 0xFFFFFFFF : 0x80000000): unsigned order of the keys == Julia's `sort` order of the floats
//   (-0.0 < +0.0; NaN unspecified).  v = the covered e ascending, n their number.  Radix select over 11 + 11 + 10 key bits:
//     1. key pass   : per pixel reads depth and alpha (the only pass over the 32-byte pixels), writes the key — 0xFFFFFFFF for
//                     a pixel that is not covered: it sorts last, no rank below n reaches it — into scratch, and counts the
//                     covered keys by their top 11 bits: LDS histogram per workgroup, one integer atomicAdd per non-empty bin.
//     2. pick 0     : one workgroup.  n = Σ histogram.  Statistics.jl's definition 7 in double:  p = percentile / 100;
//                     m = 1 - p;  aleph = fma((double)n, p, m);  j = clamp(trunc(aleph), 1, n - 1);  γ = clamp(aleph - j, 0, 1).
//                     The 0-based ranks j - 1 and j (n == 1: 0 and 0) each get their bin and their rank inside it.
//     3. narrow 1, pick 1, narrow 2, pick 2 : two passes over the 4-byte keys; a key that carries the prefix of rank A (rank B)
//                     counts into histogram A (B) by its next 11 / last 10 bits.  BOTH ranks are tracked: they may part ways at
//                     any level.  pick 2 has the two keys, hence a = v[j], b = v[j+1], and writes stats_out:
//                       d = b - a (fp32);  q = (double)a + γ · (double)d (a double product, then a double sum);
//                       scale = fmaxf((float)q, 1e-6f);   n == 0: scale = 1, a_bits = b_bits = 0.
//   This is `a + γ*(b-a)` as Statistics.jl evaluates it for a Float32 vector and a Float64 p.  Newer Statistics.jl versions
//   take (1-γ)a + γb when a ≉ b, older ones compute n*p + m without the fma; NOBODY HAS RUN JULIA AGAINST THIS.  What is
//   pinned is n and the two order statistics (a_bits, b_bits), which no version disputes.
//   Integer atomics only (LDS and global histograms): the result is the same bits run to run.  The launcher clears the
//   histograms with one memset; every other scratch word that is read was written by an earlier launch of the same call.
//
// gsr_frame_depth16 — x = expected ? (covered ? e : 0) : depth;  scale = *scale_dev or depth_max;  inv = 1.0f / scale (one
//   division);  y = fminf(fmaxf(x · inv, 0), 1);  word = (uint16) floorf(y · 65535.0f + 0.5f) — the project's quantiser form
//   (quant_level.h) at 16 bits.  FixedPointNumbers' N0f16(y) rounds y · 65535 to nearest: the two can differ only where
//   y · 65535 is an exact .5 tie.  2-byte stores; rows reversed with flip_rows.
//
// gsr_frame_normal8 — `normal_image` (render-views.jl:291-308):  n = N / fmaxf(alpha, min_alpha) (three divisions);
//   len = sqrtf((nx² + ny²) + nz²);  degenerate = len < 1e-6f || !(alpha >= min_alpha);  n = n / fmaxf(len, 1e-6f);  a degenerate
//   pixel is (0,0,0).  With R_c2w (column-major): row i of R·n = (r[i]·x + r[i+3]·y) + r[i+6]·z, a degenerate pixel stays
//   zero.  The reference multiplies through BLAS, whose order of the two sums is not known: THIS ORDER IS OURS.
//   byte = (uint8) quant_level(c · 0.5f + 0.5f), gsr_frame_rgb8's device function.  Byte stores: no alignment is asked.
//
// gsr_pick_point — `handle_pick!`: one workgroup of one wave.  The window [px-hw, px+hw] x [py-hw, py+hw] clipped to the frame
//   is numbered row-major, x fastest; lane l adds, in fp32, the raw depths > 1e-2f of elements l, l + 64, ... ascending, and
//   counts them; lane 0 adds the 64 lane sums (and counts) lane-ascending;  z = sum / (float)count.
//   cx = principal[0] · (float)W;  p.x = (((float)px - 0.5f) - cx) · z / fx  (difference, difference, product, quotient);  p.y
//   alike;  p.z = z;  target[i] = ((R[3i]·p.x + R[3i+1]·p.y) + R[3i+2]·p.z) + camera_center[i], R the camera's world->camera
//   rotation, column-major: row i of its transpose (the reference inverts the 4x4 pose; for a rigid pose that is the transpose).
//   out4 = {target, (float)count};  count == 0 or a pixel outside the frame: {0,0,0,0}.
#include "frames.h"
#include "quant_level.h"

namespace {

constexpr int TOP_BITS = 11, MID_BITS = 11, LOW_BITS = 10;       // 32 key bits in three levels
constexpr int NB_MAX = 1 << TOP_BITS;                             // bins of the widest level
constexpr unsigned NOT_COVERED = 0xFFFFFFFFu;                     // sorts last
// scratch, in 32-bit words: control block, five histograms, the keys
enum : unsigned {
    CT_N = 0, CT_PREFIX_A, CT_PREFIX_B, CT_RANK_A, CT_RANK_B, CT_GAMMA = 6 /* a double: words 6, 7 */, CT_WORDS = 16,
    HIST0 = CT_WORDS, HIST_A1 = HIST0 + (1u << TOP_BITS), HIST_B1 = HIST_A1 + (1u << MID_BITS), HIST_A2 = HIST_B1 + (1u << MID_BITS),
    HIST_B2 = HIST_A2 + (1u << LOW_BITS), KEYS = HIST_B2 + (1u << LOW_BITS)
};
static_assert(KEYS % 2 == 0, "the keys start 8-byte aligned");
constexpr int BATCH = 4;            // loads in flight per thread
constexpr unsigned MAX_BLOCKS = 1024;  // 2048 with one trip per thread measured slower (key pass 36 us for 24: DESIGN.md §18)

__device__ __forceinline__ unsigned key_of(float e) {
    const unsigned u = __float_as_uint(e);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }

__device__ __forceinline__ void clear_bins(unsigned* hist, int n) {
    for (int i = threadIdx.x; i < n; i += 256) hist[i] = 0u;
}
__device__ __forceinline__ void flush_bins(const unsigned* hist, unsigned* global, int n) {
    for (int i = threadIdx.x; i < n; i += 256) {
        const unsigned h = hist[i];
        if (h) atomicAdd(global + i, h);
    }
}

__global__ __launch_bounds__(256) void frames_key_kernel(unsigned npix, int C, const float* __restrict__ image, float min_alpha,
                                                         unsigned* __restrict__ scratch) {
    __shared__ unsigned hist[NB_MAX];
    clear_bins(hist, NB_MAX);
    __syncthreads();
    unsigned* keys = scratch + KEYS;
    const unsigned stride = gridDim.x * 256u;
    for (unsigned base = blockIdx.x * 256u + threadIdx.x; base < npix; base += BATCH * stride) {  // npix <= 2^30: no wrap
        float d[BATCH], a[BATCH];
#pragma unroll
        for (int b = 0; b < BATCH; b++) {
            const unsigned i = base + b * stride;
            const float* p = image + (size_t)min(i, npix - 1) * C;
            d[b] = p[3];
            a[b] = p[4];
        }
#pragma unroll
        for (int b = 0; b < BATCH; b++) {
            const unsigned i = base + b * stride;
            if (i >= npix) break;
            unsigned k = NOT_COVERED;
            if (a[b] >= min_alpha) {
                k = key_of(d[b] / fmaxf(a[b], min_alpha));
                atomicAdd(&hist[k >> (32 - TOP_BITS)], 1u);
            }
            keys[i] = k;
        }
    }
    __syncthreads();
    flush_bins(hist, scratch + HIST0, NB_MAX);
}

// keys whose bits above `hi_shift` equal rank A's (rank B's) prefix count by their next `bits` bits
__global__ __launch_bounds__(256) void frames_narrow_kernel(unsigned npix, int hi_shift, int bits, unsigned hist_a, unsigned hist_b,
                                                            unsigned* __restrict__ scratch) {
    __shared__ unsigned hist[2][NB_MAX];
    const int nb = 1 << bits;
    const unsigned pa = scratch[CT_PREFIX_A], pb = scratch[CT_PREFIX_B];
    const bool two = pa != pb;
    clear_bins(hist[0], nb);
    if (two) clear_bins(hist[1], nb);
    __syncthreads();
    const unsigned* keys = scratch + KEYS;
    const unsigned stride = gridDim.x * 256u;
    for (unsigned base = blockIdx.x * 256u + threadIdx.x; base < npix; base += BATCH * stride) {
        unsigned k[BATCH];
#pragma unroll
        for (int b = 0; b < BATCH; b++) k[b] = keys[min(base + b * stride, npix - 1)];
#pragma unroll
        for (int b = 0; b < BATCH; b++) {
            if (base + b * stride >= npix) break;
            const unsigned hi = k[b] >> hi_shift, bin = (k[b] >> (hi_shift - bits)) & (unsigned)(nb - 1);
            if (hi == pa) atomicAdd(&hist[0][bin], 1u);
            if (two && hi == pb) atomicAdd(&hist[1][bin], 1u);
        }
    }
    __syncthreads();
    flush_bins(hist[0], scratch + hist_a, nb);
    if (two) flush_bins(hist[1], scratch + hist_b, nb);
}

// One workgroup: the bin of each rank in this level's histogram(s), and the rank inside it.  level 0 also makes n and the two
// ranks; level 2 ends with the two keys and writes stats_out.
__global__ __launch_bounds__(256) void frames_pick_kernel(int level, double percentile, unsigned* __restrict__ scratch,
                                                          unsigned* __restrict__ stats_out) {
    __shared__ unsigned wave_a[4], wave_b[4], fin[2];
    const int tid = threadIdx.x;
    const int bits = level == 0 ? TOP_BITS : level == 1 ? MID_BITS : LOW_BITS;
    const int per = (1 << bits) / 256;  // 8 or 4 bins per thread
    unsigned pa = 0, pb = 0, ra = 0, rb = 0;
    if (level > 0) {
        pa = scratch[CT_PREFIX_A];
        pb = scratch[CT_PREFIX_B];
        ra = scratch[CT_RANK_A];
        rb = scratch[CT_RANK_B];
    }
    const unsigned* ha = scratch + (level == 0 ? HIST0 : level == 1 ? HIST_A1 : HIST_A2);
    const unsigned* hb = (level == 0 || pa == pb) ? ha : scratch + (level == 1 ? HIST_B1 : HIST_B2);
    unsigned ca[8], cb[8], ta = 0, tb = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        ca[q] = q < per ? ha[tid * per + q] : 0u;
        cb[q] = q < per ? hb[tid * per + q] : 0u;
        ta += ca[q];
        tb += cb[q];
    }
    // scan of the 256 thread sums: inside each wave by lane shifts, across the four waves through LDS
    const int lane = tid & 63, wave = tid >> 6;
    unsigned ia = ta, ib = tb;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned ua = __shfl_up(ia, off), ub = __shfl_up(ib, off);
        if (lane >= off) {
            ia += ua;
            ib += ub;
        }
    }
    if (lane == 63) {
        wave_a[wave] = ia;
        wave_b[wave] = ib;
    }
    if (tid < 2) fin[tid] = 0u;
    __syncthreads();
    unsigned ea = ia - ta, eb = ib - tb, total = 0;  // counts in front of this thread's bins; all of histogram A
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const unsigned sa = wave_a[w], sb = wave_b[w];
        total += sa;
        if (w < wave) {
            ea += sa;
            eb += sb;
        }
    }
    if (level == 0) {
        const unsigned n = total;
        double gamma = 0.0;
        if (n >= 2) {
            const double p = percentile / 100.0;
            const double m = 1.0 - p;
            const double aleph = fma((double)n, p, m);
            const double j = fmin(fmax(trunc(aleph), 1.0), (double)(n - 1));
            gamma = fmin(fmax(aleph - j, 0.0), 1.0);
            ra = (unsigned)j - 1u;
            rb = ra + 1u;
        }
        if (tid == 0) {
            scratch[CT_N] = n;
            scratch[CT_GAMMA] = (unsigned)__double2loint(gamma);
            scratch[CT_GAMMA + 1] = (unsigned)__double2hiint(gamma);
        }
    }
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const unsigned bin = (unsigned)(tid * per + q);
        if (ra >= ea && ra - ea < ca[q]) {
            const unsigned key = (pa << bits) | bin;
            scratch[CT_PREFIX_A] = key;
            scratch[CT_RANK_A] = ra - ea;
            fin[0] = key;
        }
        if (rb >= eb && rb - eb < cb[q]) {
            const unsigned key = (pb << bits) | bin;
            scratch[CT_PREFIX_B] = key;
            scratch[CT_RANK_B] = rb - eb;
            fin[1] = key;
        }
        ea += ca[q];
        eb += cb[q];
    }
    if (level < 2) return;
    __syncthreads();
    if (tid != 0) return;
    const unsigned n = scratch[CT_N];
    float scale = 1.0f;
    unsigned a_bits = 0u, b_bits = 0u;
    if (n > 0) {
        const double gamma = __hiloint2double((int)scratch[CT_GAMMA + 1], (int)scratch[CT_GAMMA]);
        const float a = value_of(fin[0]), b = value_of(fin[1]);
        const float d = b - a;
        const double t = gamma * (double)d;
        const double q = (double)a + t;
        scale = fmaxf((float)q, 1e-6f);
        a_bits = __float_as_uint(a);
        b_bits = __float_as_uint(b);
    }
    stats_out[0] = __float_as_uint(scale);
    stats_out[1] = n;
    stats_out[2] = a_bits;
    stats_out[3] = b_bits;
}

// One pixel per thread, as eval.hip's rgb8 export.
__global__ __launch_bounds__(256) void frames_depth16_kernel(int W, int H, int C, const float* __restrict__ image, int expected,
                                                             float min_alpha, float depth_max, const float* __restrict__ scale_dev,
                                                             int flip_rows, unsigned short* __restrict__ out) {
    const size_t n = (size_t)W * H, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* p = image + i * C;
    float x = p[3];
    if (expected) {
        const float alpha = p[4];
        const float e = x / fmaxf(alpha, min_alpha);
        x = alpha >= min_alpha ? e : 0.0f;
    }
    const float scale = scale_dev ? *scale_dev : depth_max;
    const float inv = 1.0f / scale;
    const float y = fminf(fmaxf(x * inv, 0.0f), 1.0f);
    size_t o = i;
    if (flip_rows) {
        const size_t gy = i / (size_t)W, gx = i - gy * (size_t)W;
        o = ((size_t)H - 1 - gy) * (size_t)W + gx;
    }
    out[o] = (unsigned short)floorf(y * 65535.0f + 0.5f);
}

__global__ __launch_bounds__(256) void frames_normal8_kernel(int W, int H, int C, const float* __restrict__ image, float min_alpha,
                                                             GsrRot rot, unsigned char* __restrict__ out) {
    const size_t n = (size_t)W * H, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* p = image + i * C;
    const float alpha = p[4];
    const float den = fmaxf(alpha, min_alpha);
    float nx = p[5] / den, ny = p[6] / den, nz = p[7] / den;
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    const bool degenerate = len < 1e-6f || !(alpha >= min_alpha);
    const float l = fmaxf(len, 1e-6f);
    nx = nx / l;
    ny = ny / l;
    nz = nz / l;
    if (degenerate) nx = ny = nz = 0.0f;
    if (rot.use && !degenerate) {
        const float* r = rot.r;
        const float wx = (r[0] * nx + r[3] * ny) + r[6] * nz;
        const float wy = (r[1] * nx + r[4] * ny) + r[7] * nz;
        const float wz = (r[2] * nx + r[5] * ny) + r[8] * nz;
        nx = wx;
        ny = wy;
        nz = wz;
    }
    unsigned char* q = out + i * 3;
    q[0] = (unsigned char)quant_level(nx * 0.5f + 0.5f);
    q[1] = (unsigned char)quant_level(ny * 0.5f + 0.5f);
    q[2] = (unsigned char)quant_level(nz * 0.5f + 0.5f);
}

__global__ __launch_bounds__(64) void frames_pick_point_kernel(int W, int H, int C, const float* __restrict__ image, GsrPickCam cam,
                                                               int px, int py, int hw, float* __restrict__ out4) {
    __shared__ float lane_sum[64];
    __shared__ unsigned lane_cnt[64];
    const int lane = threadIdx.x;
    const bool inside = px >= 1 && px <= W && py >= 1 && py <= H;
    float s = 0.0f;
    unsigned c = 0u;
    if (inside) {
        const int x0 = max(1, px - hw), x1 = min(W, px + hw), y0 = max(1, py - hw), y1 = min(H, py + hw);  // 1-based, inclusive
        const int ww = x1 - x0 + 1, count = ww * (y1 - y0 + 1);
        for (int e = lane; e < count; e += 64) {
            const int wy = e / ww, wx = e - wy * ww;
            const size_t pix = (size_t)(y0 - 1 + wy) * (size_t)W + (size_t)(x0 - 1 + wx);
            const float d = image[pix * C + 3];
            if (d > 1e-2f) {
                s = s + d;
                c++;
            }
        }
    }
    lane_sum[lane] = s;
    lane_cnt[lane] = c;
    __syncthreads();
    if (lane != 0) return;
    float sum = 0.0f;
    unsigned cnt = 0u;
    for (int l = 0; l < 64; l++) {
        sum = sum + lane_sum[l];
        cnt += lane_cnt[l];
    }
    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (cnt > 0u) {
        const float z = sum / (float)cnt;
        const float cx = cam.principal[0] * (float)W, cy = cam.principal[1] * (float)H;
        const float p0 = (((float)px - 0.5f) - cx) * z / cam.focal[0];
        const float p1 = (((float)py - 0.5f) - cy) * z / cam.focal[1];
#pragma unroll
        for (int i = 0; i < 3; i++)
            o[i] = ((cam.R[3 * i] * p0 + cam.R[3 * i + 1] * p1) + cam.R[3 * i + 2] * z) + cam.center[i];
        o[3] = (float)cnt;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out4[i] = o[i];
}

unsigned stream_blocks(size_t npix) {
    const size_t nb = (npix + (size_t)256 * BATCH * 2 - 1) / ((size_t)256 * BATCH * 2);  // two trips per thread up to MAX_BLOCKS
    return (unsigned)(nb < 1 ? 1 : nb > MAX_BLOCKS ? MAX_BLOCKS : nb);
}

}  // namespace

// the control block, the five histograms and one key per pixel; a multiple of 8
size_t gsr_frames_scratch_size(int W, int H) { return (((size_t)KEYS + (size_t)W * H) * 4 + 7) & ~(size_t)7; }

void gsr_launch_depth_scale(hipStream_t s, int W, int H, int C, const float* image, float min_alpha, double percentile,
                            void* stats_out, void* scratch) {
    const unsigned npix = (unsigned)((size_t)W * H), nb = stream_blocks(npix);
    unsigned* w = (unsigned*)scratch;
    (void)hipMemsetAsync(scratch, 0, (size_t)KEYS * 4, s);  // control block and histograms (a failure shows in hipGetLastError)
    hipLaunchKernelGGL(frames_key_kernel, dim3(nb), dim3(256), 0, s, npix, C, image, min_alpha, w);
    hipLaunchKernelGGL(frames_pick_kernel, dim3(1), dim3(256), 0, s, 0, percentile, w, (unsigned*)stats_out);
    hipLaunchKernelGGL(frames_narrow_kernel, dim3(nb), dim3(256), 0, s, npix, 32 - TOP_BITS, MID_BITS, (unsigned)HIST_A1,
                       (unsigned)HIST_B1, w);
    hipLaunchKernelGGL(frames_pick_kernel, dim3(1), dim3(256), 0, s, 1, percentile, w, (unsigned*)stats_out);
    hipLaunchKernelGGL(frames_narrow_kernel, dim3(nb), dim3(256), 0, s, npix, LOW_BITS, LOW_BITS, (unsigned)HIST_A2,
                       (unsigned)HIST_B2, w);
    hipLaunchKernelGGL(frames_pick_kernel, dim3(1), dim3(256), 0, s, 2, percentile, w, (unsigned*)stats_out);
}

void gsr_launch_frame_depth16(hipStream_t s, int W, int H, int C, const float* image, int expected, float min_alpha,
                              float depth_max, const float* scale_dev, int flip_rows, uint16_t* depth16_out) {
    const unsigned nb = (unsigned)(((size_t)W * H + 255) / 256);
    hipLaunchKernelGGL(frames_depth16_kernel, dim3(nb), dim3(256), 0, s, W, H, C, image, expected, min_alpha, depth_max, scale_dev,
                       flip_rows, (unsigned short*)depth16_out);
}

void gsr_launch_frame_normal8(hipStream_t s, int W, int H, int C, const float* image, float min_alpha, const GsrRot& rot,
                              unsigned char* normal8_out) {
    const unsigned nb = (unsigned)(((size_t)W * H + 255) / 256);
    hipLaunchKernelGGL(frames_normal8_kernel, dim3(nb), dim3(256), 0, s, W, H, C, image, min_alpha, rot, normal8_out);
}

void gsr_launch_pick_point(hipStream_t s, int W, int H, int C, const float* image, const GsrPickCam& cam, int px, int py,
                           int half_window, float* out4) {
    hipLaunchKernelGGL(frames_pick_point_kernel, dim3(1), dim3(64), 0, s, W, H, C, image, cam, px, py, half_window, out4);
}
