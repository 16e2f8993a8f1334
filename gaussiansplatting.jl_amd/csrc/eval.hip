// The evaluation head (src/training.jl:487-532 `validate`; src/utils.jl:107-109 `mse` / `psnr`, :118 `quantize8`;
// src/fused_ssim.jl:34-238 with train = false) and the 8-bit frame export (src/rasterizer.jl:155-182 `gl_texture` /
// `to_image`).  One full-frame launch scores a view: the sky composite, the 8-bit quantiser and the u8 -> float conversion of
// the target happen in the loads, the 11x11 separable filter runs once over x and y, and only the map (if asked for) and
// three sums leave the kernel.  Compiled with -ffp-contract=off: every fp32 operation below is its own operation, in the
// order written, divisions are IEEE — ONE arithmetic, the CPU oracle's (no contracted twin: evaluation is not on the step
// path, its job is to agree with the oracle).
//
// The scored colour of channel c = 0..2 at a pixel of the (C,W,H) frame:
//   x = image[c]                                   without a sky frame
//   x = image[c] + (1 - image[4]) * sky[c]         with one (a product, then a sum: sky.hip's forward, bit for bit)
//   x = quant_level(x) * (1/255)                   with quantize; quant_level(x) = floorf(fminf(fmaxf(x, 0), 1) * 255 + 0.5)
// and the target y = target_f32 (W,H,3 planar), or (float)target_u8 * (1/255) from the (3,W,H) byte image.
//
// The strip walk of ssim_strip.h, shared with ssim.hip and in its exact build's arithmetic (SSIM_EXACT at its default of 1):
// a wave walks ONE channel of a strip of STRIP_H = 32 rows; a workgroup is the three channel waves of one strip (they read
// the same lines of the channel-interleaved frame), strips in raster order over blockIdx.x.
//
// The sums, all in double, in this order:
//   lane   : per owned pixel, rows ascending:  s_ssim += (double)map;  with d = x - y (fp32):  s_sq += (double)d * (double)d;
//            s_abs += (double)fabsf(d).  (d and |d| when the pixel's input row arrives, the map value five rows later.)
//   wave   : gsr::wave_sum (xor butterfly, off = 32..1) -> one row {Σssim, Σd², Σ|d|} of `scratch` per wave; row index =
//            3 * strip + channel.
//   final  : one workgroup of 256 threads, gsr::sum_partials<3> (block_reduce.h: each thread its rows ascending, then
//            thread 0 the 256 thread sums ascending);  n = 3·W·H;  out = {(float)(Σssim / n), (float)(Σd² / n),
//            (float)(-10 · log10(Σd² / n)), (float)(Σ|d| / n)}, every quotient and the logarithm in double, rounded once.
// No float atomics, no "last workgroup" counter: results are run-to-run bit-identical.  Every scratch word the final pass
// reads was written by the scoring launch.
#include "gsr_kernels.h"
#include "block_reduce.h"
#include "quant_level.h"
#include "ssim_strip.h"

namespace {

constexpr int STRIP_H = 32;  // output rows per wave: fixed, so that the scratch size depends on W and H alone
constexpr int NSUM = 3;      // Σssim, Σd², Σ|d|

// quant_level (quant_level.h): the integer level of `quantize8` (utils.jl:118) as a float, THE quantiser of both entry points

// what one lane loads of one row: untouched until the row is filtered
template <bool SKY, bool U8>
struct Raw {
    float c, a, s, t;
    unsigned char tb;
};

template <bool SKY, bool U8>
__global__ __launch_bounds__(192) void eval_score_kernel(int W, int H, int C, const float* __restrict__ image,
                                                         const float* __restrict__ sky, const float* __restrict__ target_f32,
                                                         const unsigned char* __restrict__ target_u8, int quantize, float C1,
                                                         float C2, float* __restrict__ ssim_map, double* __restrict__ partial) {
    __shared__ v2f rowbuf[3][ROW_LDS];
    const int lane = threadIdx.x & 63, ch = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nsx = (W + STRIP_W - 1) / STRIP_W;
    const int x0 = ((int)blockIdx.x % nsx) * STRIP_W, y0 = ((int)blockIdx.x / nsx) * STRIP_H;
    const int rows = min(STRIP_H, H - y0);
    v2f* buf = rowbuf[ch];
    if (lane < HALO) clear_halo(lane, buf);
    const Column col{x0, lane, W};
    const int nrows = rows + 2 * HALO, gxc = col.gxc();  // input rows: rr = 0 is frame row y0 - 5
    const unsigned io = 4u * (unsigned)(C * gxc), so = 12u * (unsigned)gxc, po = 4u * (unsigned)gxc, uo = 3u * (unsigned)gxc;
    const float* ip = image + ch;
    const float* sp = SKY ? sky + ch : nullptr;
    const float* tp = U8 ? nullptr : target_f32 + (size_t)W * H * ch;
    const unsigned char* up = U8 ? target_u8 + ch : nullptr;
    float* mp = ssim_map ? ssim_map + (size_t)W * H * ch : nullptr;
    // straight-line loads from a clamped address; rows and columns outside the frame become zeros when the row is filtered
    auto fetch = [&](int rr) {
        const unsigned gyc = (unsigned)min(max(y0 - HALO + rr, 0), H - 1);
        Raw<SKY, U8> r = {};
        r.c = at(ip, (unsigned)(C * W) * gyc, io);
        if (SKY) {
            r.a = at(image + 4, (unsigned)(C * W) * gyc, io);
            r.s = at(sp, (unsigned)(3 * W) * gyc, so);
        }
        if (U8)
            r.tb = at(up, (unsigned)(3 * W) * gyc, uo);
        else
            r.t = at(tp, (unsigned)W * gyc, po);
        return r;
    };
    Raw<SKY, U8> nxt[AHEAD];
#pragma unroll
    for (int i = 0; i < AHEAD; i++) nxt[i] = fetch(i);
    v2f hm[RING], hq[RING];  // horizontal results of the last 11 rows: (Σx, Σy), (Σx², Σy²)
    float hc[RING];          // ... Σxy
    double s_ssim = 0.0, s_sq = 0.0, s_abs = 0.0;
    for (int base = 0; base < nrows; base += RING) {
#pragma unroll
        for (int j = 0; j < RING; j++) {
            const int rr = base + j;
            if (rr < nrows) {
                const int gy = y0 - HALO + rr;
                const Raw<SKY, U8> r = nxt[0];
#pragma unroll
                for (int i = 0; i + 1 < AHEAD; i++) nxt[i] = nxt[i + 1];
                nxt[AHEAD - 1] = fetch(rr + AHEAD);
                float x = r.c;
                if (SKY) {
                    const float t = 1.0f - r.a;
                    x = x + t * r.s;
                }
                if (quantize) x = quant_level(x) * (1.0f / 255.0f);
                const float y = U8 ? (float)r.tb * (1.0f / 255.0f) : r.t;
                const v2f XY = col.col_in && gy >= 0 && gy < H ? v2f{x, y} : v2f{0.0f, 0.0f};
                horizontal_stats(buf, col.cx, XY, hm[j], hq[j], hc[j]);
                if (col.own && rr >= HALO && rr < nrows - HALO) {
                    const float df = XY.x - XY.y;
                    s_sq += (double)df * (double)df;
                    s_abs += (double)fabsf(df);
                }
                if (rr >= 2 * HALO) {  // output row rr - 10 of the strip is complete
                    const v2f om = ring_vertical(hm, j), oq = ring_vertical(hq, j);
                    const float oc = ring_vertical(hc, j);
                    if (col.own) {
                        const int py = y0 + rr - 2 * HALO;
                        const SsimTerms t{om.x, om.y, oq.x, oq.y, oc, C1, C2};
                        const float val = (t.Cv * t.Dv) / (t.A * t.Bv);
                        if (mp) at(mp, (unsigned)W * (unsigned)py, po) = val;
                        s_ssim += (double)val;
                    }
                }
            }
        }
    }
    s_ssim = gsr::wave_sum(s_ssim);
    s_sq = gsr::wave_sum(s_sq);
    s_abs = gsr::wave_sum(s_abs);
    if (lane == 0) {
        double* row = partial + ((size_t)blockIdx.x * 3 + ch) * NSUM;
        row[0] = s_ssim;
        row[1] = s_sq;
        row[2] = s_abs;
    }
}

__global__ __launch_bounds__(256) void eval_final_kernel(int n_rows, const double* __restrict__ partial, double count,
                                                         float* __restrict__ out) {
    __shared__ double red[NSUM][256];
    double s[NSUM];
    gsr::sum_partials<NSUM>(n_rows, partial, red, s);
    if (threadIdx.x != 0) return;
    const double mse = s[1] / count;
    out[0] = (float)(s[0] / count);
    out[1] = (float)mse;
    out[2] = (float)(-10.0 * log10(mse));  // mse = 0: +Inf, as 20·log10(1 / sqrt(0)) (utils.jl:109)
    out[3] = (float)(s[2] / count);
}

// One pixel per thread: the three levels of its colours as bytes, rows reversed with flip_rows.  Byte stores (vector memory
// instructions): no alignment is asked of the output.
template <bool SKY>
__global__ __launch_bounds__(256) void eval_rgb8_kernel(int W, int H, int C, const float* __restrict__ image,
                                                        const float* __restrict__ sky, int flip_rows,
                                                        unsigned char* __restrict__ out) {
    const size_t n = (size_t)W * H, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* p = image + i * C;
    float x0 = p[0], x1 = p[1], x2 = p[2];
    if (SKY) {
        const float t = 1.0f - p[4];
        x0 = x0 + t * sky[i * 3 + 0];
        x1 = x1 + t * sky[i * 3 + 1];
        x2 = x2 + t * sky[i * 3 + 2];
    }
    size_t o = i;
    if (flip_rows) {
        const size_t gy = i / (size_t)W, gx = i - gy * (size_t)W;
        o = ((size_t)H - 1 - gy) * (size_t)W + gx;
    }
    unsigned char* q = out + o * 3;
    q[0] = (unsigned char)quant_level(x0);
    q[1] = (unsigned char)quant_level(x1);
    q[2] = (unsigned char)quant_level(x2);
}

size_t strips_of(int W, int H) { return (size_t)((W + STRIP_W - 1) / STRIP_W) * (size_t)((H + STRIP_H - 1) / STRIP_H); }

}  // namespace

// one row of three doubles per wave of the scoring launch
size_t gsr_eval_scratch_size(int W, int H) { return strips_of(W, H) * 3 * NSUM * sizeof(double); }

void gsr_launch_eval_metrics(hipStream_t s, int W, int H, int C, const float* image, const float* sky_rgb,
                             const float* target_f32, const unsigned char* target_u8, int quantize, float* ssim_map, float* out,
                             void* scratch) {
    const unsigned nb = (unsigned)strips_of(W, H);
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;  // fused_ssim.jl:374
    double* partial = (double*)scratch;
#define GSR_EVAL_LAUNCH(SKY, U8)                                                                                        \
    hipLaunchKernelGGL((eval_score_kernel<SKY, U8>), dim3(nb), dim3(192), 0, s, W, H, C, image, sky_rgb, target_f32,    \
                       target_u8, quantize, C1, C2, ssim_map, partial)
    if (sky_rgb) {
        if (target_u8) GSR_EVAL_LAUNCH(true, true); else GSR_EVAL_LAUNCH(true, false);
    } else {
        if (target_u8) GSR_EVAL_LAUNCH(false, true); else GSR_EVAL_LAUNCH(false, false);
    }
#undef GSR_EVAL_LAUNCH
    hipLaunchKernelGGL(eval_final_kernel, dim3(1), dim3(256), 0, s, (int)(nb * 3), partial, 3.0 * (double)W * (double)H, out);
}

void gsr_launch_frame_rgb8(hipStream_t s, int W, int H, int C, const float* image, const float* sky_rgb, int flip_rows,
                           unsigned char* rgb8_out) {
    const size_t n = (size_t)W * H;
    const unsigned nb = (unsigned)((n + 255) / 256);
    if (sky_rgb)
        hipLaunchKernelGGL(eval_rgb8_kernel<true>, dim3(nb), dim3(256), 0, s, W, H, C, image, sky_rgb, flip_rows, rgb8_out);
    else
        hipLaunchKernelGGL(eval_rgb8_kernel<false>, dim3(nb), dim3(256), 0, s, W, H, C, image, sky_rgb, flip_rows, rgb8_out);
}
