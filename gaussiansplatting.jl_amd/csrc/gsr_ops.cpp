// C ABI of libgsr_hip.so (include/gsr.h), the part without a handle: every entry point that checks its arguments, launches
// its kernels on the caller's stream and keeps nothing — planar SSIM, the trainer's prologue / Adam / tail, row gathers, the
// bilateral grid, the geometry, depth and sky losses, the evaluation head, the geometry frames, densification, MCMC, Morton
// codes, k-NN, the 3-D smoothing filter, the SH codebook k-means and its fine-tuning gradient, the quantised model container, TSDF fusion and mesh extraction, PLY rows, the multi-view SH gradient, the all-reduce.  (The handle and its launch choreography are gsr_api.cpp's.)
#include <dlfcn.h>

#include <algorithm>
#include <cmath>

#include "gsr_kernels.h"
#include "frames.h"
#include "adam_math.h"
#include "gsr_host.h"

using namespace gsr_host;

namespace {

// every entry point's last step: whether its launches were accepted
int launched() {
    HIPCHK(hipGetLastError());
    return GSR_OK;
}

// the caller's scratch against what `what` needs
int check_scratch(size_t scratch_bytes, size_t need, const char* what) {
    if (scratch_bytes < need) return fail(GSR_E_INVALID_ARG, "scratch of %zu bytes, the %s needs %zu", scratch_bytes, what, need);
    return GSR_OK;
}

}  // namespace

extern "C" {

int gsr_ssim_forward(int W, int H, int CH, int B, const float* img, const float* ref, float C1, float C2, int train,
                     float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream) {
    if (W <= 0 || H <= 0 || CH <= 0 || B <= 0) return fail(GSR_E_INVALID_ARG, "bad SSIM shape");
    if (!img || !ref || !ssim_map) return fail(GSR_E_INVALID_ARG, "null SSIM array");
    if (train && (!dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12)) return fail(GSR_E_INVALID_ARG, "train needs the 3 partial maps");
    if ((size_t)CH * B > 65535) return fail(GSR_E_INVALID_ARG, "CH*B too large");
    if ((size_t)W * H > 0xFFFFFFFFull) return fail(GSR_E_INVALID_ARG, "SSIM plane too large");  // 32-bit offsets inside a plane
    (g_ssim_exact.load(std::memory_order_relaxed) ? gsr_launch_ssim_fwd_exact : gsr_launch_ssim_fwd_fast)((hipStream_t)stream, W, H, CH, B, img, ref, C1, C2, train,
                                                                          ssim_map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12);
    return launched();
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
    return launched();
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
    return launched();
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
    return launched();
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
    return launched();
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
    return launched();
}

size_t gsr_mask_findall_scratch_bytes(int64_t n) { return n > 0 ? gsr_findall_scratch_bytes(n) : sizeof(uint32_t); }

int gsr_mask_findall(const uint8_t* mask, int64_t n, uint32_t* indices, uint32_t* count_out, void* scratch,
                     void* stream) {
    if (n < 0 || n > 0xFFFFFFFFll) return fail(GSR_E_INVALID_ARG, "n out of range");
    if (!count_out || (n > 0 && (!mask || !indices || !scratch))) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_findall((hipStream_t)stream, n, mask, indices, count_out, (uint32_t*)scratch);
    return launched();
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
    return launched();
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
    return launched();
}

int gsr_bilateral_slice_backward(int32_t W, int32_t H, int32_t C, const float* image, const float* grid, int32_t gx,
                                 int32_t gy, int32_t gz, const float* vout, float* vimage, float* vgrid, void* scratch,
                                 size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_bilateral_image(W, H, C)) || (rc = check_bilateral_grid(gx, gy, gz))) return rc;
    if (!image || !grid || !vout || !vimage || !vgrid || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    if ((rc = check_scratch(scratch_bytes, gsr_bilateral_scratch_bytes(W, H, gx, gy, gz), "pullback"))) return rc;
    gsr_launch_bilateral_bwd((hipStream_t)stream, W, H, C, image, grid, gx, gy, gz, vout, vimage, vgrid, (float*)scratch);
    return launched();
}

int gsr_bilateral_tv(int32_t n_images, int32_t gx, int32_t gy, int32_t gz, const float* grids, float weight,
                     float* loss_out, float* grad_out, void* scratch, size_t scratch_bytes, void* stream) {
    int rc;
    if (n_images < 1) return fail(GSR_E_INVALID_ARG, "n_images = %d", n_images);
    if ((rc = check_bilateral_grid(gx, gy, gz))) return rc;
    if (!grids || !loss_out || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    if ((rc = check_scratch(scratch_bytes, gsr_bilateral_tv_scratch_bytes(n_images), "TV"))) return rc;
    gsr_launch_bilateral_tv((hipStream_t)stream, n_images, gx, gy, gz, grids, bilateral_tv_consts(n_images, gx, gy, gz, weight),
                            loss_out, grad_out, (float*)scratch);
    return launched();
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
    if ((rc = check_scratch(scratch_bytes, gsr_bilateral_tv_scratch_bytes(n_images), "tail"))) return rc;
    const float lr_t = adam_lr_t(lr, beta1, beta2, current_step);
    const gsr::AdamHyper h{lr_t, beta1, beta2, 1.0f - beta1, 1.0f - beta2, eps};
    gsr_launch_bilateral_adam_tail((hipStream_t)stream, n_images, gx, gy, gz, grids, mu, nu, vgrid_view, view,
                                   bilateral_tv_consts(n_images, gx, gy, gz, tv_weight), h, tv_loss_out, (float*)scratch);
    return launched();
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
    if ((rc = check_scratch(scratch_bytes, gsr_normal_loss_scratch_bytes(W, H), "depth-normal loss"))) return rc;
    gsr_launch_normal_loss_fwd((hipStream_t)stream, W, H, image, cam->focal, cam->principal, weight, loss_out, stats_out,
                               weights_out, (float*)scratch);
    return launched();
}

int gsr_normal_loss_backward(int32_t W, int32_t H, int32_t C, const float* image, const gsr_camera* cam, float weight,
                             float* vpixels, const void* scratch, size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_normal_loss_frame(W, H, C)) || (rc = check_normal_loss_camera(cam))) return rc;
    if (!image || !vpixels || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    if (image == vpixels) return fail(GSR_E_INVALID_ARG, "vpixels must not be the image");
    if ((rc = check_scratch(scratch_bytes, gsr_normal_loss_scratch_bytes(W, H), "depth-normal loss"))) return rc;
    gsr_launch_normal_loss_bwd((hipStream_t)stream, W, H, image, cam->focal, cam->principal, weight, vpixels,
                               (const float*)scratch);
    return launched();
}

size_t gsr_flatten_loss_scratch_bytes(int32_t n) { return gsr_flatten_loss_scratch_floats(n) * sizeof(float); }

int gsr_flatten_loss(int32_t n, int32_t scale_dims, const float* scales_raw, float weight, float* loss_out, float* vscales,
                     void* scratch, size_t scratch_bytes, void* stream) {
    if (n < 0) return fail(GSR_E_INVALID_ARG, "negative n");
    if (scale_dims != 1 && scale_dims != 3) return fail(GSR_E_INVALID_ARG, "scale_dims = %d: 1 (isotropic) or 3", scale_dims);
    if (!loss_out || (n > 0 && (!scales_raw || !scratch))) return fail(GSR_E_INVALID_ARG, "null array");
    if (int rc = check_scratch(scratch_bytes, gsr_flatten_loss_scratch_bytes(n), "flatten loss")) return rc;
    gsr_launch_flatten_loss((hipStream_t)stream, n, scale_dims, scales_raw, weight, loss_out, vscales, (float*)scratch);
    return launched();
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
    return launched();
}

int gsr_depth_loss_forward(int32_t W, int32_t H, int32_t C, const float* image, const float* prior, const gsr_depth_anchor* anchor,
                           float qstep, float lambda_grad, float weight, float* loss_out, float* stats_out, float* target_out,
                           float* half_band_out, uint8_t* flags_out, void* scratch, size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_depth_loss_args(W, H, C, anchor, qstep))) return rc;
    if (!image || !prior || !loss_out || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    if ((uintptr_t)scratch % 16) return fail(GSR_E_INVALID_ARG, "scratch must be 16-byte aligned");
    if ((rc = check_scratch(scratch_bytes, gsr_depth_loss_scratch_bytes(W, H), "depth loss"))) return rc;
    gsr_launch_depth_loss_fwd((hipStream_t)stream, W, H, C, image, prior, &anchor->a, qstep, lambda_grad, weight, loss_out,
                              stats_out, target_out, half_band_out, flags_out, scratch);
    return launched();
}

int gsr_depth_loss_backward(int32_t W, int32_t H, int32_t C, const float* image, const float* prior, const gsr_depth_anchor* anchor,
                            float qstep, float lambda_grad, float weight, float* vpixels, const void* scratch, size_t scratch_bytes,
                            void* stream) {
    int rc;
    if ((rc = check_depth_loss_args(W, H, C, anchor, qstep))) return rc;
    if (!image || !prior || !vpixels || !scratch) return fail(GSR_E_INVALID_ARG, "null array");
    if (image == vpixels) return fail(GSR_E_INVALID_ARG, "vpixels must not be the image");
    if ((uintptr_t)scratch % 16) return fail(GSR_E_INVALID_ARG, "scratch must be 16-byte aligned");
    if ((rc = check_scratch(scratch_bytes, gsr_depth_loss_scratch_bytes(W, H), "depth loss"))) return rc;
    // prior, anchor and qstep are the forward's: what they determine per pixel is in the records the forward left in scratch
    gsr_launch_depth_loss_bwd((hipStream_t)stream, W, H, C, image, lambda_grad, weight, vpixels, scratch);
    return launched();
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
    return launched();
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
    return launched();
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
    return launched();
}

int gsr_frame_rgb8(int32_t W, int32_t H, int32_t C, const float* image, const float* sky_rgb, int32_t flip_rows,
                   uint8_t* rgb8_out, void* stream) {
    int rc;
    if ((rc = check_eval_frame(W, H, C, image, sky_rgb))) return rc;
    if (!rgb8_out) return fail(GSR_E_INVALID_ARG, "null rgb8_out");
    gsr_launch_frame_rgb8((hipStream_t)stream, W, H, C, image, sky_rgb, flip_rows != 0, rgb8_out);
    return launched();
}

// ---- geometry frames: exact depth percentile, 16-bit depth, 8-bit normals, the pick (frames.hip; render-views.jl:264-308) ----
namespace {
int check_geometry_frame(int32_t W, int32_t H, int32_t C, int32_t c_min, const void* image) {
    if (W < 1 || H < 1) return fail(GSR_E_INVALID_ARG, "image size %d x %d", W, H);
    if (C < c_min) return fail(GSR_E_INVALID_ARG, "C = %d: this call reads channel %d of the frame (C >= %d)", C, c_min - 1, c_min);
    if ((uint64_t)W * (uint64_t)H * (uint64_t)C > 0xFFFFFFFFull)
        return fail(GSR_E_INVALID_ARG, "frame too large: %d x %d x %d is 2^32 elements or more", C, W, H);
    if (!image) return fail(GSR_E_INVALID_ARG, "null image");
    return GSR_OK;
}
int check_min_alpha(float min_alpha) {
    if (!(min_alpha > 0.0f)) return fail(GSR_E_INVALID_ARG, "min_alpha = %g: must be > 0", (double)min_alpha);
    return GSR_OK;
}
}  // namespace

size_t gsr_frames_scratch_bytes(int32_t W, int32_t H) {
    if (W < 1 || H < 1) return 0;
    return gsr_frames_scratch_size(W, H);
}

int gsr_depth_scale(int32_t W, int32_t H, int32_t C, const float* image, float min_alpha, double percentile, void* stats_out,
                    void* scratch, void* stream) {
    int rc;
    if ((rc = check_geometry_frame(W, H, C, 5, image))) return rc;
    if ((rc = check_min_alpha(min_alpha))) return rc;
    if (!(percentile > 0.0 && percentile <= 100.0)) return fail(GSR_E_INVALID_ARG, "percentile = %g: must be in (0, 100]", percentile);
    if (!stats_out || !scratch) return fail(GSR_E_INVALID_ARG, "null stats_out or scratch");
    if ((uintptr_t)scratch % 8) return fail(GSR_E_INVALID_ARG, "scratch must be 8-byte aligned");
    gsr_launch_depth_scale((hipStream_t)stream, W, H, C, image, min_alpha, percentile, stats_out, scratch);
    return launched();
}

int gsr_frame_depth16(int32_t W, int32_t H, int32_t C, const float* image, int32_t expected, float min_alpha, float depth_max,
                      const float* scale_dev, int32_t flip_rows, uint16_t* depth16_out, void* stream) {
    int rc;
    if ((rc = check_geometry_frame(W, H, C, expected ? 5 : 4, image))) return rc;
    if ((rc = check_min_alpha(min_alpha))) return rc;
    if (!(depth_max >= 0.0f) || std::isinf(depth_max))
        return fail(GSR_E_INVALID_ARG, "depth_max = %g: must be finite and >= 0", (double)depth_max);
    if ((depth_max > 0.0f) == (scale_dev != nullptr))
        return fail(GSR_E_INVALID_ARG, "exactly one of depth_max > 0 and scale_dev: %s given", scale_dev ? "both" : "neither");
    if (!depth16_out) return fail(GSR_E_INVALID_ARG, "null depth16_out");
    if ((uintptr_t)depth16_out % 2) return fail(GSR_E_INVALID_ARG, "depth16_out must be 2-byte aligned");
    gsr_launch_frame_depth16((hipStream_t)stream, W, H, C, image, expected != 0, min_alpha, depth_max, scale_dev, flip_rows != 0,
                             depth16_out);
    return launched();
}

int gsr_frame_normal8(int32_t W, int32_t H, int32_t C, const float* image, float min_alpha, const float* R_c2w,
                      uint8_t* normal8_out, void* stream) {
    int rc;
    if ((rc = check_geometry_frame(W, H, C, 8, image))) return rc;
    if ((rc = check_min_alpha(min_alpha))) return rc;
    if (!normal8_out) return fail(GSR_E_INVALID_ARG, "null normal8_out");
    GsrRot rot = {};
    if (R_c2w) {
        std::copy(R_c2w, R_c2w + 9, rot.r);
        rot.use = 1;
    }
    gsr_launch_frame_normal8((hipStream_t)stream, W, H, C, image, min_alpha, rot, normal8_out);
    return launched();
}

int gsr_pick_point(int32_t W, int32_t H, int32_t C, const float* image, const gsr_camera* cam, int32_t px, int32_t py,
                   int32_t half_window, float* out4, void* stream) {
    int rc;
    if ((rc = check_geometry_frame(W, H, C, 4, image))) return rc;
    if (half_window < 0 || half_window > 16) return fail(GSR_E_INVALID_ARG, "half_window = %d: must be in [0, 16]", half_window);
    if (!cam || !out4) return fail(GSR_E_INVALID_ARG, "null cam or out4");
    GsrPickCam pc;
    std::copy(cam->R, cam->R + 9, pc.R);
    std::copy(cam->camera_center, cam->camera_center + 3, pc.center);
    std::copy(cam->focal, cam->focal + 2, pc.focal);
    std::copy(cam->principal, cam->principal + 2, pc.principal);
    gsr_launch_pick_point((hipStream_t)stream, W, H, C, image, pc, px, py, half_window, out4);
    return launched();
}

int gsr_densify_grad_mean(int64_t n, const float* accum, const float* denom, float* grad_out, void* stream) {
    if (n < 0) return fail(GSR_E_INVALID_ARG, "negative n");
    if (n == 0) return GSR_OK;
    if (!accum || !denom || !grad_out) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_grad_mean((hipStream_t)stream, n, accum, denom, grad_out);
    return launched();
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
    return launched();
}

int gsr_contribution_mask(int64_t n, int rule, double threshold, const uint32_t* max_weight, const uint64_t* hits,
                          const uint64_t* weight_sum, uint8_t* valid_out, void* stream) {
    if (rule < GSR_SCORE_MAX_WEIGHT || rule > GSR_SCORE_HITS) return fail(GSR_E_INVALID_ARG, "unknown score rule %d", rule);
    if (n < 0) return fail(GSR_E_INVALID_ARG, "negative n");
    if (!(threshold >= 0.0) || !std::isfinite(threshold)) return fail(GSR_E_INVALID_ARG, "threshold must be finite and >= 0");
    // the threshold in the score's own integers (gsr.h): the bits of the fp32 threshold | ceil(t · 2^24) | ceil(t)
    unsigned long long thr;
    const void* score;
    if (rule == GSR_SCORE_MAX_WEIGHT) {
        const float t = (float)threshold;
        if (!std::isfinite(t)) return fail(GSR_E_INVALID_ARG, "threshold does not fit fp32");
        uint32_t bits;
        __builtin_memcpy(&bits, &t, 4);
        thr = bits;
        score = max_weight;
    } else {
        const double t = std::ceil(rule == GSR_SCORE_WEIGHT_SUM ? threshold * 16777216.0 : threshold);
        if (!(t < 18446744073709551616.0)) return fail(GSR_E_INVALID_ARG, "threshold beyond 64 bits");
        thr = (unsigned long long)t;
        score = rule == GSR_SCORE_WEIGHT_SUM ? (const void*)weight_sum : (const void*)hits;
    }
    if (n == 0) return GSR_OK;
    if (!score || !valid_out) return fail(GSR_E_INVALID_ARG, "null array");
    if ((uintptr_t)score % (rule == GSR_SCORE_MAX_WEIGHT ? 4 : 8))
        return fail(GSR_E_INVALID_ARG, "max_weight must be 4-byte, hits and weight_sum 8-byte aligned");
    gsr_launch_contribution_mask((hipStream_t)stream, n, rule == GSR_SCORE_MAX_WEIGHT ? 1 : 2, score, thr, valid_out);
    return launched();
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
    return launched();
}

int gsr_split_transform(int64_t n_new, int32_t scale_dims, float* points, const float* rotations, float* scales, uint32_t seed,
                        void* stream) {
    if (n_new < 0 || (scale_dims != 1 && scale_dims != 3)) return fail(GSR_E_INVALID_ARG, "bad sizes");
    if (n_new == 0) return GSR_OK;  // densification.jl:94 `if n_new_points > 0`
    if (!points || !rotations || !scales) return fail(GSR_E_INVALID_ARG, "null array");
    if (((uintptr_t)rotations & 15) != 0) return fail(GSR_E_INVALID_ARG, "rotations must be 16-byte aligned");
    gsr_launch_split_transform((hipStream_t)stream, n_new, scale_dims, points, rotations, scales, seed);
    return launched();
}

int gsr_reset_opacity(int64_t n, float* opacities, void* stream) {
    if (n < 0) return fail(GSR_E_INVALID_ARG, "negative n");
    if (n == 0) return GSR_OK;
    if (!opacities) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_reset_opacity((hipStream_t)stream, n, opacities);
    return launched();
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
    return launched();
}

size_t gsr_mcmc_sample_scratch_bytes(int64_t n) { return gsr_mcmc_sample_scratch_words(n) * sizeof(uint64_t); }

int gsr_mcmc_sample(int64_t n, const uint32_t* q, int64_t m, uint32_t seed, uint32_t* sampled, int32_t* counts, uint64_t* total,
                    void* scratch, size_t scratch_bytes, void* stream) {
    if (n < 0 || m < 0) return fail(GSR_E_INVALID_ARG, "negative count: n=%lld m=%lld", (long long)n, (long long)m);
    if (n > 0xFFFFFFFFll || m > 0xFFFFFFFFll) return fail(GSR_E_INVALID_ARG, "rows and draws are indexed with 32 bits");
    if (m == 0) return GSR_OK;
    if (!total) return fail(GSR_E_INVALID_ARG, "null total");
    if (n > 0 && (!q || !sampled || !counts || !scratch)) return fail(GSR_E_INVALID_ARG, "null array");
    if (int rc = check_scratch(scratch_bytes, gsr_mcmc_sample_scratch_bytes(n), "sampler")) return rc;
    if ((((uintptr_t)scratch | (uintptr_t)total) & 7) != 0) return fail(GSR_E_INVALID_ARG, "scratch and total must be 8-byte aligned");
    gsr_launch_mcmc_sample((hipStream_t)stream, n, q, m, seed, sampled, counts, reinterpret_cast<unsigned long long*>(total),
                           reinterpret_cast<unsigned long long*>(scratch));
    return launched();
}

int gsr_mcmc_split_sampled(int64_t n, int32_t scale_dims, const int32_t* counts, const float* binoms, int32_t n_max,
                           float min_opacity, float* opacities_raw, float* scales_raw, void* stream) {
    int rc;
    if ((rc = check_mcmc_rows(n, scale_dims))) return rc;
    if (n_max < 1) return fail(GSR_E_INVALID_ARG, "n_max = %d: at least 1", n_max);
    if (n == 0) return GSR_OK;
    if (!counts || !binoms || !opacities_raw || !scales_raw) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_mcmc_split_sampled((hipStream_t)stream, n, scale_dims, counts, binoms, n_max, min_opacity, opacities_raw, scales_raw);
    return launched();
}

int gsr_mcmc_relocation_params(int64_t m, const float* o, const int32_t* ratio, const float* binoms, int32_t n_max,
                               float min_opacity, float* new_o, float* coeff, void* stream) {
    if (m < 0) return fail(GSR_E_INVALID_ARG, "negative m");
    if (n_max < 1) return fail(GSR_E_INVALID_ARG, "n_max = %d: at least 1", n_max);
    if (m == 0) return GSR_OK;
    if (!o || !ratio || !binoms || !new_o || !coeff) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_mcmc_relocation_params((hipStream_t)stream, m, o, ratio, binoms, n_max, min_opacity, new_o, coeff);
    return launched();
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
    return launched();
}

int gsr_mcmc_inject_noise(int64_t n, int32_t scale_dims, float* points, const float* opacities_raw, const float* scales_raw,
                          const float* rotations, float lr, float max_kick, uint32_t seed, void* stream) {
    int rc;
    if ((rc = check_mcmc_rows(n, scale_dims))) return rc;
    if (n == 0) return GSR_OK;  // mcmc.jl:292
    if (!points || !opacities_raw || !scales_raw || !rotations) return fail(GSR_E_INVALID_ARG, "null array");
    if (((uintptr_t)rotations & 15) != 0) return fail(GSR_E_INVALID_ARG, "rotations must be 16-byte aligned");
    gsr_launch_mcmc_inject_noise((hipStream_t)stream, n, scale_dims, points, opacities_raw, scales_raw, rotations, lr, max_kick, seed);
    return launched();
}

size_t gsr_mcmc_regularization_scratch_bytes(int64_t n) { return gsr_mcmc_regularization_scratch_floats(n) * sizeof(float); }

int gsr_mcmc_regularization(int64_t n, int32_t scale_dims, const float* opacities_raw, const float* scales_raw, float opacity_reg,
                            float scale_reg, float* loss_out, float* vopacities, float* vscales, void* scratch,
                            size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_mcmc_rows(n, scale_dims))) return rc;
    if (!loss_out || (n > 0 && (!opacities_raw || !scales_raw || !scratch))) return fail(GSR_E_INVALID_ARG, "null array");
    if ((rc = check_scratch(scratch_bytes, gsr_mcmc_regularization_scratch_bytes(n), "regulariser"))) return rc;
    gsr_launch_mcmc_regularization((hipStream_t)stream, n, scale_dims, opacities_raw, scales_raw, opacity_reg, scale_reg, loss_out,
                                   vopacities, vscales, (float*)scratch);
    return launched();
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
    return launched();
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
    return launched();
}

// ---- the 3-D smoothing filter: camera sweep, apply, pullback (filter3d.hip; Mip-Splatting §4.1) ----
static int check_filter3d_rows(int64_t n) {
    if (n < 0) return fail(GSR_E_INVALID_ARG, "negative n");
    if (n > 0x7FFFFFFFll) return fail(GSR_E_INVALID_ARG, "n = %lld: rows are indexed with 31 bits", (long long)n);
    return GSR_OK;
}

size_t gsr_filter3d_scratch_bytes(int64_t n) {
    if (n <= 0 || n > 0x7FFFFFFFll) return 0;
    return gsr_filter3d_scratch_size(n);
}

int gsr_filter3d_compute(int64_t n, const float* points, int32_t n_cameras, const float* camera_table, float near_plane, float k,
                         float* filter, uint8_t* seen, uint32_t* count, void* scratch, size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_filter3d_rows(n))) return rc;
    if (n_cameras < 1) return fail(GSR_E_INVALID_ARG, "n_cameras = %d: the sweep needs at least one camera", n_cameras);
    if (!(near_plane >= 0.0f) || !(k >= 0.0f))
        return fail(GSR_E_INVALID_ARG, "near_plane = %g, k = %g: neither may be negative or NaN", (double)near_plane, (double)k);
    if (n == 0) return GSR_OK;
    if (!points || !camera_table || !filter || !scratch) return fail(GSR_E_INVALID_ARG, "null points, camera_table, filter or scratch");
    if ((rc = check_scratch(scratch_bytes, gsr_filter3d_scratch_bytes(n), "camera sweep"))) return rc;
    if ((uintptr_t)scratch % 8) return fail(GSR_E_INVALID_ARG, "scratch must be 8-byte aligned");
    gsr_launch_filter3d_compute((hipStream_t)stream, n, points, n_cameras, camera_table, near_plane, k, filter, seen, count, scratch);
    return launched();
}

int gsr_filter3d_apply(int64_t n, const float* opacities_act, const float* scales_act, const float* filter, int32_t raw,
                       float* opacities_out, float* scales_out, void* stream) {
    int rc;
    if ((rc = check_filter3d_rows(n))) return rc;
    if (n == 0) return GSR_OK;
    if (!opacities_act || !scales_act || !filter || !opacities_out || !scales_out) return fail(GSR_E_INVALID_ARG, "null array");
    if (opacities_out == opacities_act || scales_out == scales_act) return fail(GSR_E_INVALID_ARG, "the outputs must not be the inputs");
    gsr_launch_filter3d_apply((hipStream_t)stream, n, opacities_act, scales_act, filter, raw != 0, opacities_out, scales_out);
    return launched();
}

int gsr_filter3d_apply_backward(int64_t n, const float* opacities_act, const float* scales_act, const float* filter,
                                const float* g_opacities, const float* g_scales, float* v_opacities, float* v_scales, void* stream) {
    int rc;
    if ((rc = check_filter3d_rows(n))) return rc;
    if (n == 0) return GSR_OK;
    if (!opacities_act || !scales_act || !filter || !g_opacities || !g_scales || !v_opacities || !v_scales)
        return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_filter3d_apply_bwd((hipStream_t)stream, n, opacities_act, scales_act, filter, g_opacities, g_scales, v_opacities,
                                  v_scales);
    return launched();
}

// ---- SH codebook compression: exact k-means, the nearest-code search on the f32 MFMA (vq.hip) ----
static int check_vq_shape(int64_t n, int32_t n_codes, int32_t dim) {
    if (n < 0 || n >= (1ll << 24)) return fail(GSR_E_INVALID_ARG, "n = %lld: 0 <= n < 2^24 rows", (long long)n);
    if (n_codes < 1 || n_codes > 65536) return fail(GSR_E_INVALID_ARG, "n_codes = %d: 1 .. 65536 (indices are uint16)", n_codes);
    if (dim < 1 || dim > 48) return fail(GSR_E_INVALID_ARG, "dim = %d: 1 .. 48", dim);
    return GSR_OK;
}

size_t gsr_vq_scratch_bytes(int64_t n, int32_t n_codes, int32_t dim) {
    if (n <= 0 || n >= (1ll << 24) || n_codes < 1 || n_codes > 65536 || dim < 1 || dim > 48) return 0;
    return gsr_vq_scratch_size(n_codes, dim);
}

int gsr_vq_assign(int64_t n, int32_t n_codes, int32_t dim, const float* rows, const float* codebook, const uint16_t* prev,
                  uint16_t* indices, float* err, uint32_t* changed, void* scratch, size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_vq_shape(n, n_codes, dim))) return rc;
    if (n == 0) return GSR_OK;
    if (!rows || !codebook || !indices || !scratch) return fail(GSR_E_INVALID_ARG, "null rows, codebook, indices or scratch");
    if ((uintptr_t)indices % 2 || (uintptr_t)prev % 2) return fail(GSR_E_INVALID_ARG, "indices and prev must be 2-byte aligned");
    if ((uintptr_t)changed % 4) return fail(GSR_E_INVALID_ARG, "changed must be 4-byte aligned");
    if ((rc = check_scratch(scratch_bytes, gsr_vq_scratch_bytes(n, n_codes, dim), "nearest-code search"))) return rc;
    if ((uintptr_t)scratch % 16) return fail(GSR_E_INVALID_ARG, "scratch must be 16-byte aligned");
    gsr_launch_vq_assign((hipStream_t)stream, (int)n, n_codes, dim, rows, codebook, prev, indices, err, changed, scratch);
    return launched();
}

int gsr_vq_accumulate(int64_t n, int32_t n_codes, int32_t dim, const float* rows, const uint16_t* indices, const uint8_t* wq,
                      int64_t* sums, uint64_t* wsum, void* stream) {
    int rc;
    if ((rc = check_vq_shape(n, n_codes, dim))) return rc;
    if (n == 0) return GSR_OK;
    if (!rows || !indices || !sums || !wsum) return fail(GSR_E_INVALID_ARG, "null rows, indices, sums or wsum");
    if ((uintptr_t)indices % 2) return fail(GSR_E_INVALID_ARG, "indices must be 2-byte aligned");
    if ((uintptr_t)sums % 8 || (uintptr_t)wsum % 8) return fail(GSR_E_INVALID_ARG, "sums and wsum must be 8-byte aligned");
    gsr_launch_vq_accumulate((hipStream_t)stream, (int)n, n_codes, dim, rows, indices, wq, reinterpret_cast<long long*>(sums),
                             reinterpret_cast<unsigned long long*>(wsum));
    return launched();
}

int gsr_vq_update(int32_t n_codes, int32_t dim, const int64_t* sums, const uint64_t* wsum, float* codebook, uint32_t* empty,
                  void* stream) {
    int rc;
    if ((rc = check_vq_shape(0, n_codes, dim))) return rc;
    if (!sums || !wsum || !codebook) return fail(GSR_E_INVALID_ARG, "null sums, wsum or codebook");
    if ((uintptr_t)sums % 8 || (uintptr_t)wsum % 8) return fail(GSR_E_INVALID_ARG, "sums and wsum must be 8-byte aligned");
    if ((uintptr_t)empty % 4) return fail(GSR_E_INVALID_ARG, "empty must be 4-byte aligned");
    gsr_launch_vq_update((hipStream_t)stream, n_codes, dim, reinterpret_cast<const long long*>(sums),
                         reinterpret_cast<const unsigned long long*>(wsum), codebook, empty);
    return launched();
}

int gsr_vq_decode(int64_t n, int32_t n_codes, int32_t dim, const float* codebook, const uint16_t* indices, float* rows_out,
                  void* stream) {
    int rc;
    if ((rc = check_vq_shape(n, n_codes, dim))) return rc;
    if (n == 0) return GSR_OK;
    if (!codebook || !indices || !rows_out) return fail(GSR_E_INVALID_ARG, "null codebook, indices or rows_out");
    if ((uintptr_t)indices % 2) return fail(GSR_E_INVALID_ARG, "indices must be 2-byte aligned");
    gsr_launch_vq_decode((hipStream_t)stream, (int)n, n_codes, dim, codebook, indices, rows_out);
    return launched();
}

// ---- SH codebook fine-tuning: rows grouped by code, fixed-order per-code gradient sums (vq_grad.hip) ----
size_t gsr_vq_group_scratch_bytes(int64_t n, int32_t n_codes) {
    if (n <= 0 || n >= (1ll << 24) || n_codes < 1 || n_codes > 65536) return 0;
    return gsr_vq_group_scratch_size(n, n_codes);
}

int gsr_vq_group(int64_t n, int32_t n_codes, const uint16_t* indices, uint32_t* order, uint32_t* offsets, void* scratch,
                 size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_vq_shape(n, n_codes, 1))) return rc;
    if (n == 0) return GSR_OK;
    if (!indices || !order || !offsets || !scratch) return fail(GSR_E_INVALID_ARG, "null indices, order, offsets or scratch");
    if ((uintptr_t)indices % 2) return fail(GSR_E_INVALID_ARG, "indices must be 2-byte aligned");
    if ((uintptr_t)order % 4 || (uintptr_t)offsets % 4) return fail(GSR_E_INVALID_ARG, "order and offsets must be 4-byte aligned");
    if ((rc = check_scratch(scratch_bytes, gsr_vq_group_scratch_bytes(n, n_codes), "grouping of the rows by code"))) return rc;
    if ((uintptr_t)scratch % 16) return fail(GSR_E_INVALID_ARG, "scratch must be 16-byte aligned");
    gsr_launch_vq_group((hipStream_t)stream, (int)n, n_codes, indices, order, offsets, scratch);
    return launched();
}

size_t gsr_vq_codebook_grad_scratch_bytes(int64_t n, int32_t n_codes, int32_t dim) {
    if (n <= 0 || n >= (1ll << 24) || n_codes < 1 || n_codes > 65536 || dim < 1 || dim > 48) return 0;
    return gsr_vq_codebook_grad_scratch_size(n, n_codes, dim);
}

int gsr_vq_codebook_grad(int64_t n, int32_t n_codes, int32_t dim, const float* g_rows, int64_t row_stride, const uint32_t* order,
                         const uint32_t* offsets, float* g_codebook, void* scratch, size_t scratch_bytes, void* stream) {
    int rc;
    if ((rc = check_vq_shape(n, n_codes, dim))) return rc;
    if (row_stride < dim) return fail(GSR_E_INVALID_ARG, "row_stride = %lld floats: at least dim = %d", (long long)row_stride, dim);
    if (n == 0) return GSR_OK;
    if (!g_rows || !order || !offsets || !g_codebook || !scratch)
        return fail(GSR_E_INVALID_ARG, "null g_rows, order, offsets, g_codebook or scratch");
    if ((uintptr_t)g_rows % 4 || (uintptr_t)g_codebook % 4) return fail(GSR_E_INVALID_ARG, "g_rows and g_codebook must be 4-byte aligned");
    if ((uintptr_t)order % 4 || (uintptr_t)offsets % 4) return fail(GSR_E_INVALID_ARG, "order and offsets must be 4-byte aligned");
    if ((rc = check_scratch(scratch_bytes, gsr_vq_codebook_grad_scratch_bytes(n, n_codes, dim), "per-code gradient sums"))) return rc;
    if ((uintptr_t)scratch % 16) return fail(GSR_E_INVALID_ARG, "scratch must be 16-byte aligned");
    gsr_launch_vq_codebook_grad((hipStream_t)stream, (int)n, n_codes, dim, g_rows, (long long)row_stride, order, offsets, g_codebook,
                                scratch);
    return launched();
}

// ---- the quantised model container: block ranges, 8/16-bit codes, the decode, the fake pass (quant.hip) ----
static int check_quant_shape(int64_t n, int32_t cols, int32_t block_rows) {
    if (n < 0 || n >= (1ll << 31)) return fail(GSR_E_INVALID_ARG, "n = %lld: 0 <= n < 2^31 rows", (long long)n);
    if (cols < 1 || cols > 48) return fail(GSR_E_INVALID_ARG, "cols = %d: 1 .. 48", cols);
    if (block_rows != 0 && (block_rows < 64 || block_rows > 1024 || block_rows % 64))
        return fail(GSR_E_INVALID_ARG, "block_rows = %d: 0, or a multiple of 64 in [64, 1024]", block_rows);
    return GSR_OK;
}

static int check_quant_code(int32_t cols, int32_t bits, int32_t kind) {
    if (bits < 1 || bits > 16) return fail(GSR_E_INVALID_ARG, "bits = %d: 1 .. 16", bits);
    if (kind != GSR_QUANT_LINEAR && kind != GSR_QUANT_UNIT_QUAT) return fail(GSR_E_INVALID_ARG, "kind = %d: GSR_QUANT_LINEAR or GSR_QUANT_UNIT_QUAT", kind);
    if (kind == GSR_QUANT_UNIT_QUAT && cols != 4) return fail(GSR_E_INVALID_ARG, "GSR_QUANT_UNIT_QUAT needs cols = 4, not %d", cols);
    return GSR_OK;
}

int gsr_quant_ranges(int64_t n, int32_t cols, const float* rows, int32_t block_rows, float* ranges, void* stream) {
    int rc;
    if ((rc = check_quant_shape(n, cols, block_rows))) return rc;
    if (n == 0 && block_rows != 0) return GSR_OK;
    if ((n > 0 && !rows) || !ranges) return fail(GSR_E_INVALID_ARG, "null rows or ranges");
    if ((uintptr_t)rows % 4 || (uintptr_t)ranges % 4) return fail(GSR_E_INVALID_ARG, "rows and ranges must be 4-byte aligned");
    gsr_launch_quant_ranges((hipStream_t)stream, n, cols, rows, block_rows, ranges);
    return launched();
}

int gsr_quant_encode(int64_t n, int32_t cols, int32_t bits, int32_t kind, const float* rows, int32_t block_rows, const float* ranges,
                     void* codes, void* stream) {
    int rc;
    if ((rc = check_quant_shape(n, cols, block_rows))) return rc;
    if ((rc = check_quant_code(cols, bits, kind))) return rc;
    if (n == 0) return GSR_OK;
    if (!rows || !codes || (kind == GSR_QUANT_LINEAR && !ranges)) return fail(GSR_E_INVALID_ARG, "null rows, codes or ranges");
    if ((uintptr_t)rows % 4 || (uintptr_t)ranges % 4) return fail(GSR_E_INVALID_ARG, "rows and ranges must be 4-byte aligned");
    if (bits > 8 && (uintptr_t)codes % 2) return fail(GSR_E_INVALID_ARG, "uint16 codes must be 2-byte aligned");
    gsr_launch_quant_encode((hipStream_t)stream, n, cols, bits, kind, rows, block_rows, ranges, codes);
    return launched();
}

int gsr_quant_decode(int64_t n, int32_t cols, int32_t bits, int32_t kind, const void* codes, int32_t block_rows, const float* ranges,
                     float* rows_out, void* stream) {
    int rc;
    if ((rc = check_quant_shape(n, cols, block_rows))) return rc;
    if ((rc = check_quant_code(cols, bits, kind))) return rc;
    if (n == 0) return GSR_OK;
    if (!codes || !rows_out || (kind == GSR_QUANT_LINEAR && !ranges)) return fail(GSR_E_INVALID_ARG, "null codes, rows_out or ranges");
    if ((uintptr_t)rows_out % 4 || (uintptr_t)ranges % 4) return fail(GSR_E_INVALID_ARG, "rows_out and ranges must be 4-byte aligned");
    if (bits > 8 && (uintptr_t)codes % 2) return fail(GSR_E_INVALID_ARG, "uint16 codes must be 2-byte aligned");
    gsr_launch_quant_decode((hipStream_t)stream, n, cols, bits, kind, codes, block_rows, ranges, rows_out);
    return launched();
}

int gsr_quant_fake(const gsr_quant_group* groups, int32_t n_groups, int64_t n, void* stream) {
    if (n_groups < 0 || n_groups > GSR_QUANT_MAX_GROUPS || (n_groups > 0 && !groups))
        return fail(GSR_E_INVALID_ARG, "n_groups must be in [0, %d]", GSR_QUANT_MAX_GROUPS);
    const float* in[GSR_QUANT_MAX_GROUPS]; float* out[GSR_QUANT_MAX_GROUPS]; const float* ranges[GSR_QUANT_MAX_GROUPS];
    int cols[GSR_QUANT_MAX_GROUPS], bits[GSR_QUANT_MAX_GROUPS], kind[GSR_QUANT_MAX_GROUPS], block_rows[GSR_QUANT_MAX_GROUPS];
    int rc;
    if (n_groups == 0 && (rc = check_quant_shape(n, 1, 0))) return rc;
    for (int g = 0; g < n_groups; g++) {
        const gsr_quant_group& a = groups[g];
        if ((rc = check_quant_shape(n, a.cols, a.block_rows))) return rc;
        if ((rc = check_quant_code(a.cols, a.bits, a.kind))) return rc;
        if (n > 0) {
            if (!a.rows_in || !a.rows_out || (a.kind == GSR_QUANT_LINEAR && !a.ranges)) return fail(GSR_E_INVALID_ARG, "group %d: null array", g);
            if ((uintptr_t)a.rows_in % 4 || (uintptr_t)a.rows_out % 4 || (uintptr_t)a.ranges % 4)
                return fail(GSR_E_INVALID_ARG, "group %d: the arrays must be 4-byte aligned", g);
        }
        in[g] = a.rows_in; out[g] = a.rows_out; ranges[g] = a.ranges;
        cols[g] = a.cols; bits[g] = a.bits; kind[g] = a.kind; block_rows[g] = a.block_rows;
    }
    if (n == 0 || n_groups == 0) return GSR_OK;
    gsr_launch_quant_fake((hipStream_t)stream, n_groups, n, in, out, ranges, cols, bits, kind, block_rows);
    return launched();
}

// ---- TSDF fusion of rendered depth and surface-nets mesh extraction (tsdf.hip) ----
namespace {
constexpr int kTsdfMaxDim = 65535;              // a (j, k) row is one workgroup row of the launch grid
constexpr long long kMeshMaxSamples = 1ll << 30;  // vertex ids are int32, 3 quads per sample are counted in 32 bits

int check_tsdf_grid(int32_t nx, int32_t ny, int32_t nz, const void* volume) {
    if (nx < 1 || ny < 1 || nz < 1) return fail(GSR_E_INVALID_ARG, "volume of %d x %d x %d samples: every side must be >= 1", nx, ny, nz);
    if (nx > kTsdfMaxDim || ny > kTsdfMaxDim || nz > kTsdfMaxDim)
        return fail(GSR_E_INVALID_ARG, "volume of %d x %d x %d samples: a side may not exceed %d", nx, ny, nz, kTsdfMaxDim);
    if (!volume) return fail(GSR_E_INVALID_ARG, "null volume");
    if ((uintptr_t)volume % 8) return fail(GSR_E_INVALID_ARG, "the volume must be 8-byte aligned: {tsdf, weight} pairs");
    return GSR_OK;
}
int check_mesh_grid(int32_t nx, int32_t ny, int32_t nz, const void* volume) {
    if (int rc = check_tsdf_grid(nx, ny, nz, volume)) return rc;
    if ((long long)nx * ny * nz > kMeshMaxSamples)
        return fail(GSR_E_INVALID_ARG, "volume of %d x %d x %d samples: the extraction indexes at most 2^30", nx, ny, nz);
    return GSR_OK;
}
int check_mesh_scratch(int32_t nx, int32_t ny, int32_t nz, const void* scratch, size_t scratch_bytes) {
    const size_t need = gsr_mesh_scratch_size(nx, ny, nz);
    if (need == 0) return GSR_OK;   // no cell: nothing is launched, nothing is touched
    if (!scratch) return fail(GSR_E_INVALID_ARG, "null scratch");
    if (int rc = check_scratch(scratch_bytes, need, "mesh extraction")) return rc;
    if ((uintptr_t)scratch % 8) return fail(GSR_E_INVALID_ARG, "scratch must be 8-byte aligned");
    return GSR_OK;
}
GsrTsdfGrid tsdf_grid(int32_t nx, int32_t ny, int32_t nz, const float* origin, float h) {
    GsrTsdfGrid g = {nx, ny, nz, {0.0f, 0.0f, 0.0f}, h};
    if (origin) std::copy(origin, origin + 3, g.o);
    return g;
}
}  // namespace

int gsr_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, const float* origin, float voxel_size, float trunc, int32_t W, int32_t H,
                       int32_t C, const float* image, const gsr_camera* cam, float min_alpha, float near_plane, float* volume,
                       float* color, void* stream) {
    int rc;
    if ((rc = check_tsdf_grid(nx, ny, nz, volume))) return rc;
    if (!origin || !cam) return fail(GSR_E_INVALID_ARG, "null origin or cam");
    if (!(voxel_size > 0.0f) || !std::isfinite(voxel_size)) return fail(GSR_E_INVALID_ARG, "voxel_size = %g: must be finite and > 0", (double)voxel_size);
    if (!(trunc > 0.0f) || !std::isfinite(trunc)) return fail(GSR_E_INVALID_ARG, "trunc = %g: must be finite and > 0", (double)trunc);
    if ((rc = check_geometry_frame(W, H, C, 5, image))) return rc;
    if ((rc = check_min_alpha(min_alpha))) return rc;
    if (std::isnan(near_plane)) return fail(GSR_E_INVALID_ARG, "near_plane is NaN");
    if (!(cam->focal[0] > 0.0f) || !(cam->focal[1] > 0.0f)) return fail(GSR_E_INVALID_ARG, "focal lengths must be positive");
    GsrTsdfCam c;
    std::copy(cam->R, cam->R + 9, c.R);
    std::copy(cam->t, cam->t + 3, c.t);
    c.fx = cam->focal[0];
    c.fy = cam->focal[1];
    c.cx = cam->principal[0] * (float)W;
    c.cy = cam->principal[1] * (float)H;
    gsr_launch_tsdf_integrate((hipStream_t)stream, tsdf_grid(nx, ny, nz, origin, voxel_size), c, W, H, C, image, min_alpha,
                              near_plane, trunc, volume, color);
    return launched();
}

size_t gsr_mesh_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (nx < 1 || ny < 1 || nz < 1 || nx > kTsdfMaxDim || ny > kTsdfMaxDim || nz > kTsdfMaxDim ||
        (long long)nx * ny * nz > kMeshMaxSamples)
        return 0;
    return gsr_mesh_scratch_size(nx, ny, nz);
}

int gsr_mesh_count(int32_t nx, int32_t ny, int32_t nz, const float* volume, uint32_t* counts, void* scratch, size_t scratch_bytes,
                   void* stream) {
    int rc;
    if ((rc = check_mesh_grid(nx, ny, nz, volume))) return rc;
    if (!counts) return fail(GSR_E_INVALID_ARG, "null counts");
    if ((rc = check_mesh_scratch(nx, ny, nz, scratch, scratch_bytes))) return rc;
    gsr_launch_mesh_count((hipStream_t)stream, tsdf_grid(nx, ny, nz, nullptr, 0.0f), volume, counts, scratch);
    return launched();
}

int gsr_mesh_emit(int32_t nx, int32_t ny, int32_t nz, const float* origin, float voxel_size, const float* volume, const float* color,
                  const void* scratch, size_t scratch_bytes, int64_t max_vertices, int64_t max_faces, float* vertices,
                  float* vertex_colors, int32_t* faces, void* stream) {
    int rc;
    if ((rc = check_mesh_grid(nx, ny, nz, volume))) return rc;
    if (!origin) return fail(GSR_E_INVALID_ARG, "null origin");
    if (!(voxel_size > 0.0f) || !std::isfinite(voxel_size)) return fail(GSR_E_INVALID_ARG, "voxel_size = %g: must be finite and > 0", (double)voxel_size);
    if (max_vertices < 0 || max_faces < 0) return fail(GSR_E_INVALID_ARG, "negative capacity");
    if ((max_vertices > 0 && !vertices) || (max_faces > 0 && !faces)) return fail(GSR_E_INVALID_ARG, "null vertices or faces");
    if ((color != nullptr) != (vertex_colors != nullptr) && max_vertices > 0)
        return fail(GSR_E_INVALID_ARG, "color and vertex_colors go together: %s given", color ? "only color" : "only vertex_colors");
    if ((rc = check_mesh_scratch(nx, ny, nz, scratch, scratch_bytes))) return rc;
    if (max_vertices == 0 && max_faces == 0) return GSR_OK;
    gsr_launch_mesh_emit((hipStream_t)stream, tsdf_grid(nx, ny, nz, origin, voxel_size), volume, color, scratch, max_vertices,
                         max_faces, vertices, vertex_colors, faces);
    return launched();
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
    return launched();
}

static int ply_rows(bool pack, int64_t n, int32_t k_rest, const float* points, const float* dc, const float* rest,
                    const float* opac, const float* scales, const float* rots, const float* rows, void* stream) {
    if (n < 0 || k_rest < 0) return fail(GSR_E_INVALID_ARG, "bad sizes: n=%lld k_rest=%d", (long long)n, k_rest);
    if (n == 0) return GSR_OK;
    if (!points || !dc || (k_rest > 0 && !rest) || !opac || !scales || !rots || !rows) return fail(GSR_E_INVALID_ARG, "null array");
    gsr_launch_ply_rows((hipStream_t)stream, pack, n, k_rest, const_cast<float*>(points), const_cast<float*>(dc),
                        const_cast<float*>(rest), const_cast<float*>(opac), const_cast<float*>(scales), const_cast<float*>(rots),
                        const_cast<float*>(rows));
    return launched();
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
    return launched();
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
    return launched();
}

int gsr_stream_triad(float* a, const float* b, const float* c, size_t count, float q, void* stream) {
    if (!a || !b || !c) return fail(GSR_E_INVALID_ARG, "null array");
    if (count % 4 != 0 || (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) != 0)
        return fail(GSR_E_INVALID_ARG, "count must be a multiple of 4 and the arrays 16-byte aligned");
    gsr_launch_triad((hipStream_t)stream, count / 4, a, b, c, q);
    return launched();
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
