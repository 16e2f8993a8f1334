"""Numpy restatement of src/geometry_regularization.jl (depth_normal_consistency_loss and flatten_loss with their
gradients), written from the reference's semantics in the package's layout: the frame is (H, W, 8), channels 3 = blended
depth D, 4 = alpha, 5..7 = the blended normal; x is the width index.

Which centres are valid is decided in float32 with the reference's own expressions (an IEEE division for e = D/α,
jump = 0.05f·e_c, |e_n - e_c| <= jump, α >= 0.5, isfinite(e_c), e_c >= 1e-6, |n|² >= 1e-24, |nr|² >= 0.1f²): the mask
is a function of the inputs.  Every product and sum after it is float64.

One intended deviation: a centre with w = 0 contributes exactly nothing to the loss and the gradients,
even when its stencil holds NaN / Inf (the reference's `sum(w .* (1 .- cosθ))` would turn NaN on 0 · NaN)."""
import numpy as np

F = np.float32
MIN_ALPHA, MAX_REL_JUMP, MIN_DEPTH, MIN_RENDER_NORM = F(0.5), F(0.05), F(1e-6), F(0.1)
MIN_COUNT, MIN_WEIGHT, MIN_CROSS_SQ = 64.0, 16.0, F(1e-24)


def pixel_rays(W, H, focal, principal=(0.5, 0.5), dtype=np.float32):
    """pixel_rays (geometry_regularization.jl:53-62): rx[x] = (x + 0.5 - principal_x·W) / fx for the 0-based x, evaluated
    in float32 as the reference does; `dtype` is what the result is handed on as."""
    cx, cy = F(principal[0]) * F(W), F(principal[1]) * F(H)
    rx = (np.arange(W, dtype=F) + F(0.5) - cx) / F(focal[0])
    ry = (np.arange(H, dtype=F) + F(0.5) - cy) / F(focal[1])
    return rx.astype(dtype), ry.astype(dtype)


def _max_keep_nan(a, b):
    """Julia's max: a NaN operand gives NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a), a, np.where(a < b, b, a)).astype(a.dtype)


def expected_depth32(image):
    """e = max(D, 0) / max(α, 1e-6) in float32 (H, W)."""
    D, A = image[..., 3].astype(F), image[..., 4].astype(F)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (_max_keep_nan(D, F(0)) / _max_keep_nan(A, MIN_DEPTH)).astype(F)


def _stencil(a):
    """(centre, x+1, x-1, y+1, y-1) views of the interior of an (H, W) array."""
    return a[1:-1, 1:-1], a[1:-1, 2:], a[1:-1, :-2], a[2:, 1:-1], a[:-2, 1:-1]


def _tangents(e, rx, ry):
    """Tangents and cross product over the interior, in the dtype of `e`, in the reference's order of operations."""
    e_c, e_xp, e_xm, e_yp, e_ym = _stencil(e)
    rx_c, rx_p, rx_m = rx[None, 1:-1], rx[None, 2:], rx[None, :-2]
    ry_c, ry_p, ry_m = ry[1:-1, None], ry[2:, None], ry[:-2, None]
    dx, dy = e_xp - e_xm, e_yp - e_ym
    tx = (e_xp * rx_p - e_xm * rx_m, dx * ry_c, dx + 0 * ry_c)
    ty = (dy * rx_c, e_yp * ry_p - e_ym * ry_m, dy + 0 * rx_c)
    n = (tx[1] * ty[2] - tx[2] * ty[1], tx[2] * ty[0] - tx[0] * ty[2], tx[0] * ty[1] - tx[1] * ty[0])
    return tx, ty, n, (rx_c, rx_p, rx_m, ry_c, ry_p, ry_m)


def valid_mask(image, focal, principal=(0.5, 0.5)):
    """The detached validity mask of the interior centres, (H-2, W-2) bool, and the weight map (H, W) float32 (α_c clamped
    to [0, 1] where valid, 0 elsewhere and on the border) — all decisions in float32."""
    H, W = image.shape[:2]
    wmap = np.zeros((H, W), F)
    if W <= 2 or H <= 2:
        return np.zeros((max(H - 2, 0), max(W - 2, 0)), bool), wmap
    img = image.astype(F)
    e = expected_depth32(img)
    rx, ry = pixel_rays(W, H, focal, principal)
    with np.errstate(invalid="ignore", over="ignore"):
        _, _, n, _ = _tangents(e, rx, ry)
        n_sq = (n[0] * n[0] + n[1] * n[1] + n[2] * n[2]).astype(F)
        nr = [img[1:-1, 1:-1, 5 + k] for k in range(3)]
        nr_sq = (nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]).astype(F)
        a = [s >= MIN_ALPHA for s in _stencil(img[..., 4])]
        opaque = a[0] & a[1] & a[2] & a[3] & a[4]
        e_c, e_xp, e_xm, e_yp, e_ym = _stencil(e)
        jump = (MAX_REL_JUMP * e_c).astype(F)
        cont = (e_c >= MIN_DEPTH) & (np.abs(e_xp - e_c) <= jump) & (np.abs(e_xm - e_c) <= jump) & \
               (np.abs(e_yp - e_c) <= jump) & (np.abs(e_ym - e_c) <= jump)
        ok = opaque & cont & np.isfinite(e_c) & (n_sq >= MIN_CROSS_SQ) & (nr_sq >= MIN_RENDER_NORM * MIN_RENDER_NORM)
    wmap[1:-1, 1:-1] = np.where(ok, np.clip(img[1:-1, 1:-1, 4], F(0), F(1)), F(0))
    return ok, wmap


def depth_normal(image, focal, principal=(0.5, 0.5), weight=1.0, skip=None):
    """-> dict(loss, sum_w, count, weights (H, W) float32, valid (H-2, W-2), n_sq, nr_sq (float32, of the interior),
    one_minus_cos (H-2, W-2) float64, 0 on invalid centres,
    vimage (H, W, 8) float64: weight · ∂loss/∂(D, α, normal) on channels 3..7, zeros elsewhere).
    `skip` (H-2, W-2) bool: centres to leave out on top of the mask (for tests)."""
    H, W = image.shape[:2]
    vimage = np.zeros((H, W, 8), np.float64)
    ok, wmap = valid_mask(image, focal, principal)
    out = dict(loss=0.0, sum_w=0.0, count=0, weights=wmap, valid=ok, vimage=vimage, n_sq=None, nr_sq=None)
    if W <= 2 or H <= 2:
        return out
    if skip is not None:
        ok = ok & ~skip
        wmap = wmap.copy()
        wmap[1:-1, 1:-1][~ok] = 0
        out.update(valid=ok, weights=wmap)
    img32 = image.astype(F)
    rx32, ry32 = pixel_rays(W, H, focal, principal)
    with np.errstate(invalid="ignore", over="ignore"):
        _, _, n32, _ = _tangents(expected_depth32(img32), rx32, ry32)
        out["n_sq"] = (n32[0] * n32[0] + n32[1] * n32[1] + n32[2] * n32[2]).astype(F)
        out["nr_sq"] = sum(img32[1:-1, 1:-1, 5 + k] * img32[1:-1, 1:-1, 5 + k] for k in range(3)).astype(F)
    w = wmap[1:-1, 1:-1].astype(np.float64)
    count, sum_w = int(ok.sum()), float(w.sum())
    out.update(sum_w=sum_w, count=count)
    # float64 from here on; invalid centres are neutralised BEFORE any arithmetic (the deviation above)
    img = image.astype(np.float64)
    D, A = img[..., 3], img[..., 4]
    okp = np.zeros((H, W), bool)   # pixels in the stencil of a valid centre: everything there is finite
    okp[1:-1, 1:-1] |= ok; okp[1:-1, 2:] |= ok; okp[1:-1, :-2] |= ok; okp[2:, 1:-1] |= ok; okp[:-2, 1:-1] |= ok
    D = np.where(okp, D, 1.0)
    A = np.where(okp, A, 1.0)
    e = np.maximum(D, 0.0) / np.maximum(A, 1e-6)
    rx, ry = pixel_rays(W, H, focal, principal, np.float64)
    tx, ty, n, (rx_c, rx_p, rx_m, ry_c, ry_p, ry_m) = _tangents(e, rx, ry)
    nr = [np.where(ok, img[1:-1, 1:-1, 5 + k], 1.0) for k in range(3)]
    n = [np.where(ok, c, 1.0) for c in n]
    n_sq = n[0] ** 2 + n[1] ** 2 + n[2] ** 2
    nr_sq = nr[0] ** 2 + nr[1] ** 2 + nr[2] ** 2
    n_norm, nr_norm = np.sqrt(n_sq), np.sqrt(nr_sq)
    facing = n[0] * rx_c + n[1] * ry_c + n[2]
    flip = np.where(facing > 0, -1.0, 1.0) / n_norm
    nd = [c * flip for c in n]
    cos = (nd[0] * nr[0] + nd[1] * nr[1] + nd[2] * nr[2]) / nr_norm
    out["one_minus_cos"] = np.where(ok, 1.0 - cos, 0.0)
    if not (count >= MIN_COUNT and sum_w >= MIN_WEIGHT):
        return out
    norm = max(sum_w, 1.0)
    out["loss"] = weight * float((w * (1.0 - cos)).sum() / norm)
    k = weight * w / norm                                  # ∂loss/∂(1 - cos) per centre
    # ∂(1 - cos)/∂nr and ∂(1 - cos)/∂n
    for c in range(3):
        vimage[1:-1, 1:-1, 5 + c] = k * (cos / nr_sq * nr[c] - nd[c] / nr_norm)
    p = (n[0] * nr[0] + n[1] * nr[1] + n[2] * nr[2]) / n_sq
    s = flip / nr_norm
    g = [-s * (nr[c] - p * n[c]) * k for c in range(3)]
    gtx = (ty[1] * g[2] - ty[2] * g[1], ty[2] * g[0] - ty[0] * g[2], ty[0] * g[1] - ty[1] * g[0])
    gty = (g[1] * tx[2] - g[2] * tx[1], g[2] * tx[0] - g[0] * tx[2], g[0] * tx[1] - g[1] * tx[0])
    ge = np.zeros((H, W), np.float64)
    ge[1:-1, 2:] += gtx[0] * rx_p + gtx[1] * ry_c + gtx[2]
    ge[1:-1, :-2] -= gtx[0] * rx_m + gtx[1] * ry_c + gtx[2]
    ge[2:, 1:-1] += gty[0] * rx_c + gty[1] * ry_p + gty[2]
    ge[:-2, 1:-1] -= gty[0] * rx_c + gty[1] * ry_m + gty[2]
    af = np.maximum(A, 1e-6)
    vimage[..., 3] = np.where(D > 0, ge / af, 0.0)
    vimage[..., 4] = np.where(A > 1e-6, -(e / af) * ge, 0.0)
    return out


def flatten(scales, weight=1.0):
    """weight · flatten_loss over raw scales (N, sd) -> (loss, ∇ w.r.t. the raw scales (N, sd), ∇ w.r.t. the ACTIVATED
    scales (N, sd): the constant weight / N on the first minimal axis)."""
    s = np.asarray(scales, np.float64)
    n = s.shape[0]
    if n == 0:
        return 0.0, np.zeros_like(s), np.zeros_like(s)
    arg = np.argmin(s, axis=1)                      # numpy's argmin returns the FIRST minimum: the cumsum tie-break
    onehot = np.zeros_like(s)
    onehot[np.arange(n), arg] = 1.0
    m = s[np.arange(n), arg]
    return weight * float(np.exp(m).sum() / n), weight * onehot * np.exp(s) / n, weight * onehot / n
