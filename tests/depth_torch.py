"""The reference formulation of anchored depth supervision (src/depth_supervision.jl:406-536) restated: `depth_target` in
numpy float32 (the masks and maps, to compare bit for bit), `ssi_depth_loss` in torch in a chosen dtype (autograd gives its
gradients), and the frame family of the depth supervision tests.  In float64 the torch form is the truth; in float32, on the
CPU, it is the YARDSTICK of the GPU tests: what another valid evaluation of the same fp32 formulation is off from float64
by.

One intended deviation from the reference is restated here too: a pixel with w = 0 is selected out, not multiplied by
zero, so a NaN / Inf depth or prior there costs nothing; a non-finite alpha counts as 0."""
import numpy as np
import torch

f32 = np.float32
MIN_ALPHA = 1e-3


class Anchor:
    """(a, b, floor, disparity, p_far) in float32, as DepthAnchor (depth_supervision.jl:51-57)."""

    def __init__(self, a, b, floor, disparity, p_far):
        self.a, self.b, self.floor, self.disparity, self.p_far = (f32(v) for v in (a, b, floor, disparity, p_far))


def depth_target(anchor, prior, qstep):
    """depth_supervision.jl:425-438 in numpy float32 -> target, half_band, valid, far_extrap."""
    a = anchor
    t = np.asarray(prior, f32)
    with np.errstate(all="ignore"):
        affine = a.a * t + a.b
        valid = np.isfinite(t) & (t > 0) & (affine > 0)
        half_step = f32(0.5) * f32(qstep) * np.abs(a.a)
        if a.disparity > 0:
            target = np.minimum(affine, f32(1) / a.floor)
            half_band = np.full_like(t, half_step)
        else:
            target = f32(1) / (affine + a.floor)
            half_band = half_step * (target * target)
        far = target < a.p_far
    return target.astype(f32), half_band.astype(f32), valid, far


def flags_of(valid, far):
    return (valid.astype(np.uint8) | (far.astype(np.uint8) << 1)).astype(np.uint8)


def _gm(x):
    return 0.5 * x * x / (1.0 + x * x)


def _deadband(r, half):
    return torch.sign(r) * torch.clamp(r.abs() - half, min=0.0)


def ssi_depth_loss(D, A, target, half_band, valid, far, floor, lambda_grad=1.0, frozen=None, info=True):
    """depth_supervision.jl:473-536 on torch tensors D, A (H, W) of one dtype, on any device; target / half_band float32,
    valid / far bool, as numpy arrays or as tensors on D's device.  The detached quantities (the weights, Σα, σ) are computed
    from `frozen` = (D, A) when given (a finite-difference check must hold them fixed), else from the detached inputs.
    -> (loss, dict of Σα, Σw_s, μ, σ, w, ... as numpy; None with info=False: nothing is read back)."""
    dt, dv = D.dtype, D.device
    c = lambda v: torch.tensor(float(v), dtype=dt, device=dv)  # noqa: E731
    t = lambda v: v if isinstance(v, torch.Tensor) else torch.tensor(np.asarray(v), device=dv)  # noqa: E731
    Dc, Ac = (D.detach(), A.detach()) if frozen is None else frozen
    valid_t, far_t, zero, one = t(valid), t(far), c(0.0), c(1.0)
    with torch.no_grad():
        a_cl = torch.where(torch.isfinite(Ac), torch.clamp(Ac, 0.0, 1.0), zero)
        w = torch.where(valid_t & (a_cl > c(f32(MIN_ALPHA))), a_cl, zero)
        live = w > 0
        sum_a = a_cl.sum()
        sum_a1 = torch.clamp(sum_a, min=1.0)
        w_s = torch.where(far_t, zero, w)
        one_sided = (far_t & live).to(dt)
    # selected out, not multiplied by zero: a pixel with w = 0 never enters the arithmetic
    Ds, As = torch.where(live, D, one), torch.where(live, A, one)
    tgt = torch.where(live, t(target).to(dt), zero)
    band = torch.where(live, t(half_band).to(dt), zero)
    fl = c(f32(floor))
    p = 1.0 / (Ds / torch.maximum(As, c(f32(1e-6))) + fl)
    with torch.no_grad():
        pc = p.detach() if frozen is None else 1.0 / (torch.where(live, Dc, one) / torch.maximum(torch.where(live, Ac, one), c(f32(1e-6))) + fl)
        sum_w = torch.clamp(w_s.sum(), min=1e-6)
        mu = (w_s * pc).sum() / sum_w
        sigma = torch.clamp(torch.sqrt(torch.clamp((w_s * (pc - mu) ** 2).sum() / sum_w, min=0.0)), min=1e-6)
        iscale = 1.0 / (2.0 * sigma)
    r = _deadband(p - tgt, band)
    r = r - one_sided * torch.clamp(r, max=0.0)
    data = (w * _gm(r * iscale)).sum()
    hx = (p[:, 1:] - p[:, :-1]) - (tgt[:, 1:] - tgt[:, :-1])
    wx = torch.minimum(w_s[:, 1:], w_s[:, :-1])
    gx = (wx * _gm(_deadband(hx, band[:, 1:] + band[:, :-1]) * iscale)).sum()
    hy = (p[1:, :] - p[:-1, :]) - (tgt[1:, :] - tgt[:-1, :])
    wy = torch.minimum(w_s[1:, :], w_s[:-1, :])
    gy = (wy * _gm(_deadband(hy, band[1:, :] + band[:-1, :]) * iscale)).sum()
    loss = (data + lambda_grad * (gx + gy)) / sum_a1
    if not info:
        return loss, None
    n = lambda v: v.detach().cpu().numpy()  # noqa: E731
    return loss, dict(sum_alpha=float(sum_a), sum_ws=float(w_s.sum()), mu=float(mu), sigma=float(sigma), w=n(w), p=n(p),
                      target=n(tgt), band=n(band), far=n(far_t & live))


def evaluate(frame, prior, anchor, qstep, weight=1.0, lambda_grad=1.0, dtype=torch.float64):
    """frame (H, W, C) numpy -> dict(loss, vimage (H, W, C) float64 = weight · ∂loss/∂frame, stats..., maps...)."""
    target, half_band, valid, far = depth_target(anchor, prior, qstep)
    x = torch.tensor(np.asarray(frame), dtype=dtype, requires_grad=True)
    loss, info = ssi_depth_loss(x[..., 3], x[..., 4], target, half_band, valid, far, anchor.floor, lambda_grad)
    (weight * loss).backward()
    g = x.grad.double().numpy()
    info.update(loss=weight * float(loss.detach()), vimage=g, target_map=target, half_band_map=half_band, valid=valid,
                far_extrap=far)
    return info


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- the frame family ----

FLOOR = 0.25
DISPARITY = Anchor(0.4, 0.01, FLOOR, 1.0, 0.4 * 0.3 + 0.01)            # support t in [0.3, 0.9]: p_far = target(0.3)
DEPTH = Anchor(-10.0, 10.5, FLOOR, 0.0, 1.0 / (-10.0 * 0.3 + 10.5 + FLOOR))  # negative slope: the far end is t = 0.3 too
ANCHORS = {"disparity": DISPARITY, "depth": DEPTH}
QSTEP = 1.0 / 255.0
PLANE_N = np.array([0.2, -0.3, -1.0]) / np.linalg.norm([0.2, -0.3, -1.0])


def make_frame(W, H, C, model, seed):
    """-> (frame (H, W, C) float32, prior (H, W) float32).  A slanted plane (e in about [4.4, 6.6]) with 1 % multiplicative
    depth noise; α uniform in [0.05, 1] with 30 % exactly 1, 8 % below 1e-3 and 2 % exactly 0; the prior is the anchor's
    inverse of the noise-free plane plus noise (so residuals fall on both sides of the deadband); a sky block (the top-right
    quarter, 1/4 x 3/5 of the frame) at t ≈ 0.005 whose left half is rendered nearer (e = 3) and whose right half farther
    (e = 500) than its target; 20 % of the priors <= 0 and 1 % NaN.  A frame of fewer than 64 pixels keeps only the plane,
    the noise and alpha in [0.3, 1] (every pixel live): too few pixels to populate the branches by shares."""
    an = ANCHORS[model]
    r = np.random.default_rng(seed)
    f = 100.0
    rx = (np.arange(W) + 0.5 - 0.5 * W) / f * (97.0 / max(W, 97))
    ry = (np.arange(H) + 0.5 - 0.5 * H) / f * (61.0 / max(H, 61))
    e0 = 5.0 * 1.0630 / (1.0 - 0.2 * rx[None, :] + 0.3 * ry[:, None])
    e = e0 * (1.0 + 1e-2 * r.standard_normal((H, W)))
    a, b, fl = float(an.a), float(an.b), float(an.floor)
    y = 1.0 / (e0 + fl) if an.disparity > 0 else e0
    t = (y - b) / a + 2e-3 * r.standard_normal((H, W))
    tiny = W * H < 64
    alpha = r.uniform(0.3 if tiny else 0.05, 1.0, (H, W))
    u = r.random((H, W)) + (1.0 if tiny else 0.0)
    alpha[u < 0.30] = 1.0
    alpha[(u >= 0.30) & (u < 0.38)] = r.uniform(0.0, 9e-4, (H, W))[(u >= 0.30) & (u < 0.38)]
    alpha[(u >= 0.38) & (u < 0.40)] = 0.0
    sx0, sx1, sy1 = W - max(W // 4, 1), W, max(3 * H // 5, 1)
    if not tiny:
        xm = (sx0 + sx1) // 2
        t[:sy1, sx0:sx1] = 0.005 + 1e-4 * r.random((sy1, sx1 - sx0))
        e[:sy1, sx0:xm] = 3.0
        e[:sy1, xm:sx1] = 500.0
    v = r.random((H, W)) + (1.0 if tiny else 0.0)
    t[v < 0.20] = -np.abs(t[v < 0.20])
    t[(v >= 0.20) & (v < 0.205)] = 0.0
    t[(v >= 0.205) & (v < 0.215)] = np.nan
    frame = np.zeros((H, W, C), f32)
    frame[..., :3] = r.uniform(0.0, 1.0, (H, W, 3))
    frame[..., 3] = e * alpha
    frame[..., 4] = alpha
    if C == 8:
        frame[..., 5:8] = alpha[..., None] * PLANE_N
    return frame, t.astype(f32)


def reference_2x2():
    """The frame of the reference's one-sided sky test (test/runtests.jl:419-452), as (H, W) arrays: anchor, prior, and the
    on-target expected depth."""
    an = Anchor(1.0, 0.05, 0.1, 1.0, anchor_p_far(1.0, 0.05, 0.1, 1.0, 0.3, 0.9))
    prior = np.array([[0.5, 0.8], [0.7, 0.005]], f32)
    target = depth_target(an, prior, QSTEP)[0]
    return an, prior, (f32(1) / target - an.floor).astype(f32)


def anchor_p_far(a, b, floor, disparity, t_lo, t_hi):
    an = Anchor(a, b, floor, disparity, 0.0)
    if not f32(t_hi) > f32(t_lo):
        return f32(0)
    lo, hi = (depth_target(an, np.array([t], f32), 0.0)[0][0] for t in (t_lo, t_hi))
    p = min(lo, hi)
    return p if np.isfinite(p) and p > 0 else f32(0)
