"""Host mirror of src/depth_supervision.jl (anchored depth supervision of :rgbd / :rgbdn training, `use_depth_loss`,
training.jl:604-620,709-718).

- The anchors — a per-camera affine alignment of a relative depth prior to the SfM cloud, fitted once at start-up — are
  host work in numpy, in fp32 where the reference is fp32: `DepthAnchor`, `anchor_target`, `ls_affine_fit`,
  `ransac_affine_fit`, `robust_aabb`, `collect_anchor_samples`, `fit_depth_anchors`.  RANSAC draws come from a
  caller-supplied `numpy.random.Generator`: they cannot match Julia's stream, the properties are the reference's.
- The loss — per-pixel work on every step — runs on the gsr_depth_* entry points: `depth_target`, `depth_loss`,
  `depth_loss_backward_`, the autograd form `ssi_depth_loss`, and the loss head `l1_ssim_depth_loss`.

Layouts: the image is the rasterizer's frame (H, W, C) ≙ the reference's (C, W, H), C = 5 (:rgbd) or 8 (:rgbdn): channel 3
blended depth, 4 alpha; a prior is (H, W) ≙ (W, H).  Not built: `load_depth_prior` (image I/O) and the TOML anchor cache
(its fingerprint is Julia's `hash`)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

from . import _args as A
from . import _lib as L

DEPTH_LOSS_WEIGHT = 2.0            # depth_loss_weight (utils.jl)
DEPTH_LOSS_FINAL_SCALE = 0.02      # depth_loss_final_scale
DEPTH_LOSS_GRADIENT_WEIGHT = 1.0   # depth_loss_gradient_weight
f32 = np.float32


# ---- anchors (host) ----

def anchor_target(a, b, floor, disparity, t) -> np.float32:
    """Map a prior value `t` through an anchor into target space (inverse depth): depth_supervision.jl:63-68."""
    a, b, floor, t = f32(a), f32(b), f32(floor), f32(t)
    with np.errstate(all="ignore"):
        affine = f32(a * t) + b
        return f32(min(affine, f32(1) / floor)) if disparity > 0 else f32(1) / (affine + floor)


@dataclass(frozen=True)
class DepthAnchor:
    """`a·t + b` maps the prior value t to inverse depth 1/(z + floor) when `disparity` > 0, to depth z otherwise; `p_far`
    is the smallest target the fit's inlier support covers (0: no support information)."""
    a: float
    b: float
    floor: float
    disparity: float
    p_far: float = 0.0

    @classmethod
    def from_support(cls, a, b, floor, disparity, t_lo, t_hi) -> "DepthAnchor":
        """The reference's six-argument constructor (depth_supervision.jl:87-98): p_far is the farther — the smaller — of
        the two endpoint targets; a bracket without width, or a non-finite or non-positive bound, gives 0."""
        a, b, floor, disparity = (float(f32(v)) for v in (a, b, floor, disparity))
        if not f32(t_hi) > f32(t_lo):
            return cls(a, b, floor, disparity, 0.0)
        p_far = min(anchor_target(a, b, floor, disparity, t_lo), anchor_target(a, b, floor, disparity, t_hi))
        if not (np.isfinite(p_far) and p_far > 0):
            p_far = 0.0
        return cls(a, b, floor, disparity, float(p_far))

    def target(self, t) -> np.float32:
        return anchor_target(self.a, self.b, self.floor, self.disparity, t)

    def struct(self) -> L.DepthAnchorS:
        return L.DepthAnchorS(self.a, self.b, self.floor, self.disparity, self.p_far)


class AnchorFit(NamedTuple):
    a: float
    b: float
    corr: float
    inlier_fraction: float
    t_lo: float
    t_hi: float
    usable: bool


def ls_affine_fit(ts, ys, var_ridge=1.5e-5):
    """Least-squares y ≈ a·t + b with the slope shrunk by `var_ridge` (depth_supervision.jl:120-127) -> (a, b) float32."""
    ts, ys = np.asarray(ts, f32), np.asarray(ys, f32)
    mt, my = ts.mean(dtype=f32), ys.mean(dtype=f32)
    cov = ((ts - mt) * (ys - my)).mean(dtype=f32)
    var = np.square(ts - mt).mean(dtype=f32)
    a = f32(cov / (var + f32(var_ridge)))
    return a, f32(my - a * mt)


def ransac_affine_fit(ts, ys, rng: np.random.Generator = None, ransac_iterations=256, min_anchor_samples=256,
                      anchor_min_inlier_fraction=0.3, anchor_min_corr=0.35, score_subset=16_384,
                      support_quantile=0.02) -> AnchorFit:
    """RANSAC affine regression (depth_supervision.jl:136-200): LS init for the residual scale (3 · 1.4826 · MAD), 2-point
    hypotheses scored by inlier count on a subset, two LS refits on the final set; `t_lo`/`t_hi` are the 2 % / 98 %
    quantiles of the inliers' prior values."""
    ts, ys = np.ascontiguousarray(ts, f32), np.ascontiguousarray(ys, f32)
    rng = np.random.default_rng(0) if rng is None else rng
    n = ts.shape[0]
    if n == 0:
        return AnchorFit(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, False)
    a, b = ls_affine_fit(ts, ys)
    res = np.abs(ys - (a * ts + b))
    eps = max(f32(3) * f32(1.4826) * f32(np.median(res)), f32(1e-8))
    sub = slice(None) if n <= score_subset else np.round(np.linspace(1, n, score_subset)).astype(np.int64) - 1
    ts_s, ys_s = ts[sub], ys[sub]

    def score(a, b):
        return int(np.count_nonzero(np.abs(ys_s - (a * ts_s + b)) <= eps))

    best_a, best_b, best = a, b, score(a, b)
    for _ in range(ransac_iterations):
        i, j = (int(v) for v in rng.integers(0, n, 2))
        dt = ts[i] - ts[j]
        if abs(dt) < f32(1e-8):
            continue
        ai = f32((ys[i] - ys[j]) / dt)
        bi = f32(ys[i] - ai * ts[i])
        s = score(ai, bi)
        if s > best:
            best_a, best_b, best = ai, bi, s
    a, b = best_a, best_b
    inl = np.zeros(0, np.int64)
    for _ in range(2):
        inl = np.flatnonzero(np.abs(ys - (a * ts + b)) <= eps)
        if inl.size < min_anchor_samples:
            break
        a, b = ls_affine_fit(ts[inl], ys[inl])
    frac = f32(inl.size / n)
    corr = f32(0)
    if inl.size >= 2:
        with np.errstate(all="ignore"):
            corr = f32(np.corrcoef(ts[inl].astype(np.float64), ys[inl].astype(np.float64))[0, 1])
        if not np.isfinite(corr):
            corr = f32(0)
    t_lo = t_hi = f32(0)
    if inl.size >= 2:
        t_lo, t_hi = (f32(v) for v in np.quantile(ts[inl], [support_quantile, 1.0 - support_quantile]))
    usable = bool(n >= min_anchor_samples and frac >= f32(anchor_min_inlier_fraction) and abs(corr) >= f32(anchor_min_corr))
    return AnchorFit(float(a), float(b), float(corr), float(frac), float(t_lo), float(t_hi), usable)


def robust_aabb(points, q=0.01, pad=0.1):
    """The [q, 1-q] quantile box of the (N, 3) points, padded by `pad` of its extent (depth_supervision.jl:202-207)."""
    points = np.asarray(points, f32)
    lo = np.quantile(points, q, axis=0).astype(f32)
    hi = np.quantile(points, 1.0 - q, axis=0).astype(f32)
    margin = f32(pad) * (hi - lo)
    return lo - margin, hi + margin


def collect_anchor_samples(points, camera, prior, aabb_min, aabb_max, near_plane=0.2, max_anchor_samples=262_144):
    """Project the (N, 3) points into `camera` and pair the prior's value at each hit pixel with the point's camera-space
    depth (depth_supervision.jl:216-251) -> (ts, zs) float32.  `prior` is (H, W)."""
    points = np.asarray(points, f32)
    prior = np.asarray(prior, f32)
    n = points.shape[0]
    stride = max(1, -(-n // max_anchor_samples))
    x = points[::stride]
    W, H = int(camera.width), int(camera.height)
    if prior.shape != (H, W):
        raise ValueError("prior must be (height, width) of the camera")
    fx, fy = f32(camera.focal[0]), f32(camera.focal[1])
    cx, cy = f32(camera.principal[0]) * f32(W), f32(camera.principal[1]) * f32(H)
    R, t = np.asarray(camera.R, f32).reshape(3, 3), np.asarray(camera.t, f32).reshape(3)
    keep = np.all((x >= aabb_min) & (x <= aabb_max), axis=1)
    p = x @ R.T + t
    z = p[:, 2]
    keep &= z > f32(near_plane)
    with np.errstate(all="ignore"):
        px = np.floor(fx * p[:, 0] / z + cx)
        py = np.floor(fy * p[:, 1] / z + cy)
    keep &= (px >= 0) & (px < W) & (py >= 0) & (py < H)
    idx = np.flatnonzero(keep)
    tp = prior[py[idx].astype(np.int64), px[idx].astype(np.int64)]
    ok = np.isfinite(tp) & (tp > 0)
    return tp[ok].astype(f32), z[idx][ok].astype(f32)


def fit_depth_anchors(points, cameras, priors, mode="ssi", min_anchor_samples=256, depth_floor_fraction=0.05,
                      flat_prior_var=1e-6, rng: np.random.Generator = None):
    """Per-camera anchors against the SfM cloud (depth_supervision.jl:265-337) -> list of DepthAnchor / None.  Every camera
    with a prior gets a disparity fit (1/(z + floor) ≈ a·t + b) and a depth fit (z ≈ a·t + b); `mode` "ssi" resolves the
    dataset-wide model by majority vote over the per-camera correlations, "ssi_disparity" / "ssi_depth" force it; cameras
    whose selected fit is unusable, or whose slope sign is outvoted, get None."""
    if mode not in ("ssi", "ssi_disparity", "ssi_depth"):
        raise ValueError(f"Invalid depth loss mode: {mode}")
    rng = np.random.default_rng(0) if rng is None else rng
    points = np.asarray(points, f32)
    fits = [None] * len(cameras)
    lo, hi = robust_aabb(points)
    for i, (cam, prior) in enumerate(zip(cameras, priors)):
        if prior is None:
            continue
        ts, zs = collect_anchor_samples(points, cam, prior, lo, hi)
        if ts.size < min_anchor_samples or ts.var(ddof=1, dtype=f32) < f32(flat_prior_var):   # a constant prior: no signal
            continue
        floor = max(f32(1e-8), f32(depth_floor_fraction) * f32(np.median(zs)))
        fits[i] = (floor, ransac_affine_fit(ts, f32(1) / (zs + floor), rng, min_anchor_samples=min_anchor_samples),
                   ransac_affine_fit(ts, zs, rng, min_anchor_samples=min_anchor_samples))
    if mode == "ssi":
        votes = total = 0
        for fit in fits:
            if fit is None or not (fit[1].usable or fit[2].usable):
                continue
            total += 1
            votes += (not fit[2].usable) or (fit[1].usable and abs(fit[1].corr) >= abs(fit[2].corr))
        disparity = votes >= total - votes
    else:
        disparity = mode == "ssi_disparity"
    sel = [None if fit is None else (fit[1] if disparity else fit[2]) for fit in fits]
    sign_vote = sum(int(np.sign(f.a)) for f in sel if f is not None and f.usable)
    slope_sign = 1.0 if sign_vote >= 0 else -1.0
    anchors = [None] * len(cameras)
    for i, f in enumerate(sel):
        if f is None or not (f.usable and np.sign(f.a) == slope_sign):
            continue
        anchors[i] = DepthAnchor.from_support(f.a, f.b, fits[i][0], 1.0 if disparity else 0.0, f.t_lo, f.t_hi)
    return anchors


def depth_weight(step, weight=DEPTH_LOSS_WEIGHT, final_scale=DEPTH_LOSS_FINAL_SCALE, steps=30000) -> float:
    """weight · final_scale^clamp(step/steps, 0, 1) in fp32: the exponential decay of the term's weight (training.jl)."""
    frac = f32(min(max(f32(step) / f32(steps), f32(0)), f32(1)))
    return float(f32(weight) * np.power(f32(final_scale), frac, dtype=f32))


# ---- the loss (device) ----

check_frame = A.frame_check((5, 8), "{} must be a contiguous float32 (H, W, 5) or (H, W, 8) HIP tensor (a :rgbd / :rgbdn frame)")


def _check_prior(prior, H=None, W=None, device=None):
    A.check(prior, "prior must be a contiguous float32 (H, W) HIP tensor", shape=(None, None))
    return prior if H is None else A.check(prior, "prior must have the image's height, width and device", shape=(H, W), device=device)


def depth_loss_scratch_bytes(W: int, H: int) -> int:
    return int(L.load().gsr_depth_loss_scratch_bytes(int(W), int(H)))


_SCRATCH = A.FrameScratch(depth_loss_scratch_bytes, align=16)  # what depth_loss leaves for depth_loss_backward_


def depth_target(anchor: DepthAnchor, prior, qstep: float):
    """`depth_target` (depth_supervision.jl:425-438) on the device -> (target (H, W) float32, half_band (H, W) float32,
    flags (H, W) uint8: bit 0 valid, bit 1 far_extrap)."""
    torch = A._torch()
    H, W = _check_prior(prior).shape
    target, half = torch.empty_like(prior), torch.empty_like(prior)
    flags = torch.empty((H, W), dtype=torch.uint8, device=prior.device)
    an = anchor.struct()
    with torch.cuda.device(prior.device):
        L.check(L.load().gsr_depth_target(W, H, prior.data_ptr(), C.byref(an), float(qstep), target.data_ptr(), half.data_ptr(),
                                          flags.data_ptr(), L.stream()))
    return target, half, flags


def depth_loss(image, prior, anchor: DepthAnchor, qstep: float, weight: float, lambda_grad: float = DEPTH_LOSS_GRADIENT_WEIGHT,
               stats: bool = False, scratch=None, maps: bool = False):
    """weight · ssi_depth_loss (depth_supervision.jl:473-536) of a :rgbd / :rgbdn frame against the target built from
    `prior` and `anchor`, as a 0-d tensor.  `stats=True` also returns the device vector (Σα, Σw_supported, μ, σ);
    `maps=True` the (target, half_band, flags) the kernel built.  `scratch` (optional, caller-owned, >=
    depth_loss_scratch_bytes): what `depth_loss_backward_` of the same image reads; by default a buffer kept per device
    and image size."""
    torch = A._torch()
    H, W, Cn = check_frame(image).shape
    _check_prior(prior, H, W, image.device)
    buf = _SCRATCH.get(scratch, W, H, image.device)
    loss = torch.empty((), dtype=torch.float32, device=image.device)
    st = torch.empty(4, dtype=torch.float32, device=image.device)
    tm = hm = fm = None
    if maps:
        tm, hm = torch.empty_like(prior), torch.empty_like(prior)
        fm = torch.empty((H, W), dtype=torch.uint8, device=image.device)
    an = anchor.struct()
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_depth_loss_forward(
            W, H, Cn, image.data_ptr(), prior.data_ptr(), C.byref(an), float(qstep), float(lambda_grad), float(weight),
            loss.data_ptr(), st.data_ptr(), *(None if m is None else m.data_ptr() for m in (tm, hm, fm)), buf.data_ptr(),
            buf.numel() * buf.element_size(), L.stream()))
    out = (loss,) + ((st,) if stats else ()) + (((tm, hm, fm),) if maps else ())
    return out[0] if len(out) == 1 else out


def depth_loss_backward_(image, prior, anchor: DepthAnchor, qstep: float, vpixels, weight: float,
                         lambda_grad: float = DEPTH_LOSS_GRADIENT_WEIGHT, scratch=None):
    """ADDS weight · ∂ssi_depth_loss/∂(D, α) onto channels 3 and 4 of `vpixels` (H, W, C), in place; no other channel is
    touched.  Needs `depth_loss` of the same image, prior, anchor and qstep (and the same `scratch`) run before it.
    Run-to-run bit-identical.  A `vpixels` this was added onto must go to `backward_raw` with `color_cotangent=False`."""
    torch = A._torch()
    H, W, Cn = check_frame(image).shape
    A.check_vpixels(check_frame, vpixels, image)
    _check_prior(prior, H, W, image.device)
    buf = _SCRATCH.get(scratch, W, H, image.device, create=False)
    if buf is None:
        raise ValueError("run depth_loss of this image first: the backward reads what it left on the device")
    an = anchor.struct()
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_depth_loss_backward(
            W, H, Cn, image.data_ptr(), prior.data_ptr(), C.byref(an), float(qstep), float(lambda_grad), float(weight),
            vpixels.data_ptr(), buf.data_ptr(), buf.numel() * buf.element_size(), L.stream()))
    return vpixels


def ssi_depth_loss(image, prior, anchor: DepthAnchor, qstep: float, weight: float = 1.0,
                   lambda_grad: float = DEPTH_LOSS_GRADIENT_WEIGHT):
    """weight · ssi_depth_loss, differentiable w.r.t. the (H, W, C) frame (channels 3 and 4; the others get zeros)."""
    return A.cotangent_term(
        image, lambda im, scratch: depth_loss(im, prior, anchor, qstep, weight, lambda_grad, scratch=scratch),
        lambda im, v, scratch: depth_loss_backward_(im, prior, anchor, qstep, v, weight, lambda_grad, scratch=scratch),
        depth_loss_scratch_bytes)


def l1_ssim_depth_loss(rast, image, target, prior, anchor: Optional[DepthAnchor], qstep: float, step: int,
                       lambda_dssim: float = 0.2, weight: float = DEPTH_LOSS_WEIGHT, final_scale: float = DEPTH_LOSS_FINAL_SCALE,
                       steps: int = 30000, lambda_grad: float = DEPTH_LOSS_GRADIENT_WEIGHT, camera=None,
                       normal_weight: float = None, bgrid=None, view: int = None, terms: dict = None):
    """The loss of `step!` with `use_depth_loss` (training.jl:604-620,709-718), one term only: `training_loss` with the
    depth term at depth_weight(step) and, for a :rgbdn frame given `camera` and `normal_weight`, the depth-normal term (its
    value goes into `terms["normal"]` when a dict is passed).  Returns (photometric, depth_term, vpixels); `anchor=None` (a
    camera that lost the vote) means no depth term: depth_term is None.  Whether `vpixels` may still go to `backward_raw`
    with `color_cotangent=True` is `StepLoss.color_cotangent` of the same call of `training_loss`."""
    from . import training_loss as T
    check_frame(image)
    w = depth_weight(step, weight, final_scale, steps)
    out = T.training_loss(rast, image, target, lambda_dssim=lambda_dssim, bgrid=bgrid, view=view,
                          depth=None if anchor is None else T.DepthTerm(prior, anchor, qstep, w, lambda_grad),
                          normal=None if normal_weight is None else T.NormalTerm(camera, normal_weight))
    if terms is not None and out.normal_term is not None:
        terms["normal"] = out.normal_term
    return out.photometric, out.depth_term, out.vpixels
