"""Host mirror of src/sky_dome.jl: a frozen shell of Gaussians at a large radius, rendered in its own :rgb pass and
composited BEHIND the scene (`use_sky_dome`; `step!`, training.jl:593-598,634-639,673-676,721-725; `validate`, :512-516).

- The lattice and the dome object are host work, fp32 numpy where the reference is fp32: `fibonacci_sphere`,
  `sky_dome_directions`, `sky_dome_radius`, `SkyDome`, `merge_sky`.  Only the dome's colours (`features_dc`) train.
- What the step adds per pixel runs on the gsr_sky_* entry points (csrc/sky.hip): `composite_sky`, `composite_sky_`,
  `sky_composite_backward_`, `sky_opacity_loss`, and the loss head `l1_ssim_sky_loss`.  The dome is rendered by its own
  `GaussianRasterizer(mode="rgb", far_plane=4·radius)`: `render_sky`, `sky_backward`.

Layouts: the scene frame is the rasterizer's (H, W, C) ≙ the reference's (C, W, H), C = 5 (:rgbd) or 8 (:rgbdn), channel 4
alpha; the sky frame is (H, W, 3); a mask is (H, W) ≙ (W, H) in [0, 1].  The scene pass of a step with a dome is rendered
over a ZERO background (training.jl:596): the dome is the background.  Not built: `load_sky_mask` (image I/O and resize),
`sky_init_color` and `estimate_up_vec` (dataset side)."""
from __future__ import annotations

import math

import numpy as np

from . import _args as A
from . import _lib as L

f32 = np.float32
SKY_DOME_SHAPES = ("hemisphere", "sphere")   # sky_dome.jl:74
SKY_DOME_OVERLAP = f32(1.0)                  # Gaussian std as a multiple of the lattice spacing (sky_dome.jl:99-108)
SKY_DOME_POINTS = 32_768                     # sky_dome_points (utils.jl)
SKY_DOME_LR = 25e-4                          # sky_dome_lr
SKY_DOME_RADIUS_FACTOR = 100.0               # sky_dome_radius_factor: camera extents
SKY_LOSS_FROM_ITER = 500                     # sky_loss_from_iter
SH0 = f32(0.28209479177387814)


# ---- the lattice (host) ----

def fibonacci_sphere(n: int):
    """`n` roughly equal-area unit vectors (Fibonacci lattice) as an (n, 3) float32 array ≙ the reference's (3, n), and the
    mean angular spacing sqrt(4π / n) that sizes the Gaussians (sky_dome.jl:57-71).  z, r and θ in fp32; the golden angle
    and the spacing are rounded once from double."""
    i = np.arange(1, n + 1, dtype=f32)
    golden_angle = f32(math.pi * (3.0 - math.sqrt(5.0)))
    z = f32(1) - f32(2) * (i - f32(0.5)) / f32(n)
    r = np.sqrt(np.maximum(f32(1) - z * z, f32(0)))
    theta = golden_angle * (i - f32(1))
    return np.stack([r * np.cos(theta), r * np.sin(theta), z], 1).astype(f32), f32(math.sqrt(4 * math.pi / n))


def sky_dome_directions(n: int, shape: str, up=(0.0, 0.0, 1.0)):
    """`n` directions of the dome and the lattice's spacing (sky_dome.jl:87-97).  "sphere" is the whole sky; "hemisphere"
    keeps what is at or above the horizon against the normalised `up`, of a lattice of 2n points: `n` means "Gaussians in
    the dome" either way, and the spacing — a property of the lattice, not of the surviving subset — still sizes them."""
    if shape not in SKY_DOME_SHAPES:
        raise ValueError(f"Invalid sky dome shape: `{shape}` not in {SKY_DOME_SHAPES}.")
    if shape == "sphere":
        return fibonacci_sphere(n)
    dirs, spacing = fibonacci_sphere(2 * n)
    up = np.asarray(up, f32)
    up = up / np.sqrt((up * up).sum(dtype=f32))
    kept = (dirs[:, 0] * up[0] + dirs[:, 1] * up[1]) + dirs[:, 2] * up[2] >= f32(0)
    return np.ascontiguousarray(dirs[kept]), spacing


def sky_dome_radius(far_plane: float, factor: float = SKY_DOME_RADIUS_FACTOR, extent: float = 1.0) -> float:
    """`factor` camera extents, clamped so that the whole shell stays inside the SCENE rasterizer's far plane too
    (sky_dome.jl:155-159): min(factor · extent, 0.8 · far_plane - extent), in fp32."""
    return float(min(f32(factor) * f32(extent), f32(0.8) * f32(far_plane) - f32(extent)))


def rgb_2_sh(c):
    """gaussians.jl:133"""
    return ((np.asarray(c, f32) - f32(0.5)) * (f32(1) / SH0)).astype(f32)


def inverse_sigmoid(x) -> np.float32:
    """gaussians.jl:137"""
    x = f32(x)
    return f32(np.log(x / (f32(1) - x)))


def sky_hard(mask):
    """The mask thresholded, for uses that cannot act on a fraction of a pixel (sky_dome.jl:297)."""
    return mask > 0.5


# ---- the dome ----

class SkyDome:
    """SkyDome(kab, camera, opt_params; center, radius, up, color) — sky_dome.jl:43-48,120-146.  `gaussians` (a
    ply.GaussianModel of device tensors, max_sh_degree 0): frozen points `center + radius · dirs`, log-scales
    log(radius · spacing · SKY_DOME_OVERLAP), identity rotations, opacity logits inverse_sigmoid(0.99); `features_dc`
    (n, 1, 3) = rgb_2_sh(color) is the only trainable array, with `optimizer` = optim.Adam(features_dc, lr, eps=1e-15).
    `rast`: the dome's own :rgb rasterizer at the camera's resolution with far_plane = 4 · radius (the default 1000 would cull
    the whole shell of any sizeable scene).  Handles are independent: the scene's forward / backward pair is not disturbed."""

    def __init__(self, camera, n: int = SKY_DOME_POINTS, shape: str = "hemisphere", center=(0.0, 0.0, 0.0), radius: float = 100.0,
                 up=(0.0, 0.0, 1.0), color=(0.5, 0.5, 0.5), lr: float = SKY_DOME_LR, device="cuda"):
        torch = A._torch()
        from . import optim, ply
        from .rasterizer import GaussianRasterizer
        if n <= 0:
            raise ValueError(f"`sky_dome_points={n}` must be positive.")
        dirs, spacing = sky_dome_directions(int(n), shape, up)
        n = dirs.shape[0]   # the cut lands near, but not exactly on, n
        radius = f32(radius)
        points = dirs * radius + np.asarray(center, f32)
        scales = np.full((n, 3), np.log(radius * spacing * SKY_DOME_OVERLAP), f32)
        rotations = np.zeros((n, 4), f32)
        rotations[:, 0] = 1
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(device)  # noqa: E731
        self.gaussians = ply.GaussianModel(
            to(points), to(np.tile(rgb_2_sh(color).reshape(1, 1, 3), (n, 1, 1))), to(np.zeros((n, 0, 3), f32)), to(scales),
            to(rotations), to(np.full((n, 1), inverse_sigmoid(0.99), f32)), 0, 0)
        self.radius = float(radius)
        self.device = self.gaussians.points.device
        self.optimizer = optim.Adam(self.gaussians.features_dc, lr=lr, eps=1e-15)
        self.rast = GaussianRasterizer(camera.width, camera.height, mode="rgb", far_plane=4.0 * self.radius, device=device)
        self._refresh_activations()

    def _refresh_activations(self):
        """σ(opacities) and exp(scales) of the frozen arrays (the functor prologue, rasterizer.jl:218-247): computed at
        construction and after a checkpoint restored the arrays, never per step."""
        from .rasterizer import prologue_forward
        g = self.gaussians
        _, self._opacities_act, self._scales_act = prologue_forward(g.features_dc, None, g.opacities, g.scales)

    def __len__(self):
        return int(self.gaussians.points.shape[0])

    def view_rasterizer(self, camera):
        """`sky_view_rasterizer` (sky_dome.jl:206-207): an :rgb rasterizer at `camera`'s resolution with the dome's far
        plane, for render paths outside training."""
        from .rasterizer import GaussianRasterizer
        return GaussianRasterizer(camera.width, camera.height, mode="rgb", far_plane=4.0 * self.radius, device=self.device)

    def memory_usage(self) -> int:
        """sky_dome.jl:161-164: the model, the optimizer's moments and the rasterizer."""
        g = self.gaussians
        arrays = (g.points, g.features_dc, g.features_rest, g.scales, g.rotations, g.opacities, self.optimizer.mu, self.optimizer.nu)
        return sum(t.numel() * t.element_size() for t in arrays) + self.rast.memory_usage()

    def close(self):
        """KA.unsafe_free!(sky) — sky_dome.jl:166-171"""
        self.rast.close()


def render_sky(sky: SkyDome, camera, features_dc=None, rast=None, forward_only: bool = False):
    """`render_sky` (sky_dome.jl:186-198): the dome's rgb for `camera` at sh_degree 0 -> (H, W, 3), the rasterizer's own
    image (overwritten by its next render).  `features_dc` defaults to the dome's colours; every other array is the frozen
    constant.  `rast` defaults to the dome's rasterizer; views at another resolution pass `sky.view_rasterizer(camera)`.
    forward_only=True keeps no backward state (`validate`, GUI)."""
    g = sky.gaussians
    rast = sky.rast if rast is None else rast
    dc = g.features_dc if features_dc is None else features_dc
    return rast.forward_raw(g.points, dc, sky._opacities_act, sky._scales_act, g.rotations, camera, 0, (0.0, 0.0, 0.0),
                            forward_only=forward_only)


def sky_backward(sky: SkyDome, camera, vsky, features_dc=None, rast=None):
    """∇features_dc (n, 1, 3) of the dome's last `render_sky` for the cotangent `vsky` (H, W, 3).  The handle's ordinary
    backward; the gradients of the frozen arrays are dropped."""
    g = sky.gaussians
    rast = sky.rast if rast is None else rast
    dc = g.features_dc if features_dc is None else features_dc
    return rast.backward_raw(vsky, g.points, dc, sky._opacities_act, sky._scales_act, g.rotations, camera, 0, (0.0, 0.0, 0.0))[1]


# ---- composite and sky-mask loss (device) ----

check_frame = A.frame_check((5, 8), "{} must be a contiguous float32 (H, W, 5) or (H, W, 8) HIP tensor (a :rgbd / :rgbdn frame: "
                            ":rgb has no alpha row)")


def sky_scratch_bytes(W: int, H: int) -> int:
    return int(L.load().gsr_sky_scratch_bytes(int(W), int(H)))


_SCRATCH = A.FrameScratch(sky_scratch_bytes, align=8)  # what composite_sky with a mask leaves for its backward


def composite_sky(image, sky_rgb, out=None, sky_weight=None, sky_loss_weight: float = 1.0, scratch=None):
    """`composite_sky` (sky_dome.jl:246-250): image + (1 - α) · sky over the rgb channels of the frame -> `out` (H, W, C), a
    whole frame (channels >= 3 copied); `out=image` composites in place.  With `sky_weight` (H, W) the same pass evaluates
    the sky-mask loss: returns (out, sky_loss_weight · sky_opacity_loss) and leaves in `scratch` (default: a buffer kept
    per device and image size) what `sky_composite_backward_` reads."""
    torch = A._torch()
    H, W, Cn = check_frame(image).shape
    A.check_like(sky_rgb, "sky_rgb", (H, W, 3), image.device)
    out = torch.empty_like(image) if out is None else A.check_like(out, "out", image.shape, image.device)
    loss = buf = None
    if sky_weight is not None:
        A.check_like(sky_weight, "sky_weight", (H, W), image.device)
        buf = _SCRATCH.get(scratch, W, H, image.device)
        loss = torch.empty((), dtype=torch.float32, device=image.device)
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_sky_composite_forward(W, H, Cn, image.data_ptr(), sky_rgb.data_ptr(), L.ptr(sky_weight),
                                                   float(sky_loss_weight), out.data_ptr(), L.ptr(loss), L.ptr(buf), L.stream()))
    return out if sky_weight is None else (out, loss)


def composite_sky_(rast_image, sky: SkyDome, camera, sky_rast=None):
    """`composite_sky!` (sky_dome.jl:217-228), the non-AD form for `validate` and display: renders the dome forward-only
    and adds it into the rgb channels of `rast_image` in place; depth and alpha are untouched.  An :rgb frame has no alpha
    row and is returned as it is."""
    if rast_image.dim() == 3 and rast_image.shape[2] == 3:
        return rast_image
    return composite_sky(rast_image, render_sky(sky, camera, rast=sky_rast, forward_only=True), out=rast_image)


def sky_composite_backward_(image, sky_rgb, vpixels, sky_weight=None, sky_loss_weight: float = 1.0, vsky=None, scratch=None):
    """The pullback of `composite_sky` (and of the sky-mask loss when `sky_weight` is given).  `vpixels` (H, W, C) holds the
    cotangent g of the composite in its rgb channels (the loss head's output).  Returns vsky (H, W, 3) = (1 - α) · g, and
    ADDS -(g · sky) + sky_loss_weight · 2·w·α / max(Σw, 1) onto channel 4 of `vpixels`, in place, as one fp32 add; no other
    channel is written.  With a mask it needs `composite_sky` of the same image and mask (and the same `scratch`) run
    before it.  A `vpixels` this was added onto must go to `backward_raw` with `color_cotangent=False`."""
    torch = A._torch()
    H, W, Cn = check_frame(image).shape
    A.check_like(sky_rgb, "sky_rgb", (H, W, 3), image.device)
    A.check_like(vpixels, "vpixels", image.shape, image.device)
    if vpixels.data_ptr() == image.data_ptr():
        raise ValueError("vpixels must not be the image")
    vsky = torch.empty_like(sky_rgb) if vsky is None else A.check_like(vsky, "vsky", (H, W, 3), image.device)
    buf = None
    if sky_weight is not None:
        A.check_like(sky_weight, "sky_weight", (H, W), image.device)
        buf = _SCRATCH.get(scratch, W, H, image.device, create=False)
        if buf is None:
            raise ValueError("run composite_sky of this image and mask first: the backward reads what it left on the device")
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_sky_composite_backward(W, H, Cn, image.data_ptr(), sky_rgb.data_ptr(), L.ptr(sky_weight),
                                                    float(sky_loss_weight), vpixels.data_ptr(), vsky.data_ptr(), L.ptr(buf),
                                                    L.stream()))
    return vsky


def sky_opacity_loss(image, sky_weight, weight: float = 1.0):
    """weight · `sky_opacity_loss` (sky_dome.jl:315-320) = weight · Σ w·α² / max(Σw, 1) of the frame's alpha channel — the raw
    channel, so that a saturated pixel keeps its gradient 2w / Σw —, differentiable w.r.t. the (H, W, C) frame (channel 4;
    the others get zeros).  The stand-alone form: it runs the fused passes against a zero sky frame; a training step uses
    `l1_ssim_sky_loss`, where the loss rides on the composite's passes."""
    zero_sky = A._torch().zeros(tuple(image.shape[:2]) + (3,), dtype=A._torch().float32, device=image.device)
    return A.cotangent_term(image, lambda im, scratch: composite_sky(im, zero_sky, None, sky_weight, weight, scratch=scratch)[1],
                            lambda im, v, scratch: sky_composite_backward_(im, zero_sky, v, sky_weight, weight, scratch=scratch),
                            sky_scratch_bytes)


def l1_ssim_sky_loss(rast, image, target, sky: SkyDome, camera, sky_weight=None, sky_loss_weight: float = 1.0, step: int = None,
                     sky_loss_from_iter: int = SKY_LOSS_FROM_ITER, lambda_dssim: float = 0.2, bgrid=None, view: int = None,
                     depth: dict = None, normal: float = None, terms: dict = None):
    """The loss of `step!` with `use_sky_dome` (training.jl:634-639,673-676,721-725): `training_loss` with the dome behind
    `image` and the schedules resolved here.  `sky_weight` (H, W) is ignored while `step` < `sky_loss_from_iter` (`step=None`
    means "active"): sky_term is then None.  `depth` = dict(prior=, anchor=, qstep=, step=[, weight=, final_scale=, steps=,
    lambda_grad=]) adds the anchored depth term at depth_weight(step) (`terms["depth"]`; ignored when its anchor is None), and
    for a :rgbdn frame `normal` (a weight) the depth-normal term (`terms["normal"]`).  Returns (photometric, sky_term or None,
    vpixels, vsky).

    `image` must be the scene rendered over a ZERO background (training.jl:596); `vpixels` carries an alpha cotangent
    (`StepLoss.color_cotangent` is false); `vsky` goes to `sky_backward(sky, camera, vsky)`."""
    from . import depth_supervision as DS, training_loss as T
    check_frame(image)
    active = sky_weight is not None and (step is None or step >= sky_loss_from_iter)
    if depth is not None and depth.get("anchor") is not None:
        w = DS.depth_weight(depth["step"], depth.get("weight", DS.DEPTH_LOSS_WEIGHT),
                            depth.get("final_scale", DS.DEPTH_LOSS_FINAL_SCALE), depth.get("steps", 30000))
        depth = T.DepthTerm(depth["prior"], depth["anchor"], depth["qstep"], w, depth.get("lambda_grad", DS.DEPTH_LOSS_GRADIENT_WEIGHT))
    else:
        depth = None
    out = T.training_loss(rast, image, target, lambda_dssim=lambda_dssim, bgrid=bgrid, view=view, depth=depth,
                          sky=T.SkyTerm(sky, camera, sky_weight if active else None, sky_loss_weight),
                          normal=None if normal is None else T.NormalTerm(camera, normal))
    if terms is not None:
        terms.update({k: v for k, v in (("depth", out.depth_term), ("normal", out.normal_term)) if v is not None})
    return out.photometric, out.sky_term, out.vpixels, out.vsky


# ---- export ----

def merge_sky(gs, sky):
    """`merge_sky` (sky_dome.jl:259-278): one Gaussian set for export, the dome LAST (it sorts behind the scene by
    construction).  The dome's SH is degree 0: its higher bands are zero-padded up to the scene's band count, a constant
    colour under any viewer's SH evaluation; for an isotropic scene ((N, 1) scales) the dome's scales are averaged to one
    column.  `gs`: the scene's model (host or device arrays); `sky`: a SkyDome or its model.  Returns a host
    ply.GaussianModel, for `ply.export_ply`."""
    from .checkpoint import _host
    from .ply import GaussianModel
    sg = getattr(sky, "gaussians", sky)
    a = {k: np.asarray(_host(getattr(gs, k)), f32) for k in ("points", "features_dc", "features_rest", "scales", "rotations", "opacities")}
    b = {k: np.asarray(_host(getattr(sg, k)), f32) for k in ("points", "features_dc", "scales", "rotations", "opacities")}
    n, ns = a["points"].shape[0], b["points"].shape[0]
    k_rest = a["features_rest"].shape[1] if a["features_rest"].ndim == 3 else 0
    scales = b["scales"].mean(axis=1, keepdims=True, dtype=f32) if a["scales"].shape[1] == 1 else b["scales"]
    max_deg = getattr(gs, "max_sh_degree", None)
    if max_deg is None:
        max_deg = int(round(math.sqrt(k_rest + 1))) - 1
    return GaussianModel(
        np.concatenate([a["points"], b["points"]]), np.concatenate([a["features_dc"], b["features_dc"]]),
        np.concatenate([a["features_rest"].reshape(n, k_rest, 3), np.zeros((ns, k_rest, 3), f32)]),
        np.concatenate([a["scales"], scales]), np.concatenate([a["rotations"], b["rotations"]]),
        np.concatenate([a["opacities"], b["opacities"]]), int(getattr(gs, "sh_degree", max_deg)), int(max_deg))
