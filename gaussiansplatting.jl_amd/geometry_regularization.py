"""Host mirror of src/geometry_regularization.jl (the geometry regularisation of :rgbdn training, `use_normal_loss`,
training.jl:625-733) on top of the gsr_normal_loss_* / gsr_flatten_loss entry points.

- `depth_normal_loss`: normals implied by the rendered depth map must agree with the blended Gaussian normals;
- `flatten_loss`: an L1 prior on each Gaussian's thinnest axis, which makes the min-axis normal well defined.

Layouts: the image is the rasterizer's :rgbdn frame (H, W, 8) ≙ the reference's (8, W, H): channels 0..2 rgb, 3 blended
depth, 4 alpha, 5..7 the blended normal; scales are (N, 3) or (N, 1) ≙ (3, N) / (1, N), raw (pre-exp).

The fused `optim.fused_backward_tail_step` never materialises ∇scales, so it cannot take the flatten gradient: a step with
the regulariser on runs `rast.backward_raw` + `flatten_loss(..., vscales=...)` + `optim.trainer_tail_step`."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import fused_ssim
from .camera import Camera

NORMAL_CONSISTENCY_WEIGHT = 0.05   # normal_consistency_weight (utils.jl)
NORMAL_FLATTEN_WEIGHT = 0.005      # this package's default of normal_flatten_weight


def _check_frame(image: torch.Tensor, name: str = "image"):
    if not (image.is_cuda and image.dtype == torch.float32 and image.is_contiguous() and image.dim() == 3
            and image.shape[2] == 8):
        raise ValueError(f"{name} must be a contiguous float32 (H, W, 8) HIP tensor (a :rgbdn frame)")
    return image


def _camera_struct(camera: Camera, W: int, H: int) -> L.CameraS:
    """The fields the kernels read: focal and principal (the rays of `pixel_rays`)."""
    if (int(camera.width), int(camera.height)) != (W, H):
        raise ValueError("camera resolution does not match the image")
    cs = L.CameraS()
    for k in range(2):
        cs.focal[k] = float(camera.focal[k])
        cs.principal[k] = float(camera.principal[k])
    if not (cs.focal[0] > 0 and cs.focal[1] > 0):
        raise ValueError("focal lengths must be positive")
    return cs


def _scratch(cache: dict, key, nbytes: int, device) -> torch.Tensor:
    buf = cache.get(key)
    if buf is None or buf.numel() < nbytes or buf.device != device:
        buf = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=device)
        cache[key] = buf
    return buf


_SCRATCH: dict = {}  # grow-only scratch of the functional entry points, per use and device


def _check_scratch(scratch, nbytes: int, device):
    if not (isinstance(scratch, torch.Tensor) and scratch.is_cuda and scratch.is_contiguous() and scratch.device == device
            and scratch.numel() * scratch.element_size() >= nbytes):
        raise ValueError(f"scratch must be a contiguous HIP tensor of at least {nbytes} bytes on the image's device")
    return scratch


def normal_loss_scratch_bytes(W: int, H: int) -> int:
    return int(L.load().gsr_normal_loss_scratch_bytes(int(W), int(H)))


def depth_normal_loss(image: torch.Tensor, camera: Camera, weight: float = NORMAL_CONSISTENCY_WEIGHT, weights: bool = False,
                      stats: bool = False, scratch: torch.Tensor = None):
    """weight · depth_normal_consistency_loss (geometry_regularization.jl:87-183) of a :rgbdn frame as a 0-d tensor; a view
    with too little evidence gives exactly 0 (decided on the device).  `weights=True` also returns the detached weight map
    (H, W); `stats=True` the device pair (Σw, count).  `scratch` (optional, caller-owned, >= normal_loss_scratch_bytes):
    what `depth_normal_loss_backward_` of the same image reads; by default a buffer kept per device and image size."""
    H, W, _ = _check_frame(image).shape
    cs = _camera_struct(camera, W, H)
    lib = L.load()
    nb = int(lib.gsr_normal_loss_scratch_bytes(W, H))
    buf = _scratch(_SCRATCH, ("normal", W, H, image.device), nb, image.device) if scratch is None else \
        _check_scratch(scratch, nb, image.device)
    loss = torch.empty((), dtype=torch.float32, device=image.device)
    st = torch.empty(2, dtype=torch.float32, device=image.device)
    wmap = torch.empty((H, W), dtype=torch.float32, device=image.device) if weights else None
    with torch.cuda.device(image.device):
        L.check(lib.gsr_normal_loss_forward(W, H, 8, image.data_ptr(), C.byref(cs), float(weight), loss.data_ptr(),
                                            st.data_ptr(), None if wmap is None else wmap.data_ptr(), buf.data_ptr(),
                                            buf.numel() * buf.element_size(), L.stream()))
    out = (loss,) + ((wmap,) if weights else ()) + ((st,) if stats else ())
    return out[0] if len(out) == 1 else out


def depth_normal_loss_backward_(image: torch.Tensor, camera: Camera, vpixels: torch.Tensor,
                                weight: float = NORMAL_CONSISTENCY_WEIGHT, scratch: torch.Tensor = None) -> torch.Tensor:
    """ADDS weight · ∂depth_normal_consistency_loss/∂(D, α, normal) onto channels 3..7 of `vpixels` (H, W, 8), in place;
    channels 0..2 are not touched.  Needs `depth_normal_loss` of the same image (and the same `scratch`) run before it: the
    gate and the normaliser are read from what it left on the device.  Run-to-run bit-identical.  A `vpixels` this was
    added onto must go to `backward_raw` with `color_cotangent=False`."""
    H, W, _ = _check_frame(image).shape
    _check_frame(vpixels, "vpixels")
    if vpixels.shape != image.shape or vpixels.device != image.device:
        raise ValueError("vpixels must have the image's shape and device")
    if vpixels.data_ptr() == image.data_ptr():
        raise ValueError("vpixels must not be the image")
    cs = _camera_struct(camera, W, H)
    lib = L.load()
    nb = int(lib.gsr_normal_loss_scratch_bytes(W, H))
    if scratch is None:
        buf = _SCRATCH.get(("normal", W, H, image.device))
        if buf is None:
            raise ValueError("run depth_normal_loss of this image first: the backward reads what it left on the device")
    else:
        buf = _check_scratch(scratch, nb, image.device)
    with torch.cuda.device(image.device):
        L.check(lib.gsr_normal_loss_backward(W, H, 8, image.data_ptr(), C.byref(cs), float(weight), vpixels.data_ptr(),
                                             buf.data_ptr(), buf.numel() * buf.element_size(), L.stream()))
    return vpixels


def _check_scales(scales: torch.Tensor):
    if not (scales.is_cuda and scales.dtype == torch.float32 and scales.is_contiguous() and scales.dim() == 2
            and scales.shape[1] in (1, 3)):
        raise ValueError("scales must be a contiguous float32 (N, 3) or (N, 1) HIP tensor of raw scales")
    return scales


def flatten_loss(scales: torch.Tensor, weight: float = NORMAL_FLATTEN_WEIGHT, vscales: torch.Tensor = None,
                 scratch: torch.Tensor = None) -> torch.Tensor:
    """weight · flatten_loss(scales) (geometry_regularization.jl:197-211) = weight · mean_i exp(min_j scales[i, j]) over the
    RAW scales, as a 0-d tensor (0 for N = 0).  With `vscales` (N, 3) — the ∇scales `backward_raw` wrote, w.r.t. the
    ACTIVATED scale — the gradient weight / N is added onto it on each Gaussian's first minimal axis (column 0 for (N, 1)
    scales); `rasterizer.prologue_backward` / `optim.trainer_tail_step` then yield weight · exp(s) / N on the raw scale."""
    n, sd = _check_scales(scales).shape
    if vscales is not None:
        if not (vscales.is_cuda and vscales.dtype == torch.float32 and vscales.is_contiguous()
                and tuple(vscales.shape) == (n, 3) and vscales.device == scales.device):
            raise ValueError("vscales must be a contiguous float32 (N, 3) HIP tensor on the scales' device")
    lib = L.load()
    nb = int(lib.gsr_flatten_loss_scratch_bytes(n))
    buf = _scratch(_SCRATCH, ("flatten", scales.device), nb, scales.device) if scratch is None else \
        _check_scratch(scratch, nb, scales.device)
    loss = torch.empty((), dtype=torch.float32, device=scales.device)
    with torch.cuda.device(scales.device):
        L.check(lib.gsr_flatten_loss(n, sd, scales.data_ptr() if n else None, float(weight), loss.data_ptr(),
                                     None if vscales is None or n == 0 else vscales.data_ptr(), buf.data_ptr(),
                                     buf.numel() * buf.element_size(), L.stream()))
    return loss


class _DepthNormalLoss(torch.autograd.Function):
    """depth_normal_consistency_loss under AD: w.r.t. the frame (channels 3..7; the rgb channels get zeros)."""

    @staticmethod
    def forward(ctx, image, camera, weight):
        image = image.detach().contiguous()
        ctx.scratch = torch.empty(max(normal_loss_scratch_bytes(image.shape[1], image.shape[0]), 4), dtype=torch.uint8,
                                  device=image.device)
        ctx.save_for_backward(image)
        ctx.camera, ctx.weight = camera, float(weight)
        return depth_normal_loss(image, camera, weight, scratch=ctx.scratch)

    @staticmethod
    def backward(ctx, delta):
        (image,) = ctx.saved_tensors
        v = torch.zeros_like(image)
        depth_normal_loss_backward_(image, ctx.camera, v, ctx.weight, scratch=ctx.scratch)
        return v * delta, None, None


class _FlattenLoss(torch.autograd.Function):
    """flatten_loss under AD, w.r.t. the raw scales."""

    @staticmethod
    def forward(ctx, scales, weight):
        scales = scales.detach().contiguous()
        ctx.save_for_backward(scales)
        ctx.weight = float(weight)
        return flatten_loss(scales, weight)

    @staticmethod
    def backward(ctx, delta):
        (scales,) = ctx.saved_tensors
        v = torch.zeros((scales.shape[0], 3), dtype=torch.float32, device=scales.device)
        flatten_loss(scales, ctx.weight, vscales=v)
        return v[:, :scales.shape[1]] * torch.exp(scales) * delta, None   # the prologue's pullback: ∂exp(s)/∂s


def depth_normal_consistency_loss(image: torch.Tensor, camera: Camera, weight: float = 1.0) -> torch.Tensor:
    """weight · depth_normal_consistency_loss, differentiable w.r.t. the (H, W, 8) frame."""
    return _DepthNormalLoss.apply(image, camera, weight)


def flatten_loss_autograd(scales: torch.Tensor, weight: float = 1.0) -> torch.Tensor:
    """weight · flatten_loss(scales), differentiable w.r.t. the raw (N, 3) / (N, 1) scales."""
    return _FlattenLoss.apply(scales, weight)


def l1_ssim_normal_loss(rast, image: torch.Tensor, target: torch.Tensor, camera: Camera, scales: torch.Tensor = None,
                        lambda_dssim: float = 0.2, normal_weight: float = NORMAL_CONSISTENCY_WEIGHT,
                        flatten_weight: float = NORMAL_FLATTEN_WEIGHT, bgrid=None, view: int = None):
    """The loss of `step!` with `use_normal_loss` (training.jl:625-733): the fused L1 / D-SSIM loss head (through the
    view's bilateral grid when `bgrid` and `view` are given: its pullback touches channels 0..2 only), then the
    depth-normal consistency term ADDED onto channels 3..7 of the head's cotangent.  Returns (photometric, normal_term,
    flatten_term, vpixels); flatten_term is None without `scales` (raw).

    This `vpixels` carries depth / alpha / normal cotangents: it must go to `backward_raw` with `color_cotangent=False`.
    The flatten gradient joins after the backward: `flatten_loss(scales, flatten_weight, vscales=...)` on the ∇scales it
    wrote, then `optim.trainer_tail_step` (the fused backward + tail has no gradient arrays to add it to)."""
    _check_frame(image)
    if bgrid is not None:
        from . import bilateral_grid
        loss, vpix = bilateral_grid.l1_ssim_bilateral_loss(rast, image, target, bgrid, view, lambda_dssim)
    else:
        loss, vpix = fused_ssim.l1_ssim_loss(rast, image, target, lambda_dssim)
    normal_term = depth_normal_loss(image, camera, normal_weight)
    depth_normal_loss_backward_(image, camera, vpix, normal_weight)
    flatten_term = None if scales is None else flatten_loss(scales, flatten_weight)
    return loss, normal_term, flatten_term, vpix
