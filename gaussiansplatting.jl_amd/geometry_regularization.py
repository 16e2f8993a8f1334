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

from . import _args as A
from . import _lib as L
from .camera import Camera

NORMAL_CONSISTENCY_WEIGHT = 0.05   # normal_consistency_weight (utils.jl)
NORMAL_FLATTEN_WEIGHT = 0.005      # this package's default of normal_flatten_weight


check_frame = A.frame_check((8,), "{} must be a contiguous float32 (H, W, 8) HIP tensor (a :rgbdn frame)")


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


def normal_loss_scratch_bytes(W: int, H: int) -> int:
    return int(L.load().gsr_normal_loss_scratch_bytes(int(W), int(H)))


_SCRATCH = A.FrameScratch(normal_loss_scratch_bytes, min_bytes=4)  # what depth_normal_loss leaves for its backward
_FLATTEN_SCRATCH: dict = {}  # grow-only scratch of flatten_loss, per device


def depth_normal_loss(image: torch.Tensor, camera: Camera, weight: float = NORMAL_CONSISTENCY_WEIGHT, weights: bool = False,
                      stats: bool = False, scratch: torch.Tensor = None):
    """weight · depth_normal_consistency_loss (geometry_regularization.jl:87-183) of a :rgbdn frame as a 0-d tensor; a view
    with too little evidence gives exactly 0 (decided on the device).  `weights=True` also returns the detached weight map
    (H, W); `stats=True` the device pair (Σw, count).  `scratch` (optional, caller-owned, >= normal_loss_scratch_bytes):
    what `depth_normal_loss_backward_` of the same image reads; by default a buffer kept per device and image size."""
    H, W, _ = check_frame(image).shape
    cs = _camera_struct(camera, W, H)
    buf = _SCRATCH.get(scratch, W, H, image.device)
    loss = torch.empty((), dtype=torch.float32, device=image.device)
    st = torch.empty(2, dtype=torch.float32, device=image.device)
    wmap = torch.empty((H, W), dtype=torch.float32, device=image.device) if weights else None
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_normal_loss_forward(W, H, 8, image.data_ptr(), C.byref(cs), float(weight), loss.data_ptr(),
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
    H, W, _ = check_frame(image).shape
    A.check_vpixels(check_frame, vpixels, image)
    cs = _camera_struct(camera, W, H)
    buf = _SCRATCH.get(scratch, W, H, image.device, create=False)
    if buf is None:
        raise ValueError("run depth_normal_loss of this image first: the backward reads what it left on the device")
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_normal_loss_backward(W, H, 8, image.data_ptr(), C.byref(cs), float(weight), vpixels.data_ptr(),
                                                  buf.data_ptr(), buf.numel() * buf.element_size(), L.stream()))
    return vpixels


def flatten_loss(scales: torch.Tensor, weight: float = NORMAL_FLATTEN_WEIGHT, vscales: torch.Tensor = None,
                 scratch: torch.Tensor = None) -> torch.Tensor:
    """weight · flatten_loss(scales) (geometry_regularization.jl:197-211) = weight · mean_i exp(min_j scales[i, j]) over the
    RAW scales, as a 0-d tensor (0 for N = 0).  With `vscales` (N, 3) — the ∇scales `backward_raw` wrote, w.r.t. the
    ACTIVATED scale — the gradient weight / N is added onto it on each Gaussian's first minimal axis (column 0 for (N, 1)
    scales); `rasterizer.prologue_backward` / `optim.trainer_tail_step` then yield weight · exp(s) / N on the raw scale."""
    # (checked in line, not through _args.check: this launch takes 15 µs and the host path in front of it is what is timed)
    if not (scales.is_cuda and scales.dtype == torch.float32 and scales.is_contiguous() and scales.dim() == 2
            and scales.shape[1] in (1, 3)):
        raise ValueError("scales must be a contiguous float32 (N, 3) or (N, 1) HIP tensor of raw scales")
    n, sd = scales.shape
    if vscales is not None:
        if not (vscales.is_cuda and vscales.dtype == torch.float32 and vscales.is_contiguous()
                and tuple(vscales.shape) == (n, 3) and vscales.device == scales.device):
            raise ValueError("vscales must be a contiguous float32 (N, 3) HIP tensor on the scales' device")
    lib = L.load()
    nb = int(lib.gsr_flatten_loss_scratch_bytes(n))
    buf = A.grow_scratch(_FLATTEN_SCRATCH, scales.device, nb, scales.device, 4) if scratch is None else \
        A.check_scratch(scratch, nb, scales.device)
    loss = torch.empty((), dtype=torch.float32, device=scales.device)
    with torch.cuda.device(scales.device):
        L.check(lib.gsr_flatten_loss(n, sd, scales.data_ptr() if n else None, float(weight), loss.data_ptr(),
                                     None if vscales is None or n == 0 else vscales.data_ptr(), buf.data_ptr(),
                                     buf.numel() * buf.element_size(), L.stream()))
    return loss


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
    """weight · depth_normal_consistency_loss, differentiable w.r.t. the (H, W, 8) frame (channels 3..7; rgb gets zeros)."""
    weight = float(weight)
    return A.cotangent_term(image, lambda im, scratch: depth_normal_loss(im, camera, weight, scratch=scratch),
                            lambda im, v, scratch: depth_normal_loss_backward_(im, camera, v, weight, scratch=scratch),
                            lambda W, H: max(normal_loss_scratch_bytes(W, H), 4))


def flatten_loss_autograd(scales: torch.Tensor, weight: float = 1.0) -> torch.Tensor:
    """weight · flatten_loss(scales), differentiable w.r.t. the raw (N, 3) / (N, 1) scales."""
    return _FlattenLoss.apply(scales, weight)


def l1_ssim_normal_loss(rast, image: torch.Tensor, target: torch.Tensor, camera: Camera, scales: torch.Tensor = None,
                        lambda_dssim: float = 0.2, normal_weight: float = NORMAL_CONSISTENCY_WEIGHT,
                        flatten_weight: float = NORMAL_FLATTEN_WEIGHT, bgrid=None, view: int = None):
    """The loss of `step!` with `use_normal_loss` (training.jl:625-733), these terms only: `training_loss` with the
    depth-normal term and, given the raw `scales`, the flatten term.  Returns (photometric, normal_term, flatten_term,
    vpixels); flatten_term is None without `scales`.  `vpixels` carries depth / alpha / normal cotangents
    (`StepLoss.color_cotangent` is false).  The flatten gradient joins after the backward: `flatten_loss(scales,
    flatten_weight, vscales=...)` on the ∇scales it wrote, then `optim.trainer_tail_step` (the fused backward + tail has no
    gradient arrays to add it to)."""
    from . import training_loss as T
    out = T.training_loss(rast, check_frame(image), target, lambda_dssim=lambda_dssim, bgrid=bgrid, view=view,
                          normal=T.NormalTerm(camera, normal_weight),
                          flatten=None if scales is None else T.FlattenTerm(scales, flatten_weight))
    return out.photometric, out.normal_term, out.flatten_term, out.vpixels
