"""Host mirror of src/bilateral_grid.jl (bilateral grid appearance correction) on top of the gsr_bilateral_* entry
points, and of its use in `Trainer.step!` (training.jl:676-706,784-790, update_lr! :813-818).

Each training image owns a low-resolution `(x, y, guidance)` grid of 3x4 affine colour transforms.  The current view's
grid is sliced trilinearly at (pixel x, pixel y, grey(rgb)) and applied to the render before L1 / D-SSIM; a total-variation
prior over all grids joins the loss; one `NU.Adam` updates all grids every step.

Layouts: all grids are one (n, 12, gz, gy, gx) tensor ≙ the reference's (gx, gy, gz, 12, n); a view's grid is
(12, gz, gy, gx); images are (H, W, C) ≙ (C, W, H), C = 3, 5 or 8 (the rasterizer's modes)."""
from __future__ import annotations

import numpy as np
import torch

from . import _args as A
from . import _lib as L
from .optim import Adam

GRID_SIZE = (16, 16, 8)  # bilateral_grid_size (utils.jl:60): (x, y, guidance)


def lr_exp_scheduler(lr_start: float, lr_end: float, steps: int):
    """utils.jl:75-83, in float32 as the reference evaluates it."""
    f32 = np.float32
    a, b = f32(lr_start), f32(lr_end)

    def _scheduler(step: int) -> np.float32:
        if step < 0 or (a == 0 and b == 0):
            return f32(0.0)
        t = min(max(f32(step / steps), f32(0.0)), f32(1.0))
        return f32(np.exp(f32(np.log(a) * (f32(1.0) - t)) + f32(np.log(b) * t)))
    return _scheduler


def bilateral_grid_scheduler(lr: float, steps: int, warmup_steps: int = 1000, warmup_start: float = 0.01,
                             final_factor: float = 0.01):
    """bilateral_grid.jl:45-64: linear warm-up from 1 % of `lr` over the first 1000 steps, then exponential decay to 1 %
    of `lr` by `steps`."""
    f32 = np.float32
    lr, ws, ff = f32(lr), f32(warmup_start), f32(final_factor)
    decay = lr_exp_scheduler(lr, f32(ff * lr), steps)

    def _scheduler(step: int) -> np.float32:
        warmup = f32(ws + f32((f32(1.0) - ws) * f32(step / warmup_steps))) if step < warmup_steps else f32(1.0)
        return f32(warmup * decay(step))
    return _scheduler


_check_image = A.frame_check((3, 5, 8), "{} must be a contiguous float32 (H, W, C) HIP tensor with C in (3, 5, 8)")


def _check_grid(grid: torch.Tensor):
    return A.check(grid, "grid must be a contiguous float32 (12, gz, gy, gx) HIP tensor", shape=(12, None, None, None))


_SCRATCH: dict = {}  # grow-only scratch of the functional entry points, per device


def slice_forward(image: torch.Tensor, grid: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """`bilateral_slice(image, grid)` (bilateral_grid.jl:75-85): rgb corrected, channels >= 3 copied."""
    H, W, Cc = _check_image(image).shape
    gz, gy, gx = _check_grid(grid).shape[1:]
    out = torch.empty_like(image) if out is None else A.check_same(_check_image(out, "out"), "out", image)
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_bilateral_slice_forward(W, H, Cc, image.data_ptr(), grid.data_ptr(), gx, gy, gz, out.data_ptr(),
                                                     L.stream()))
    return out


def slice_backward(image: torch.Tensor, grid: torch.Tensor, vout: torch.Tensor, vimage: torch.Tensor = None,
                   vgrid: torch.Tensor = None, scratch: dict = None):
    """The pullback (bilateral_grid.jl:87-100): -> (∇image, ∇grid).  `vimage` may be `vout` (in place); `vgrid` is
    overwritten.  Run-to-run bit-identical."""
    H, W, Cc = _check_image(image).shape
    gz, gy, gx = _check_grid(grid).shape[1:]
    A.check_same(_check_image(vout, "vout"), "vout", image)
    vimage = torch.empty_like(image) if vimage is None else A.check_same(_check_image(vimage, "vimage"), "vimage", image)
    vgrid = torch.empty_like(grid) if vgrid is None else A.check_same(_check_grid(vgrid), "vgrid", grid, "grid")
    lib = L.load()
    nb = int(lib.gsr_bilateral_scratch_bytes(W, H, gx, gy, gz))
    buf = A.grow_scratch(_SCRATCH if scratch is None else scratch, "slice", nb, image.device)
    with torch.cuda.device(image.device):
        L.check(lib.gsr_bilateral_slice_backward(W, H, Cc, image.data_ptr(), grid.data_ptr(), gx, gy, gz, vout.data_ptr(),
                                                 vimage.data_ptr(), vgrid.data_ptr(), buf.data_ptr(), buf.numel(), L.stream()))
    return vimage, vgrid


def tv(grids: torch.Tensor, weight: float = 1.0, grad: bool = False, scratch: dict = None):
    """weight · tv_loss(grids) (bilateral_grid.jl:102-119) as a 0-d tensor, and weight · ∇tv_loss when `grad`."""
    A.check(grids, "grids must be a contiguous float32 (n, 12, gz, gy, gx) HIP tensor", shape=(None, 12, None, None, None))
    n, _, gz, gy, gx = grids.shape
    loss = torch.empty((), dtype=torch.float32, device=grids.device)
    g = torch.empty_like(grids) if grad else None
    lib = L.load()
    buf = A.grow_scratch(_SCRATCH if scratch is None else scratch, "tv", int(lib.gsr_bilateral_tv_scratch_bytes(n)), grids.device)
    with torch.cuda.device(grids.device):
        L.check(lib.gsr_bilateral_tv(n, gx, gy, gz, grids.data_ptr(), float(weight), loss.data_ptr(),
                                     None if g is None else g.data_ptr(), buf.data_ptr(), buf.numel(), L.stream()))
    return (loss, g) if grad else loss


class _BilateralSlice(torch.autograd.Function):
    """CRC.rrule(::typeof(bilateral_slice), image, grid) — bilateral_grid.jl:87-100"""

    @staticmethod
    def forward(ctx, image, grid):
        image, grid = image.detach().contiguous(), grid.detach().contiguous()
        ctx.save_for_backward(image, grid)
        return slice_forward(image, grid)

    @staticmethod
    def backward(ctx, delta):
        image, grid = ctx.saved_tensors
        return slice_backward(image, grid, delta.contiguous())


class _TvLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        grids = grids.detach().contiguous()
        ctx.save_for_backward(grids)
        return tv(grids)

    @staticmethod
    def backward(ctx, delta):
        (grids,) = ctx.saved_tensors
        return tv(grids, grad=True)[1] * delta


def bilateral_slice(image: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    """bilateral_slice(image, grid), differentiable w.r.t. both (image (H, W, C), grid (12, gz, gy, gx))."""
    return _BilateralSlice.apply(image, grid)


def tv_loss(grids: torch.Tensor) -> torch.Tensor:
    """tv_loss(grids), differentiable (grids (n, 12, gz, gy, gx))."""
    return _TvLoss.apply(grids)


class BilateralGrid:
    """`BilateralGrid(kab, n_images, opt_params)` (bilateral_grid.jl:14-35): identity-initialised grids, one NU.Adam
    (ϵ = 1e-15) over all of them and the learning-rate schedule.  Also holds the slice gradient of the view the loss was
    last taken on (`vgrid`), which `step` folds into the update."""

    def __init__(self, n_images: int, size=GRID_SIZE, lr: float = 2e-3, lr_steps: int = 30_000, device="cuda"):
        gx, gy, gz = (int(s) for s in size)
        if n_images < 1 or min(gx, gy, gz) < 1:
            raise ValueError("n_images and every grid side must be >= 1")
        self.size = (gx, gy, gz)
        self.grids = torch.zeros((n_images, 12, gz, gy, gx), dtype=torch.float32, device=device)
        for d in range(3):  # identity transform in every cell
            self.grids[:, d * 4 + d] = 1.0
        self.optimizer = Adam(self.grids, lr, eps=1e-15)
        self.scheduler = bilateral_grid_scheduler(lr, lr_steps)
        self.vgrid = torch.zeros((12, gz, gy, gx), dtype=torch.float32, device=self.grids.device)
        self.vgrid_view = None
        self.tv_term = torch.zeros((), dtype=torch.float32, device=self.grids.device)
        self._scratch: dict = {}

    @property
    def n_images(self) -> int:
        return int(self.grids.shape[0])

    def grid(self, view: int) -> torch.Tensor:
        """bgrids[:, :, :, :, view] (0-based view)."""
        return self.grids[view]

    def memory_usage(self) -> int:
        """bilateral_grid.jl:37-38: bytes of the grids and the optimizer's moments."""
        return sum(t.numel() * t.element_size() for t in (self.grids, self.optimizer.mu, self.optimizer.nu))

    def slice(self, image: torch.Tensor, view: int) -> torch.Tensor:
        return slice_forward(image, self.grid(view))

    def slice_backward_(self, image: torch.Tensor, view: int, vout: torch.Tensor) -> torch.Tensor:
        """Pullback of `slice(image, view)` IN PLACE on `vout`; the view's ∇grid is kept for `step`."""
        slice_backward(image, self.grid(view), vout, vimage=vout, vgrid=self.vgrid, scratch=self._scratch)
        self.vgrid_view = int(view)
        return vout

    def step(self, view: int, trainer_step: int, tv_weight: float = 10.0) -> torch.Tensor:
        """update_lr! (training.jl:816) + `NU.step!(bgrid.optimizer, bgrid.grids, ∇grids)` (:784-790), where ∇grids =
        tv_weight · ∇tv_loss + the slice gradient of `view`, in one pass (gsr_bilateral_adam_tail).  Returns the TV term
        tv_weight · tv_loss(grids) of the grids BEFORE the update (training.jl:704-705) as a 0-d tensor."""
        if self.vgrid_view != int(view):
            raise ValueError(f"no slice gradient of view {view}: run the loss (slice_backward_) of that view first")
        n, _, gz, gy, gx = self.grids.shape
        o = self.optimizer
        o.lr = float(self.scheduler(int(trainer_step)))
        lib = L.load()
        buf = A.grow_scratch(self._scratch, "tv", int(lib.gsr_bilateral_tv_scratch_bytes(n)), self.grids.device)
        with torch.cuda.device(self.grids.device):
            L.check(lib.gsr_bilateral_adam_tail(n, gx, gy, gz, self.grids.data_ptr(), o.mu.data_ptr(), o.nu.data_ptr(),
                                                self.vgrid.data_ptr(), int(view), float(tv_weight), o.lr, o.current_step + 1,
                                                o.beta1, o.beta2, o.eps, self.tv_term.data_ptr(), buf.data_ptr(), buf.numel(),
                                                L.stream()))
        o.current_step += 1  # committed after validation and a successful launch
        self.vgrid_view = None
        return self.tv_term


def l1_ssim_bilateral_loss(rast, image: torch.Tensor, target: torch.Tensor, bgrid: BilateralGrid, view: int,
                           lambda_dssim: float = 0.2):
    """training.jl:676-694 with the appearance correction alone: `training_loss(..., bgrid=, view=)`.  Returns (photometric
    loss, vpixels): vpixels is the cotangent w.r.t. the RAW render (`StepLoss.color_cotangent` stays true), and the view's
    ∇grid stays in `bgrid` for `bgrid.step`."""
    from .training_loss import training_loss
    step = training_loss(rast, _check_image(image), target, lambda_dssim=lambda_dssim, bgrid=bgrid, view=view)
    return step.photometric, step.vpixels
