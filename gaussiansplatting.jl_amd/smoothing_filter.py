"""The 3-D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024, §4.1) on top of the gsr_filter3d_* entry points
(csrc/filter3d.hip) — the world-space companion of `GaussianRasterizer(antialiased=True)`.

Every Gaussian is low-pass filtered by the highest rate at which any training camera samples it:

    filter = compute_filter_3d(points, cameras)              # after every densification round: the points changed
    shs, oa, sa = _Prologue.apply(dc, rest, opacities, scales)
    oe, se = apply_filter_3d(oa, sa, filter)                 # autograd: forward and pullback are the library's kernels
    image = rasterize(points, shs, oe, se, rotations, rast=rast, camera=camera, ...)

The filter is a constant of the step (it is recomputed, never differentiated).  A training step without autograd runs
`rast.backward_raw` + `apply_filter_3d_backward_` (in place on vopacities / vscales) + `optim.trainer_tail_step`; the fused
`optim.fused_backward_tail_step` never materialises ∇scales / ∇opacities and cannot carry the extra chain step — as with
`geometry_regularization.flatten_loss`.  `merged_raw` gives the raw opacities / scales of the filtered model, for export.

Layouts: points (N, 3), opacities_act (N, 1) or (N,), scales_act (N, 3) as `prologue_forward` writes them, filter (N,)."""
from __future__ import annotations

import math

import numpy as np

import torch

from . import _args as A
from . import _lib as L

f32 = np.float32

CAMERA_FLOATS = L.FILTER3D_CAMERA_FLOATS
FILTER_MARGIN = 0.15     # a point counts as seen up to 15 % of the resolution outside the image (Mip-Splatting)
FILTER_VARIANCE = 0.2    # the variance of the filter in units of the sampling interval (Mip-Splatting)
NEAR = 0.2


def filter_scale(variance: float = FILTER_VARIANCE) -> np.float32:
    """k of gsr_filter3d_compute: f32(sqrt(variance))."""
    if not (isinstance(variance, (int, float, np.floating)) and math.isfinite(variance) and variance >= 0):
        raise ValueError(f"variance = {variance!r} must be a finite number >= 0")
    return f32(math.sqrt(float(variance)))


def camera_table(cameras, margin: float = FILTER_MARGIN) -> np.ndarray:
    """The (V, CAMERA_FLOATS) float32 table gsr_filter3d_compute sweeps, from objects with `width`, `height`, `focal`,
    `principal`, `R` (world -> camera, row-major) and `t` (camera.Camera): R column-major, t, focal,
    pp = f32(principal) · f32(res), lo = f32(-margin) · f32(res), hi = f32(1 + margin) · f32(res),
    inv_f = f32(1) / max(f32(fx), f32(fy)), one pad word (0).  Every product is one fp32 operation."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("no cameras: the 3-D filter is the sampling rate of at least one view")
    if not (isinstance(margin, (int, float, np.floating)) and math.isfinite(margin) and margin >= 0):
        raise ValueError(f"margin = {margin!r} must be a finite number >= 0")
    table = np.zeros((len(cameras), CAMERA_FLOATS), f32)
    for row, cam in zip(table, cameras):
        R = np.asarray(cam.R, f32)
        t = np.asarray(cam.t, f32)
        if R.shape != (3, 3) or t.shape != (3,):
            raise ValueError("a camera's R must be (3, 3) and its t (3,)")
        focal = np.array([cam.focal[0], cam.focal[1]], f32)
        if not (focal > 0).all():
            raise ValueError("focal lengths must be positive")
        res = np.array([cam.width, cam.height], f32)
        row[0:9] = R.T.reshape(-1)          # column-major: row[i + 3 j] = R[i, j]
        row[9:12] = t
        row[12:14] = focal
        row[14:16] = np.array([cam.principal[0], cam.principal[1]], f32) * res
        row[16:18] = f32(-margin) * res
        row[18:20] = f32(1.0 + margin) * res
        row[20] = f32(1) / max(focal[0], focal[1])
    return table


def _points(points):
    if not (isinstance(points, torch.Tensor) and points.is_cuda):
        raise ValueError("points must be a HIP device tensor (no CPU path)")
    return A.check(points, "points must be a contiguous float32 (N, 3) HIP tensor", shape=(None, 3))


def _table(cameras, margin, device):
    if isinstance(cameras, torch.Tensor):
        return A.check(cameras, f"a camera table must be a contiguous float32 (V, {CAMERA_FLOATS}) HIP tensor on the points' device",
                       shape=(None, CAMERA_FLOATS), device=device)
    if isinstance(cameras, np.ndarray):
        if cameras.dtype != f32 or cameras.ndim != 2 or cameras.shape[1] != CAMERA_FLOATS:
            raise ValueError(f"a camera table must be a float32 (V, {CAMERA_FLOATS}) array")
        host = np.ascontiguousarray(cameras)
    else:
        host = camera_table(cameras, margin)
    return torch.from_numpy(host).to(device)


def compute_filter_3d(points: torch.Tensor, cameras, near: float = NEAR, variance: float = FILTER_VARIANCE,
                      return_seen: bool = False, margin: float = FILTER_MARGIN):
    """The filter (N,) of `points` (N, 3) under `cameras`: a sequence of cameras (`camera_table(cameras, margin)` is built
    and uploaded), a (V, CAMERA_FLOATS) float32 numpy table, or such a table already on the device (the trainer's: built once).
    Per point the smallest depth / max(focal) over the cameras that see it (depth > `near`, projection inside the image
    grown by the table's margin) times sqrt(variance); a point no camera sees gets the largest filter of the others.
    `return_seen`: also the (N,) uint8 seen flags and the 1-element int32 count of seen points, both left on the device.
    Nothing is read back: the call is asynchronous.  Run-to-run bit-identical."""
    n = int(_points(points).shape[0])
    k = filter_scale(variance)
    if not (isinstance(near, (int, float, np.floating)) and math.isfinite(near) and near >= 0):
        raise ValueError(f"near = {near!r} must be a finite number >= 0")
    table = _table(cameras, margin, points.device)
    if table.shape[0] < 1:
        raise ValueError("no cameras: the 3-D filter is the sampling rate of at least one view")
    dev = points.device
    out = torch.empty(n, dtype=torch.float32, device=dev)
    seen = torch.empty(n, dtype=torch.uint8, device=dev) if return_seen else None
    count = torch.zeros(1, dtype=torch.int32, device=dev) if return_seen else None
    if n > 0:
        lib = L.load()
        nb = int(lib.gsr_filter3d_scratch_bytes(n))
        scratch = torch.empty(nb, dtype=torch.uint8, device=dev)  # (torch allocations are 256-byte aligned)
        with torch.cuda.device(dev):
            L.check(lib.gsr_filter3d_compute(n, L.ptr(points), int(table.shape[0]), L.ptr(table), float(near), float(k), L.ptr(out),
                                             L.ptr(seen), L.ptr(count), L.ptr(scratch), nb, L.stream()))
    return (out, seen, count) if return_seen else out


def _rows(opacities_act, scales_act, filter):
    """The three arrays of one model, checked: -> n."""
    scales_act = A.check(scales_act, "scales_act must be a contiguous float32 (N, 3) HIP tensor", shape=(None, 3))
    n, dev = int(scales_act.shape[0]), scales_act.device
    A.check(opacities_act, "opacities_act must be a contiguous float32 HIP tensor of N elements on the scales' device", device=dev)
    A.check(filter, "filter must be a contiguous float32 (N,) HIP tensor on the scales' device", shape=(n,), device=dev)
    if opacities_act.numel() != n or opacities_act.dim() not in (1, 2):
        raise ValueError("opacities_act must be a contiguous float32 HIP tensor of N elements on the scales' device")
    return n


def _apply(opacities_act, scales_act, filter, raw: bool):
    n = _rows(opacities_act, scales_act, filter)
    oe, se = torch.empty_like(opacities_act), torch.empty_like(scales_act)
    with torch.cuda.device(scales_act.device):
        L.check(L.load().gsr_filter3d_apply(n, L.ptr(opacities_act), L.ptr(scales_act), L.ptr(filter), 1 if raw else 0, L.ptr(oe),
                                            L.ptr(se), L.stream()))
    return oe, se


def _apply_backward(opacities_act, scales_act, filter, g_opacities, g_scales, v_opacities, v_scales):
    n = _rows(opacities_act, scales_act, filter)
    for t, like, nm in ((g_opacities, opacities_act, "the opacity cotangent"), (g_scales, scales_act, "the scale cotangent"),
                        (v_opacities, opacities_act, "the opacity gradient"), (v_scales, scales_act, "the scale gradient")):
        A.check(t, f"{nm} must be a contiguous float32 HIP tensor like its parameter", device=like.device)
        if t.numel() != like.numel():
            raise ValueError(f"{nm} must be a contiguous float32 HIP tensor like its parameter")
    with torch.cuda.device(scales_act.device):
        L.check(L.load().gsr_filter3d_apply_backward(n, L.ptr(opacities_act), L.ptr(scales_act), L.ptr(filter), L.ptr(g_opacities),
                                                     L.ptr(g_scales), L.ptr(v_opacities), L.ptr(v_scales), L.stream()))
    return v_opacities, v_scales


def apply_filter_3d_forward(opacities_act, scales_act, filter):
    """(opacities_eff, scales_eff) of gsr_filter3d_apply, no autograd: se = sqrt(s² + f²) per axis, o_eff = o · Π s/se."""
    return _apply(opacities_act, scales_act, filter, raw=False)


def apply_filter_3d_backward(opacities_act, scales_act, filter, g_opacities, g_scales):
    """The pullback of `apply_filter_3d_forward` into fresh tensors: (v_opacities, v_scales) w.r.t. the activated values from
    the cotangents w.r.t. the effective ones (`backward_raw`'s vopacities / vscales)."""
    return _apply_backward(opacities_act, scales_act, filter, g_opacities, g_scales, torch.empty_like(g_opacities),
                           torch.empty_like(g_scales))


def apply_filter_3d_backward_(opacities_act, scales_act, filter, vopacities, vscales):
    """The same in place: `vopacities` / `vscales` — the arrays `backward_raw` wrote — become the gradients w.r.t. the
    activated values, ready for `prologue_backward` / `optim.trainer_tail_step`.  Bit-identical to the out-of-place form."""
    return _apply_backward(opacities_act, scales_act, filter, vopacities, vscales, vopacities, vscales)


class _ApplyFilter3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacities_act, scales_act, filter):
        o, s, f = (t.detach().contiguous() for t in (opacities_act, scales_act, filter))
        ctx.save_for_backward(o, s, f)
        return _apply(o, s, f, raw=False)

    @staticmethod
    def backward(ctx, g_o, g_s):
        o, s, f = ctx.saved_tensors
        g_o = torch.zeros_like(o) if g_o is None else g_o.contiguous()
        g_s = torch.zeros_like(s) if g_s is None else g_s.contiguous()
        vo, vs = apply_filter_3d_backward(o, s, f, g_o, g_s)
        return vo, vs, None


def apply_filter_3d(opacities_act, scales_act, filter):
    """(opacities_eff, scales_eff) under autograd, between `_Prologue` and `rasterize`; differentiable w.r.t. the activated
    opacities and scales, the filter is a constant."""
    return _ApplyFilter3D.apply(opacities_act, scales_act, filter)


def merged_raw(opacities_act, scales_act, filter):
    """(opacities_raw, scales_raw) of the filtered model — logit(o_eff) and log(se), what a .ply stores — so that an exported
    model renders filtered in any viewer (the original's `save_fused_ply`)."""
    return _apply(opacities_act, scales_act, filter, raw=True)
