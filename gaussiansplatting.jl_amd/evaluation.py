"""Host mirror of the reference's evaluation protocol: `validate(trainer; quantize)` (src/training.jl:487-532) with `mse`,
`psnr` (utils.jl:107-109) and `quantize8` (utils.jl:118), and the 8-bit frame `gl_texture` / `to_image`
(rasterizer.jl:155-182) display, save and score.  The per-pixel work runs on the gsr_eval_* / gsr_frame_rgb8 entry points
(csrc/eval.hip): one launch scores a view — sky composite, 8-bit rounding and the u8 target's conversion in its loads —,
and the export shares its quantiser, so that scoring a quantised render equals scoring the picture that would be written.

Layouts: a frame is the rasterizer's (H, W, C) ≙ the reference's (C, W, H), C >= 3; the sky frame is (H, W, 3); a float
target is (3, H, W) ≙ (W, H, 3), as the loss head takes it; a byte target and an exported frame are (H, W, 3) uint8 ≙ the
dataset's (3, W, H); the SSIM map is (3, H, W).  Image file I/O is not built: `frame_rgb8` ends at the bytes."""
from __future__ import annotations

import numpy as np

from . import _args as A
from . import _lib as L

METRICS = ("eval_ssim", "eval_mse", "eval_psnr", "eval_l1")


def _check_scored(image, sky_rgb):
    message = "image must be a contiguous float32 (H, W, C >= 3) HIP tensor"
    H, W, Cn = A.check(image, message, shape=(None, None, None)).shape
    if Cn < 3:
        raise ValueError(message)
    if sky_rgb is not None:
        if Cn < 5:
            raise ValueError("a sky frame needs the alpha row of a :rgbd / :rgbdn frame (C >= 5): :rgb has none")
        A.check_like(sky_rgb, "sky_rgb", (H, W, 3), image.device)
    return H, W, Cn


def eval_scratch_bytes(W: int, H: int) -> int:
    return int(L.load().gsr_eval_scratch_bytes(int(W), int(H)))


_SCRATCH = A.FrameScratch(eval_scratch_bytes, align=8)  # eval_metrics' per-workgroup partials


def eval_metrics(image, target, sky_rgb=None, quantize: bool = False, ssim_map=None, out=None, scratch=None):
    """The scores of one view -> a (4,) device tensor {mean SSIM, MSE, PSNR, mean |x - y|} (`out`, or a new one) over the
    rgb channels of `image` (H, W, C), composited over `sky_rgb` (H, W, 3) when given and rounded to the 8-bit grid when
    `quantize` (training.jl:514-526).  `target`: float32 (3, H, W), or uint8 (H, W, 3) as the dataset stores images —
    converted as u · (1/255) in the kernel's loads.  `ssim_map` (3, H, W), when given, receives the SSIM map of the scored
    colours.  Nothing is read back: `.cpu()` the result, or let `validate` do it once for all views."""
    torch = A._torch()
    H, W, Cn = _check_scored(image, sky_rgb)
    if not isinstance(target, torch.Tensor):
        raise ValueError("target must be a HIP tensor")
    if target.dtype == torch.uint8:
        A.check_like(target, "target", (H, W, 3), image.device, torch.uint8)
        t32, t8 = None, target
    elif target.dtype == torch.float32:
        A.check_like(target, "target", (3, H, W), image.device)
        t32, t8 = target, None
    else:
        raise ValueError("target must be float32 (3, H, W) or uint8 (H, W, 3)")
    if ssim_map is not None:
        A.check_like(ssim_map, "ssim_map", (3, H, W), image.device)
        if ssim_map.data_ptr() == image.data_ptr():
            raise ValueError("ssim_map must not be the image")
    out = torch.empty(4, dtype=torch.float32, device=image.device) if out is None else A.check_like(out, "out", (4,), image.device)
    buf = _SCRATCH.get(scratch, W, H, image.device)
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_eval_metrics(W, H, Cn, image.data_ptr(), L.ptr(sky_rgb), L.ptr(t32), L.ptr(t8), 1 if quantize else 0,
                                          L.ptr(ssim_map), out.data_ptr(), buf.data_ptr(), L.stream()))
    return out


def frame_rgb8(image, sky_rgb=None, flip_rows: bool = False, out=None):
    """The 8-bit picture of a frame -> (H, W, 3) uint8 (`out`, or a new tensor): the rgb channels of `image`, composited over
    `sky_rgb` when given, each floor(clamp(x, 0, 1) · 255 + 0.5) — the level `eval_metrics(quantize=True)` scores, bit for
    bit.  flip_rows=True reverses the row order (`gl_texture`, rasterizer.jl:155-182).  The layout is the dataset's: an
    exported frame can be passed back as a uint8 `target`."""
    torch = A._torch()
    H, W, Cn = _check_scored(image, sky_rgb)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=image.device) if out is None else \
        A.check_like(out, "out", (H, W, 3), image.device, torch.uint8)
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_frame_rgb8(W, H, Cn, image.data_ptr(), L.ptr(sky_rgb), 1 if flip_rows else 0, out.data_ptr(), L.stream()))
    return out


def average_views(per_view) -> dict:
    """training.jl:492-496,524-531: each metric is the per-view values added up in fp32 in view order, then divided by the
    number of views; no views give zeros.  `per_view`: (V, 4) host array, columns as `eval_metrics` orders them."""
    per_view = np.asarray(per_view, np.float32).reshape(-1, len(METRICS))
    acc = np.zeros(len(METRICS), np.float32)
    if per_view.shape[0] == 0:
        return {k: 0.0 for k in METRICS}
    with np.errstate(invalid="ignore", over="ignore"):
        for row in per_view:
            acc = acc + row
        acc = acc / np.float32(per_view.shape[0])
    return {k: float(v) for k, v in zip(METRICS, acc)}


def _read_back(t):
    """THE device -> host copy of `validate`."""
    return t.cpu().numpy()


def validate(rast, points, acts, rotations, cameras, targets, sh_degree, background=(0.0, 0.0, 0.0), sky=None,
             quantize: bool = False):
    """`validate(trainer; quantize)` (training.jl:487-532) -> dict(eval_ssim, eval_mse, eval_psnr, eval_l1), each the mean
    over the views.  `acts` = (shs, σ(opacities), exp(scales)) as `prologue_forward` returns them; `cameras` and `targets`
    (float32 (3, H, W) or uint8 (H, W, 3) each) run in step.  Per view: a forward-only render, the dome's forward-only render
    when `sky` (a SkyDome) is given — pass the zero background a dome trains over —, and `eval_metrics` into row v of one
    (V, 4) device tensor; ONE read-back at the end.  quantize=True scores the 8-bit picture (the published numbers:
    GaussianSplatting.jl:329); False is the in-training readout (:182)."""
    torch = A._torch()
    cameras, targets = list(cameras), list(targets)
    if len(cameras) != len(targets):
        raise ValueError(f"{len(cameras)} cameras, {len(targets)} targets")
    if not cameras:
        return average_views(np.zeros((0, len(METRICS)), np.float32))
    shs, opacities_act, scales_act = acts
    if sky is not None:
        from .sky_dome import render_sky
    rows = torch.empty((len(cameras), len(METRICS)), dtype=torch.float32, device=points.device)
    scratch = torch.empty(eval_scratch_bytes(rast.width, rast.height), dtype=torch.uint8, device=points.device)
    bg = tuple(float(b) for b in background)
    for v, (camera, target) in enumerate(zip(cameras, targets)):
        image = rast.forward_raw(points, shs, opacities_act, scales_act, rotations, camera, sh_degree, bg, forward_only=True)
        sky_rgb = render_sky(sky, camera, forward_only=True) if sky is not None else None
        eval_metrics(image, target, sky_rgb, quantize, out=rows[v], scratch=scratch)
    return average_views(_read_back(rows))
