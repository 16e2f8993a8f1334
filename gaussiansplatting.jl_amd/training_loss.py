"""The loss of one `Trainer.step!` (src/training.jl:593-733), composed ONCE: the fused L1 / D-SSIM head, optionally behind the
sky dome's composite and through the view's bilateral grid, and the terms that ADD onto channels >= 3 of the head's
cotangent.  `l1_ssim_bilateral_loss`, `l1_ssim_normal_loss`, `l1_ssim_depth_loss` and `l1_ssim_sky_loss` are this function
with one `use_*` option on.  Specs carry RESOLVED weights: schedules (`depth_weight(step)`, `sky_loss_from_iter`) stay with
the caller."""
from __future__ import annotations

import sys
import types
from typing import Any, NamedTuple, Optional

from . import depth_supervision as DS
from . import fused_ssim
from . import geometry_regularization as G
from . import sky_dome as SD


class SkyTerm(NamedTuple):
    """`use_sky_dome`: the SkyDome and the view's camera; `mask` (H, W), when given, adds weight · sky_opacity_loss; `rast`
    renders the dome at another resolution than its own rasterizer's (`SkyDome.view_rasterizer`)."""
    dome: Any
    camera: Any
    mask: Any = None
    weight: float = 1.0
    rast: Any = None


class DepthTerm(NamedTuple):
    """`use_depth_loss`: weight · ssi_depth_loss against the (H, W) prior mapped through the view's DepthAnchor."""
    prior: Any
    anchor: Any
    qstep: float
    weight: float
    lambda_grad: float = DS.DEPTH_LOSS_GRADIENT_WEIGHT


class NormalTerm(NamedTuple):
    """`use_normal_loss`: weight · depth_normal_consistency_loss of a :rgbdn frame seen by `camera`."""
    camera: Any
    weight: float = G.NORMAL_CONSISTENCY_WEIGHT


class FlattenTerm(NamedTuple):
    """weight · flatten_loss of the RAW scales: the value only (its gradient joins after the backward, `flatten_loss`)."""
    scales: Any
    weight: float = G.NORMAL_FLATTEN_WEIGHT


class StepLoss(NamedTuple):
    """What a step needs back: every value a 0-d device tensor, None for a term that was off.  `vpixels` (H, W, C) goes to the
    scene's `backward_raw`, `vsky` (H, W, 3) to `sky_backward`.  `color_cotangent`: whether `backward_raw` may still take
    `color_cotangent=True` for `vpixels` — true exactly when nothing was added onto its channels >= 3 (no sky, depth or
    normal term ran; the bilateral slice touches channels 0..2 only)."""
    photometric: Any
    vpixels: Any
    sky_term: Optional[Any]
    vsky: Optional[Any]
    depth_term: Optional[Any]
    normal_term: Optional[Any]
    flatten_term: Optional[Any]
    color_cotangent: bool


def training_loss(rast, image, target, *, lambda_dssim: float = 0.2, bgrid=None, view: int = None, sky: SkyTerm = None,
                  depth: DepthTerm = None, normal: NormalTerm = None, flatten: FlattenTerm = None) -> StepLoss:
    """`image` (H, W, C): the scene's frame as `rast` rendered it (over a ZERO background with `sky`), `target` (3, H, W).  A
    term whose spec is None is off.  The launch order is fixed, so that any combination gives the bits of the same calls
    made by hand: 1. `render_sky` + `composite_sky` (with the mask's loss); 2. the head on the composite, or on the image —
    with `bgrid` and `view` as slice -> head -> `slice_backward_`, the view's ∇grid staying in `bgrid`; 3.
    `sky_composite_backward_`; 4. `depth_loss` + `depth_loss_backward_`; 5. `depth_normal_loss` +
    `depth_normal_loss_backward_`; 6. `flatten_loss`.  Depth and normal read the SCENE frame, not the composite."""
    if bgrid is not None and view is None:
        raise ValueError("a bilateral grid needs the view whose grid slices the image")
    if normal is not None and normal.camera is None:
        raise ValueError("the depth-normal term needs the camera")
    for spec, module in ((sky, SD), (depth, DS), (normal, G)):   # before any launch: an :rgb frame has no such channels
        if spec is not None:
            module.check_frame(image)
    sky_rgb = sky_term = vsky = depth_term = normal_term = flatten_term = None
    shown = image   # what the head sees
    if sky is not None:
        sky_rgb = SD.render_sky(sky.dome, sky.camera, rast=sky.rast)
        shown = SD.composite_sky(image, sky_rgb, None, sky.mask, sky.weight)
        if sky.mask is not None:
            shown, sky_term = shown
    if bgrid is not None:
        photometric, vpixels = fused_ssim.l1_ssim_loss(rast, bgrid.slice(shown, view), target, lambda_dssim)
        bgrid.slice_backward_(shown, view, vpixels)
    else:
        photometric, vpixels = fused_ssim.l1_ssim_loss(rast, shown, target, lambda_dssim)
    if sky is not None:
        vsky = SD.sky_composite_backward_(image, sky_rgb, vpixels, sky.mask, sky.weight)
    if depth is not None:
        depth_term = DS.depth_loss(image, depth.prior, depth.anchor, depth.qstep, depth.weight, depth.lambda_grad)
        DS.depth_loss_backward_(image, depth.prior, depth.anchor, depth.qstep, vpixels, depth.weight, depth.lambda_grad)
    if normal is not None:
        normal_term = G.depth_normal_loss(image, normal.camera, normal.weight)
        G.depth_normal_loss_backward_(image, normal.camera, vpixels, normal.weight)
    if flatten is not None:
        flatten_term = G.flatten_loss(flatten.scales, flatten.weight)
    return StepLoss(photometric, vpixels, sky_term, vsky, depth_term, normal_term, flatten_term,
                    color_cotangent=sky is None and depth is None and normal is None)


class _Module(types.ModuleType):
    """The package's attribute `training_loss` is this module whenever any importer got here first, so the module itself
    is the function: `pkg.training_loss(rast, image, target, depth=pkg.training_loss.DepthTerm(...))`."""
    __call__ = staticmethod(training_loss)


sys.modules[__name__].__class__ = _Module
