"""`training_loss` (gaussiansplatting.jl_amd/training_loss.py) on the MI355X: one call against the same primitive calls
written out by hand, in the same order, on the same handles and inputs.  The bar is BIT equality: both runs launch the same
deterministic kernels on the same inputs in the same order, and the library has no float atomics.  The heads it replaces
are held to the oracle by their own files (test_gpu_sky_dome.py, test_gpu_depth_supervision.py,
test_gpu_geometry_regularization.py, test_gpu_bilateral_grid.py); here: that the composition is those calls and nothing
else, for combinations no single head could express, and that `StepLoss.color_cotangent` is the right answer.

Shapes: 257 Gaussians, K = 4, 130 x 70 and 55 x 33 — the sizes of test_gpu_guarded_buffers.py that end in partial tiles and
strips."""
import numpy as np
import pytest
import torch

from hip_helpers import dev
from test_gpu_sky_dome import _bits, _mask

pytestmark = pytest.mark.gpu

N, K, DEG, LAMBDA, QSTEP = 257, 4, 1, 0.2, 1.0 / 255.0
BG = (0.0, 0.0, 0.0)


def _same(a, b):
    return (a is None and b is None) or (a.shape == b.shape and torch.equal(_bits(a.reshape(-1)), _bits(b.reshape(-1))))


class _Setup:
    """One rendered view and everything the terms read; the handles are shared by the two runs of a case."""

    def __init__(self, pkg, mode, W, H, bgrid=False, sky=False):
        T, DS, B, SD = pkg.training_loss, pkg.depth_supervision, pkg.bilateral_grid, pkg.sky_dome
        self.pkg, self.W, self.H = pkg, W, H
        s = pkg.synthetic.make_scene(N, W, H, DEG, 400 + N + W, sigma_px=4.0, K=K)
        self.camera = pkg.Camera(W, H, tuple(s.focal))
        self.rast = pkg.rasterizer.GaussianRasterizer(W, H, mode=mode, form_tuner=False)
        self.t = [dev(s.means), dev(s.shs), dev(s.opacities.reshape(-1, 1)), dev(s.scales), dev(s.rotations)]
        self.scales_raw = dev(s.scales_raw)
        self.image = self.rast.forward_raw(*self.t, self.camera, DEG, BG)
        self.target = dev(pkg.synthetic.make_target(W, H, N))
        self.bgrid = self.dome = None
        if bgrid:   # two images, every cell off the identity
            self.bgrid = B.BilateralGrid(2, size=(4, 3, 2))
            self.bgrid.grids += dev(np.random.default_rng(W).normal(scale=0.05, size=tuple(self.bgrid.grids.shape)))
        if sky:
            self.dome = SD.SkyDome(self.camera, 2048, "hemisphere", radius=50.0, color=(0.3, 0.5, 0.8))
        if mode != "rgb":   # a prior 15 % off the render, and sky-far where the scene is thin
            e = self.image[..., 3] / torch.clamp(self.image[..., 4], min=1e-6)
            prior = torch.where(self.image[..., 4] > 0.3, 1.0 / (1.15 * e + 0.15), torch.full_like(e, 0.004)).contiguous()
            self.depth = T.DepthTerm(prior, DS.DepthAnchor.from_support(1.0, 0.0, 0.15, 1.0, 0.25, 0.4), QSTEP, DS.depth_weight(1000))
        self.mask = dev(_mask(H, W))

    def close(self):
        if self.dome is not None:
            self.dome.close()
        self.rast.close()

    def gradients(self, vpixels, color_cotangent):
        return [g.clone() for g in self.rast.backward_raw(vpixels, *self.t, self.camera, DEG, BG, color_cotangent=color_cotangent)[:5]]

    def by_hand(self, view=None, sky=None, depth=None, normal=None, flatten=None):
        """The primitive calls in `training_loss`'s documented order -> a dict with StepLoss's field names."""
        pkg = self.pkg
        SD, DS, G, F = pkg.sky_dome, pkg.depth_supervision, pkg.geometry_regularization, pkg.fused_ssim
        out = dict.fromkeys(("sky_term", "vsky", "depth_term", "normal_term", "flatten_term"))
        shown = self.image
        if sky is not None:                                                                      # 1
            sky_rgb = SD.render_sky(sky.dome, sky.camera)
            shown = SD.composite_sky(self.image, sky_rgb, None, sky.mask, sky.weight)
            if sky.mask is not None:
                shown, out["sky_term"] = shown
        if view is not None:                                                                     # 2
            corrected = pkg.bilateral_grid.slice_forward(shown, self.bgrid.grid(view))
            out["photometric"], vp = F.l1_ssim_loss(self.rast, corrected, self.target, LAMBDA)
            self.bgrid.slice_backward_(shown, view, vp)
        else:
            out["photometric"], vp = F.l1_ssim_loss(self.rast, shown, self.target, LAMBDA)
        if sky is not None:                                                                      # 3
            out["vsky"] = SD.sky_composite_backward_(self.image, sky_rgb, vp, sky.mask, sky.weight)
        if depth is not None:                                                                    # 4
            out["depth_term"] = DS.depth_loss(self.image, depth.prior, depth.anchor, depth.qstep, depth.weight, depth.lambda_grad)
            DS.depth_loss_backward_(self.image, depth.prior, depth.anchor, depth.qstep, vp, depth.weight, depth.lambda_grad)
        if normal is not None:                                                                   # 5
            out["normal_term"] = G.depth_normal_loss(self.image, normal.camera, normal.weight)
            G.depth_normal_loss_backward_(self.image, normal.camera, vp, normal.weight)
        if flatten is not None:                                                                  # 6
            out["flatten_term"] = G.flatten_loss(flatten.scales, flatten.weight)
        out["vpixels"] = vp
        return out

    def both(self, view=None, **specs):
        """training_loss once (every tensor cloned: `render_sky` returns the dome rasterizer's own image), then the same
        by hand; asserts the bit equality of every field, of the grid's slice gradient and of the parameter gradients."""
        bgrid = self.bgrid if view is not None else None
        step = self.pkg.training_loss(self.rast, self.image, self.target, lambda_dssim=LAMBDA, bgrid=bgrid, view=view, **specs)
        got = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in step._asdict().items()}
        if bgrid is not None:
            got["vgrid"], got["vgrid_view"] = bgrid.vgrid.clone(), bgrid.vgrid_view
            bgrid.vgrid.fill_(float("nan"))
            bgrid.vgrid_view = None
        got["grads"] = self.gradients(step.vpixels, step.color_cotangent)
        want = self.by_hand(view, **specs)
        for k, v in want.items():
            print(f"[{self.W}x{self.H}] {k}: {None if v is None else (v.item() if v.dim() == 0 else float(v.abs().sum()))}")
            assert _same(got[k], v), k
        if bgrid is not None:
            assert _same(got["vgrid"], bgrid.vgrid) and got["vgrid_view"] == bgrid.vgrid_view == view
        for a, b in zip(got["grads"], self.gradients(want["vpixels"], False)):
            assert _same(a, b)
        return got


def test_every_term_at_once(pkg):
    """bgrid + sky with an active mask + depth + normal + flatten on a :rgbdn frame: no single head could express it."""
    T, G = pkg.training_loss, pkg.geometry_regularization
    S = _Setup(pkg, "rgbdn", 130, 70, bgrid=True, sky=True)
    try:
        got = S.both(view=1, sky=T.SkyTerm(S.dome, S.camera, S.mask, 0.7), depth=S.depth,
                     normal=T.NormalTerm(S.camera, G.NORMAL_CONSISTENCY_WEIGHT), flatten=T.FlattenTerm(S.scales_raw, G.NORMAL_FLATTEN_WEIGHT))
        assert got["color_cotangent"] is False
        assert all(got[k] is not None for k in ("sky_term", "vsky", "depth_term", "normal_term", "flatten_term"))
        assert got["vsky"].any().item() and got["vpixels"][..., 3:].any().item() and got["vgrid"].any().item()
    finally:
        S.close()


def test_sky_without_mask_and_depth(pkg):
    T = pkg.training_loss
    S = _Setup(pkg, "rgbd", 55, 33, sky=True)
    try:
        got = S.both(sky=T.SkyTerm(S.dome, S.camera), depth=S.depth)
        assert got["sky_term"] is None and got["color_cotangent"] is False and got["normal_term"] is None
        assert got["vsky"].any().item() and got["depth_term"].item() > 0
    finally:
        S.close()


def test_normal_and_flatten_is_the_normal_head(pkg):
    T, G = pkg.training_loss, pkg.geometry_regularization
    S = _Setup(pkg, "rgbdn", 55, 33)
    try:
        got = S.both(normal=T.NormalTerm(S.camera, 0.05), flatten=T.FlattenTerm(S.scales_raw, 0.005))
        assert got["color_cotangent"] is False
        head = G.l1_ssim_normal_loss(S.rast, S.image, S.target, S.camera, S.scales_raw, LAMBDA, 0.05, 0.005)
        for k, v in zip(("photometric", "normal_term", "flatten_term", "vpixels"), head):
            assert _same(got[k], v), k
    finally:
        S.close()


def test_bilateral_grid_alone_keeps_the_color_cotangent(pkg):
    S = _Setup(pkg, "rgb", 55, 33, bgrid=True)
    try:
        got = S.both(view=0)      # (its backward_raw ran with color_cotangent=True against the by-hand run's False)
        assert got["color_cotangent"] is True
        loss, vp = pkg.bilateral_grid.l1_ssim_bilateral_loss(S.rast, S.image, S.target, S.bgrid, 0, LAMBDA)
        assert _same(got["photometric"], loss) and _same(got["vpixels"], vp)
    finally:
        S.close()


def test_no_term_is_the_plain_head(pkg):
    S = _Setup(pkg, "rgbd", 55, 33)
    try:
        got = S.both()
        assert got["color_cotangent"] is True
        assert not _bits(got["vpixels"][..., 3:]).any().item()          # all-zero words, not merely == 0
        loss, vp = pkg.fused_ssim.l1_ssim_loss(S.rast, S.image, S.target, LAMBDA)
        assert _same(got["photometric"], loss) and _same(got["vpixels"], vp)
    finally:
        S.close()


def test_frame_scratch_cache(pkg):
    """The shared cache on device buffers: the module's grow-only buffer, and a caller's own handed back unchanged or
    refused for its size or its alignment."""
    A = pkg._args
    cache = A.FrameScratch(lambda W, H: 16 * W * H, align=16, min_bytes=4)
    device = torch.device("cuda", torch.cuda.current_device())
    assert cache.get(None, 8, 4, device, create=False) is None
    own = cache.get(None, 8, 4, device)
    assert own.numel() == 512 and own.dtype == torch.uint8 and cache.get(None, 8, 4, device, create=False) is own
    assert cache.get(None, 8, 4, device) is own and cache.get(None, 0, 0, device).numel() == 4
    mine = torch.zeros(512 + 16, dtype=torch.uint8, device=device)
    assert cache.get(mine, 8, 4, device) is mine and cache.get(mine.view(torch.float32), 8, 4, device, create=False).data_ptr() == mine.data_ptr()
    message = "scratch must be a contiguous, 16-byte aligned HIP tensor of at least 512 bytes on the image's device"
    for bad in (mine[:511], mine[4:516], mine[::2], mine.cpu(), None if torch.cuda.device_count() < 2 else mine.to("cuda:1")):
        if bad is not None:
            with pytest.raises(ValueError, match=message):
                cache.get(bad, 8, 4, device)
