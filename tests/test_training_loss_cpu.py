"""The shared argument plumbing (gaussiansplatting.jl_amd/_args.py) and `training_loss`'s refusals without a GPU: CPU tensors
can reach the error paths only — every message is the one the modules raised before they shared the code.  The paths that
need a device buffer are in test_gpu_training_loss.py."""
from types import SimpleNamespace

import pytest
import torch


@pytest.mark.parametrize("align,wording", [(16, "contiguous, 16-byte aligned HIP"), (8, "contiguous, 8-byte aligned HIP"), (1, "contiguous HIP")])
def test_frame_scratch_refuses_and_does_not_create(pkg, align, wording):
    asked = []
    cache = pkg._args.FrameScratch(lambda W, H: asked.append((W, H)) or 40 * W * H, align=align)
    device = torch.device("cpu")
    assert cache.get(None, 7, 3, device, create=False) is None and cache.cache == {} and asked == [(7, 3)]
    message = f"scratch must be a {wording} tensor of at least 840 bytes on the image's device"
    for bad in (torch.zeros(839, dtype=torch.uint8), torch.zeros(4096, dtype=torch.uint8), torch.zeros(4096)[1:], [0] * 840):
        with pytest.raises(ValueError, match=message):     # too small, on another device (the host), misaligned, no tensor
            cache.get(bad, 7, 3, device)
    assert cache.cache == {}


def test_one_tensor_check(pkg):
    A = pkg._args
    frame = A.frame_check((5, 8), "{} must be a frame")
    for bad in (torch.zeros(4, 6, 5), None, torch.zeros(4, 6, 3), torch.zeros(6, 5)):
        with pytest.raises(ValueError, match="^vpixels must be a frame$"):
            frame(bad, "vpixels")
    with pytest.raises(ValueError, match=r"out must be a contiguous uint8 HIP tensor of shape \(4, 6, 3\) on the image's device"):
        A.check_like(torch.zeros(4, 6, 3), "out", (4, 6, 3), torch.device("cpu"), torch.uint8)
    with pytest.raises(ValueError, match="vgrid must have the grid's shape and device"):
        A.check_same(torch.zeros(12, 2, 3, 4), "vgrid", torch.zeros(12, 2, 3, 5), "grid")


def test_training_loss_refuses_before_any_launch(pkg):
    T = pkg.training_loss
    rgb, target = torch.zeros(33, 55, 3), torch.zeros(3, 33, 55)
    cam = pkg.Camera(55, 33, (60.0, 60.0))
    with pytest.raises(ValueError, match=r"image must be .*\(a :rgbd / :rgbdn frame: :rgb has no alpha row\)"):
        T(None, rgb, target, sky=T.SkyTerm(None, cam))
    with pytest.raises(ValueError, match=r"image must be .*\(H, W, 5\) or \(H, W, 8\) HIP tensor \(a :rgbd / :rgbdn frame\)"):
        T(None, rgb, target, depth=T.DepthTerm(torch.zeros(33, 55), None, 1.0 / 255.0, 2.0))
    with pytest.raises(ValueError, match=r"image must be .*\(H, W, 8\) HIP tensor \(a :rgbdn frame\)"):
        T(None, rgb, target, normal=T.NormalTerm(cam))
    with pytest.raises(ValueError, match="the depth-normal term needs the camera"):
        T(None, torch.zeros(33, 55, 8), target, normal=T.NormalTerm(None, 0.05))
    with pytest.raises(ValueError, match="a bilateral grid needs the view"):
        T(None, rgb, target, bgrid=SimpleNamespace())
    # the heads keep their own first message, and their own special cases
    with pytest.raises(ValueError, match=r"image must be .* with C in \(3, 5, 8\)"):
        pkg.bilateral_grid.l1_ssim_bilateral_loss(None, torch.zeros(33, 55, 4), target, SimpleNamespace(), 0)
    with pytest.raises(ValueError, match=r"\(a :rgbd / :rgbdn frame\)$"):
        pkg.depth_supervision.l1_ssim_depth_loss(None, rgb, target, None, None, 1.0 / 255.0, 10)
    with pytest.raises(ValueError, match="no alpha row"):
        pkg.sky_dome.l1_ssim_sky_loss(None, rgb, target, None, cam)
