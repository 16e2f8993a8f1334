"""-m gpu: the footprint masks the library writes (rast.instance_masks; csrc/tile_mask.h instance_row_mask) against the kernels'
own blend test, bits(sigma) < X, on the 256 pixel centres of every instance's tile.

sigma is restated in numpy fp32 in the kernels' operation order (tests/footprint_ref.py kernel_sigma) on the library's own
projection (means2d, conics) and X is read from the library's geometry record, so the test holds whatever the opacity
activation and the threshold search did.  Every pixel that passes must lie in a flagged row AND a flagged quadrant
(bit 16 + 2 qy + qx), in both list modes (reference lists: the 3-sigma square; exact tile cull: the default).

  a. 160 x 96, 2 500 strongly anisotropic splats (the scene of test_gpu_parity.py test_footprint_masks_are_conservative);
     also tight: flagged rows <= 1.25 x active rows + 16; at least 3 000 instances checked;
  b. 96 x 64, 300 needles: axis ratio >= 50 : 1 after the 0.3 px^2 blur, long axis (6 sigma) >= 180 px; 130 at 0, 100 at 45 and
     30 at 90 degrees in the image plane (up to the perspective skew), 40 at any angle;
  c. 96 x 64, 300 splats with opacity 1/255 + 1e-4, 1/255 - 1e-4 and 0.9 / 255 (and ordinary ones between them);
  d. 64 x 48, 40 splats: 3-sigma radius > 200 px, and splats centred up to 3 sigma outside the image;
  e. the :rgbd stream (X travels in the fourth plane there) on scene c.

On every scene at least a quarter of the checked instances — those of both list modes together — have between 1 and 15 rows
flagged, and each run has some: a mask of all ones cannot pass.  (Counted per list mode the needles cannot reach a quarter: the
reference's list of a needle is the 3-sigma square of its long axis, all 24 tiles of the image, of which a line crosses six to nine.)
(A build whose threshold ts is lowered by 0.05 fails: profiles/fwd_footprint_masks/bench_ab.txt.)"""
import math

import numpy as np
import pytest

import footprint_ref as fr
from hip_helpers import HipRun

pytestmark = pytest.mark.gpu


def _shs(rng, n):
    return rng.normal(0.0, 0.5, (n, 1, 3)).astype(np.float32)


def _planar(rng, W, H, u, v, major_px, minor_px, theta, opac):
    """Splats facing the camera: projected centre (u, v) px, image-plane axes major_px / minor_px (standard deviations, before the
    blur) with the major axis at angle theta.  Returns the activated inputs and the focal length."""
    n = len(u)
    fx = 0.5 * W / math.tan(math.radians(30.0))
    z = rng.uniform(2.0, 12.0, n)
    means = np.stack([(u - 0.5 * W) * z / fx, (v - 0.5 * H) * z / fx, z], 1).astype(np.float32)
    scales = np.stack([major_px * z / fx, minor_px * z / fx, 0.5 * minor_px * z / fx], 1).astype(np.float32)
    rots = np.stack([np.cos(0.5 * theta), np.zeros(n), np.zeros(n), np.sin(0.5 * theta)], 1).astype(np.float32)
    return means, _shs(rng, n), np.asarray(opac, np.float32), scales, rots, (np.float32(fx), np.float32(fx))


def scene_anisotropic(pkg):
    W, H, n = 160, 96, 2500
    s = pkg.synthetic.make_scene(n, W, H, 0, 29, sigma_px=5.0)
    rng = np.random.default_rng(29)
    scales = (s.scales * np.exp(rng.normal(0, 0.8, (n, 3)))).astype(np.float32)
    return (s.means, s.shs, s.opacities, scales, s.rotations), (W, H, s.focal)


def scene_needles(pkg):
    W, H, n = 96, 64, 300
    rng = np.random.default_rng(31)
    theta = rng.uniform(0.0, math.pi, n)
    theta[:130], theta[130:230], theta[230:260] = 0.0, 0.25 * math.pi, 0.5 * math.pi
    major = rng.uniform(30.0, 60.0, n)
    minor = rng.uniform(0.05, 0.3, n)       # + the 0.3 px^2 blur: 0.55 .. 0.63 px, ratio 50 : 1 and more
    u, v = rng.uniform(-8.0, W + 8.0, n), rng.uniform(-8.0, H + 8.0, n)
    opac = rng.uniform(0.01, 0.9, n)
    m, shs, o, sc, ro, focal = _planar(rng, W, H, u, v, major, minor, theta, opac)
    return (m, shs, o, sc, ro), (W, H, focal)


def scene_threshold_opacities(pkg):
    W, H, n = 96, 64, 300
    rng = np.random.default_rng(37)
    sig = rng.uniform(1.0, 3.0, n)
    u, v = rng.uniform(0.0, W, n), rng.uniform(0.0, H, n)
    opac = rng.uniform(0.006, 0.9, n)
    amin = 1.0 / 255.0
    opac[0:40], opac[40:80], opac[80:100] = amin + 1e-4, amin - 1e-4, 0.9 * amin
    m, shs, o, sc, ro, focal = _planar(rng, W, H, u, v, sig * rng.uniform(1.0, 2.0, n), sig, rng.uniform(0.0, math.pi, n), opac)
    return (m, shs, o, sc, ro), (W, H, focal)


def scene_large_and_outside(pkg):
    W, H, n = 64, 48, 40
    rng = np.random.default_rng(41)
    big = 12
    major = np.concatenate([rng.uniform(70.0, 120.0, big), rng.uniform(4.0, 14.0, n - big)])     # 3 sigma > 200 px
    minor = np.concatenate([rng.uniform(2.0, 6.0, big), rng.uniform(2.0, 6.0, n - big)])
    theta = rng.uniform(0.0, math.pi, n)
    theta[:big] = rng.uniform(-0.3, 0.3, big)
    u, v = rng.uniform(0.0, W, n), rng.uniform(0.0, H, n)
    # centred outside the image, by up to 3 sigma of the axis that points back at it (the minor one at least)
    side = rng.integers(0, 4, n - big)
    off = rng.uniform(0.2, 3.0, n - big) * minor[big:]
    u[big:] = np.where(side == 0, -off, np.where(side == 1, W - 1 + off, u[big:]))
    v[big:] = np.where(side == 2, -off, np.where(side == 3, H - 1 + off, v[big:]))
    opac = rng.uniform(0.02, 0.9, n)
    m, shs, o, sc, ro, focal = _planar(rng, W, H, u, v, major, minor, theta, opac)
    return (m, shs, o, sc, ro), (W, H, focal)


SCENES = {"anisotropic": scene_anisotropic, "needles": scene_needles, "threshold-opacities": scene_threshold_opacities,
          "large-and-outside": scene_large_and_outside}


def instance_table(means2d, conics, X_of, ids, ranges, W):
    """Per sorted instance: float32 mx, my, a, b, c, uint32 X and the int64 origin of its tile."""
    gx = (W + 15) // 16
    n_inst = ranges[:, 1] - ranges[:, 0]
    tile = np.repeat(np.arange(ranges.shape[0]), np.maximum(n_inst, 0))
    pos = np.concatenate([np.arange(a, b) for a, b in ranges if b > a]) if len(tile) else np.zeros(0, np.int64)
    g = ids[pos]
    return pos, (means2d[g, 0], means2d[g, 1], conics[g, 0], conics[g, 1], conics[g, 2], X_of[g],
                 ((tile % gx) * 16).astype(np.int64), ((tile // gx) * 16).astype(np.int64))


def check_run(pkg, run, W):
    """Checks the masks of one forward against the blend test; returns (instances, instances with 1 .. 15 rows flagged,
    active rows, flagged rows)."""
    import torch
    masks = run.rast.instance_masks.cpu().numpy().astype(np.int64) & 0xFFFFF
    ids = run.rast.values_sorted.cpu().numpy().astype(np.int64)
    ranges = run.rast.ranges.cpu().numpy().reshape(-1, 2).astype(np.int64)
    rec = run.rast._buffer(pkg._lib.BUF_GEOM, torch.float32, (run.t[0].shape[0], 16)).cpu().numpy()
    X_of = np.ascontiguousarray(rec[:, 14]).view(np.uint32)       # q3.z: the blend-test threshold bits of the Gaussian
    pos, inst = instance_table(np.ascontiguousarray(rec[:, 0:2]), np.ascontiguousarray(rec[:, 2:5]), X_of, ids, ranges, W)
    assert len(pos) == len(masks) == len(ids)
    act = fr.active_pixels(*inst)
    miss_rows, miss_quads, act_rows, flag_rows, act_quads, flag_quads = fr.check_masks(masks[pos], act)
    nrows = np.array([bin(int(m) & 0xFFFF).count("1") for m in masks[pos]])
    partial = int(((nrows >= 1) & (nrows <= 15)).sum())
    print(f"instances {len(pos)}, partly flagged {partial}, rows active {act_rows} flagged {flag_rows}, quadrants active {act_quads} "
          f"flagged {flag_quads}, missed rows {miss_rows} quadrants {miss_quads}")
    assert miss_rows == 0, "an active pixel lies in a row that is not flagged"
    assert miss_quads == 0, "an active pixel lies in a quadrant that is not flagged"
    return len(pos), partial, act_rows, flag_rows


@pytest.mark.parametrize("name", list(SCENES))
def test_masks_cover_every_pixel_that_passes_the_blend_test(pkg, orc, name):
    args, (W, H, focal) = SCENES[name](pkg)
    checked = partial = 0
    for exact in (False, True):  # reference lists (the 3-sigma square: most instances of a needle reach no pixel), exact tile cull
        run = HipRun(pkg, *args, orc.Camera(W, H, focal), 0, exact_tile_cull=exact)
        run.forward()
        n, part, act_rows, flag_rows = check_run(pkg, run, W)
        assert part > 0
        if name == "anisotropic":
            assert n >= 3000
            assert flag_rows <= 1.25 * act_rows + 16
        checked += n; partial += part
    assert 4 * partial >= checked, "a quarter of the scene's instances have 1 .. 15 rows flagged"


def test_masks_in_rgbd_mode(pkg, orc):
    args, (W, H, focal) = scene_threshold_opacities(pkg)
    run = HipRun(pkg, *args, orc.Camera(W, H, focal), 0, mode="rgbd")
    run.forward()
    n, part, _, _ = check_run(pkg, run, W)
    assert n >= 100 and 4 * part >= n
