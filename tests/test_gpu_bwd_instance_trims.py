"""-m gpu: the per-instance work of the one-wave backward, composite_bwd_kernel (composite.hip).

A lane owns rows y, y + 4, y + 8, y + 12 of its column: pixel group q is rows 4q .. 4q + 3 of the tile, and an instance visits
the groups its footprint mask names — four wave-uniform tests read next to the mask, before the first group is walked.

a. instances whose first visited group is not group 0: splats whose alpha >= 1/255 footprint stays inside rows 4-7, 8-11 or
   12-15, alone, together, and mixed with splats of rows 0-3 and broad ones — each gradient within the suite's 1e-4 relative L2
   of the oracle, the banded splats' rows also by themselves.
b. instances no lane blends (opacity below 1/255; a footprint that falls between the pixel centres) keep exact zero rows, on
   buffers poisoned with GSR_DEBUG_FILL=nan.
(A build whose test of group q reads the bits of group q ^ 1 fails all twelve cases: profiles/bwd_instance_trims/bench_ab.txt.)

The scenes are built in the 16 x 16 tile of tests/list_scenes.py and seen through a 40 x 24 camera with the same principal
point in pixels: rows 12-15 spill into a tile whose rows 24 .. 31 lie outside the image."""
import contextlib
import os

import numpy as np
import pytest

import list_scenes as ls
from hip_helpers import HipRun, compare_backward, rel_l2
from oracle.oracle import Camera

pytestmark = pytest.mark.gpu

W, H = 40, 24
BG = (0.3, 0.1, 0.6)


def wide(sc, cx=8.0):
    """The scene of a 16 x 16 (32 x 16: cx = 16) builder behind a 40 x 24 camera with the same focal length and principal point IN
    PIXELS: every projected centre keeps its pixel coordinates."""
    sc.cam = Camera(W, H, sc.cam.focal, principal=(cx / W, 8.0 / H))
    return sc


@contextlib.contextmanager
def env(name, value):
    old = os.environ.pop(name, None)
    if value is not None:
        os.environ[name] = value
    try:
        yield
    finally:
        os.environ.pop(name, None)
        if old is not None:
            os.environ[name] = old


# ---- a. the first visited pixel group is not group 0 ----
def band_scene(bands, broad, seed, deg=1):
    """Per band (q: rows 4q .. 4q + 3) 40 faint splats centred on rows 4q + 1.9 .. 4q + 2.1 and `broad` splats of 5 px on top.
    A banded splat has sigma 0.88 .. 0.95 px (with the 0.3 px^2 blur at most 1.10 px: radius 4, above the radius clip of 3)
    and opacity 0.010 .. 0.016: alpha reaches 1/255 within 1.10 * sqrt(2 ln(255 * 0.016)) = 1.84 px of its centre."""
    rng = np.random.default_rng([int(seed)] + list(bands))
    cam = ls._camera()
    fx = float(cam.focal[0])
    n = 40 * len(bands) + broad
    depths = ls._unique_depths(rng, n)
    slot = rng.permutation(n)
    K = (deg + 1) ** 2
    parts = [np.zeros((n, 3)), np.zeros((n, K, 3)), np.zeros(n), np.zeros((n, 3)), np.zeros((n, 4))]
    band_of = np.full(n, -1)
    for i, q in enumerate(bands):
        idx = slot[40 * i:40 * i + 40]
        z = depths[idx]
        u, v = rng.uniform(2.0, 13.0, 40), rng.uniform(4 * q + 1.9, 4 * q + 2.1, 40)
        parts[0][idx] = np.stack([(u - 8.0) * z / fx, (v - 8.0) * z / fx, z], 1)
        parts[1][idx, 0] = rng.normal(0.0, 0.5, (40, 3))
        parts[1][idx, 1:] = rng.normal(0.0, 0.1, (40, K - 1, 3))
        parts[2][idx] = rng.uniform(0.010, 0.016, 40)
        parts[3][idx] = (0.95 * z / fx)[:, None] * rng.permuted(np.tile([1.0, 0.93, 0.97], (40, 1)), axis=1)
        parts[4][idx] = rng.standard_normal((40, 4))
        band_of[idx] = q
    idx = slot[40 * len(bands):]
    fr = ls._front(rng, broad, depths[idx], 5.0, 0.3, fx, np.zeros(broad, bool), deg)
    for k in range(5):
        parts[k][idx] = fr[k]
    sc = wide(ls._pack(parts, np.arange(n, dtype=np.int64), cam, deg))
    sc.band_of = band_of
    return sc


def blended_rows(st, opac, i):
    """Rows of the pixels of tile (0, 0) at which Gaussian i reaches alpha >= 1/255 (float64 on the oracle's projection)."""
    ys, xs = np.mgrid[0:16, 0:16].astype(np.float64)
    (mx, my), (a, b, c) = st.means2d[i].astype(np.float64), st.conics[i].astype(np.float64)
    dx, dy = mx - xs, my - ys
    alpha = float(opac[i]) * np.exp(-(0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy))
    return np.unique(ys[alpha >= 1.0 / 255.0].astype(np.int64))


@pytest.mark.parametrize("mode", ["rgb", "rgbdn"])
@pytest.mark.parametrize("bands,broad", [((1,), 0), ((2,), 0), ((3,), 0), ((1, 2, 3), 0), ((0, 1, 2, 3), 6)],
                         ids=["rows4-7", "rows8-11", "rows12-15", "three-bands", "mixed"])
def test_first_visited_group_is_not_group_0(pkg, orc, bands, broad, mode):
    sc = band_scene(bands, broad, 23)
    st = orc.forward(*sc.args, sc.cam, sc.deg, background=BG, mode=mode)
    blending = 0
    for i in np.flatnonzero(sc.band_of >= 0):
        rows = blended_rows(st, sc.opac, i)
        assert ((rows // 4) == sc.band_of[i]).all(), (i, rows)
        blending += rows.size > 0
    assert blending >= 30 * len(bands), "the banded splats blend somewhere"
    vp = np.random.default_rng(29).standard_normal(st.image.shape).astype(np.float32)
    g = orc.backward(st, vp, *sc.args, sc.cam, sc.deg, background=BG)
    run = HipRun(pkg, *sc.args, sc.cam, sc.deg, BG, mode)
    run.forward()
    assert np.array_equal(run.rast.values_sorted.cpu().numpy().astype(np.uint32), st.values_sorted)
    out = run.backward(vp)
    compare_backward(g, out, st.radii > 0)
    assert rel_l2(run.rast.grad_means_2d.cpu().numpy(), g.vmeans2d) <= 1e-4
    ids = np.flatnonzero(sc.band_of > 0)          # ... and the rows of the banded splats by themselves
    if ids.size:
        for a, b in zip([o.cpu().numpy() for o in out[:5]], (g.vmeans, g.vshs, g.vopacities, g.vscales, g.vrots)):
            assert rel_l2(a.reshape(len(sc.opac), -1)[ids], np.asarray(b).reshape(len(sc.opac), -1)[ids]) <= 1e-4


# ---- b. instances no lane blends ----
def ghost_scene(L, seed):
    """single_tile_scene(L) with four of its front splats turned into ghosts that stay in the list (reference lists: the 3-sigma
    square) and blend nowhere: two of sigma 3 px and opacity 0.003 < 1/255, and two of sigma 0.9 px (1.05 px with the blur:
    radius 4, above the radius clip) and opacity 0.0043 centred between four pixel centres — alpha >= 1/255 within
    1.05 * sqrt(2 ln(255 * 0.0043)) = 0.45 px, the nearest pixel centre is 0.71 px away."""
    sc = ls.single_tile_scene(L, seed)
    fx = float(sc.cam.focal[0])
    ghosts = sc.order[[L // 4, L // 2, L // 2 + 9, L - 3]]
    for k, i in enumerate(ghosts):
        z = float(sc.means[i, 2])
        if k % 2 == 0:
            sc.opac[i] = 0.003
            sc.scales[i] = 3.0 * z / fx
        else:
            sc.opac[i] = 0.0043
            sc.scales[i] = 0.9 * z / fx
            sc.means[i, :2] = np.float32((5.5 + k - 8.0) * z / fx), np.float32((6.5 - 8.0) * z / fx)
    return wide(sc), ghosts


@pytest.mark.parametrize("mode", ["rgb", "rgbd"])
def test_instances_no_lane_touches_keep_exact_zero_rows(pkg, orc, mode):
    L = 129
    sc, ghosts = ghost_scene(L, 31)
    st = orc.forward(*sc.args, sc.cam, sc.deg, background=BG, mode=mode)
    assert (st.radii[ghosts] > 0).all() and (st.tiles_touched[ghosts] > 0).all(), "the ghosts are listed"
    for i in ghosts:
        assert blended_rows(st, sc.opac, i).size == 0
    vp = np.random.default_rng(37).standard_normal(st.image.shape).astype(np.float32)
    g = orc.backward(st, vp, *sc.args, sc.cam, sc.deg, background=BG)
    with env("GSR_DEBUG_FILL", "nan"):
        run = HipRun(pkg, *sc.args, sc.cam, sc.deg, BG, mode)
        run.forward()
        assert run.rast.stats.n_rendered == st.n_rendered
        out = run.backward(vp)
    compare_backward(g, out, st.radii > 0)
    for o in list(out[:5]) + [run.rast.grad_means_2d]:
        o = o.cpu().numpy().reshape(len(sc.opac), -1)
        assert np.isfinite(o).all()
        assert not o[ghosts].any(), "a ghost's gradient rows are exact zeros"
