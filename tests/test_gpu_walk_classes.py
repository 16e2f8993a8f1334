"""-m gpu: the class boundaries of preprocess's flattened walk against the oracle, on an odd and an even tile grid.

preprocess_kernel sorts a visible Gaussian's tile rect into classes: at most FLAT_MAX = 16 aligned tile pairs -> the flattened
walk over the lanes; more pairs, or more than EMIT_COOP = 48 tiles -> emitted by the whole wave; at most DENSE_RECT = 32 tiles
-> one gradient-row slot per EMITTED tile (the emitted mask in the record), else one per tile of the rect.  The other tests reach
these classes by chance of their scenes.  Here two scenes are first shown to hold every class on both sides of every boundary
(rects from the oracle's means2d / radii, the pair count restated below), then the direct form, the aggregating form and the
forced compact mode (the SCATTER pass) run two views each — the second one with fitted bins — in both list modes:
  reference lists: n_rendered, ranges, sorted ids and per-Gaussian tile counts equal the oracle's, image and gradients meet
                   the parity criteria (the gradients are what check the emitted masks and the slot counts);
  exact cull:      image bit-identical to the reference-list image, every list an order-preserving subsequence of the
                   reference's, gradients meet the oracle criteria;
  every cell and view of a mode is bit-identical to the others in lists, image and gradients.
The form matrix runs at SH degree 0, 1 and 3 (the SH stage sits inside every binning form); the rects do not depend on it.
The banded and 2 x 16-bit instantiations need 1440p / 4K grids: test_gpu_preprocess_forms.py holds them to the direct form."""
import ctypes as C

import numpy as np
import pytest
import torch

from hip_helpers import HipRun, compare_backward, compare_forward
from test_gpu_preprocess_forms import form

pytestmark = pytest.mark.gpu

FLAT_MAX, DENSE_RECT, EMIT_COOP = 16, 32, 48   # csrc/preprocess.hip, gsr_kernels.h
N, DEGREES, SIGMA_PX, BG = 3000, (0, 1, 3), 9.0, (0.1, 0.3, 0.2)
SCENES = {"odd_21x13": (328, 200, 5100), "even_20x12": (320, 192, 5101)}
CELLS = {"direct": (0, 0), "aggregating": (1, 0), "compact": (1, 1)}   # (gsr_preprocess_form, bins_budget_bytes)
_cache = {}


def _oracle(pkg, orc, name, deg):
    """Scene, camera, oracle forward state, pixel cotangent and oracle gradients: computed once per scene and degree, never
    modified."""
    if (name, deg) not in _cache:
        W, H, seed = SCENES[name]
        s = pkg.synthetic.make_scene(N, W, H, deg, seed, sigma_px=SIGMA_PX)
        cam = orc.Camera(W, H, s.focal)
        st = orc.forward(s.means, s.shs, s.opacities, s.scales, s.rotations, cam, deg, background=BG)
        vp = np.random.default_rng(seed).standard_normal((H, W, 3)).astype(np.float32)
        g = orc.backward(st, vp, s.means, s.shs, s.opacities, s.scales, s.rotations, cam, deg, background=BG)
        _cache[name, deg] = (s, cam, st, vp, g)
    return _cache[name, deg]


def _rects(orc, st, grid):
    """(x0, y0, x1, y1) of every visible Gaussian, by the oracle's get_rect."""
    P = lambda a, ct: a.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    g = np.asarray(grid, np.int32)
    rmin, rmax = np.zeros(2, np.int32), np.zeros(2, np.int32)
    out = []
    for i in np.flatnonzero(st.radii > 0):
        px = np.ascontiguousarray(st.means2d[i], np.float32)
        orc.lib().orc_get_rect(P(px, C.c_float), int(st.radii[i]), P(g, C.c_int), P(rmin, C.c_int), P(rmax, C.c_int))
        out.append((int(rmin[0]), int(rmin[1]), int(rmax[0]), int(rmax[1])))
    return out


def _pair_counts(x0, y0, x1, grid_x):
    """Aligned tile pairs (on the linear tile index t = y * grid_x + x) in the rect's even and in its odd rows — the kernel's
    formula: a row starting on an even t holds ceil(w / 2) of them, on an odd t floor(w / 2) + 1."""
    w, t0 = x1 - x0, y0 * grid_x + x0
    t0b = t0 + grid_x
    return ((t0 + w - 1) >> 1) - (t0 >> 1) + 1, ((t0b + w - 1) >> 1) - (t0b >> 1) + 1


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_holds_every_walk_class(pkg, orc, name):
    _, cam, st, _, _ = _oracle(pkg, orc, name, 1)   # (the geometry is drawn before the SH coefficients: the same at every degree)
    grid_x = cam.grid[0]
    classes = dict.fromkeys(["fcnt == 16", "fcnt 17..18, area <= 48", "area == 32", "area 33..36", "area == 48", "area 49..56",
                             "pa != pb, height > 1"], 0)
    for x0, y0, x1, y1 in _rects(orc, st, cam.grid):
        w, h = x1 - x0, y1 - y0
        area = w * h
        if area == 0:
            continue
        pa, pb = _pair_counts(x0, y0, x1, grid_x)
        fcnt = ((h + 1) >> 1) * pa + (h >> 1) * pb
        # brute force over the rect's tiles: the number of distinct aligned pairs it touches
        assert fcnt == len({(y * grid_x + x) >> 1 for y in range(y0, y1) for x in range(x0, x1)})
        classes["fcnt == 16"] += area <= EMIT_COOP and fcnt == FLAT_MAX
        classes["fcnt 17..18, area <= 48"] += area <= EMIT_COOP and fcnt in (FLAT_MAX + 1, FLAT_MAX + 2)
        classes["area == 32"] += area == DENSE_RECT
        classes["area 33..36"] += DENSE_RECT < area <= DENSE_RECT + 4
        classes["area == 48"] += area == EMIT_COOP
        classes["area 49..56"] += EMIT_COOP < area <= EMIT_COOP + 8
        classes["pa != pb, height > 1"] += pa != pb and h > 1
    print(name, classes)
    if grid_x % 2 == 0:
        assert classes.pop("pa != pb, height > 1") == 0   # rows of a rect alternate on grids of odd width only
    assert min(classes.values()) >= 10, classes


def _run_cell(pkg, cam, s, deg, vp, exact, f, budget, check):
    """Two views on one handle under form f; check(run, img) is called per view while the handle lives."""
    out = []
    with form(pkg, f):
        run = HipRun(pkg, s.means, s.shs, s.opacities, s.scales, s.rotations, cam, deg, BG, "rgb", exact_tile_cull=exact,
                     bins_budget_bytes=budget)
        for _ in range(2):
            img = run.forward().clone()
            rec = dict(img=img, T=run.rast.accum_alpha.clone(), ranges=run.rast.ranges.clone(), ids=run.rast.values_sorted.clone(),
                       n_rendered=int(run.rast.stats.n_rendered), compact=int(run.rast.stats.compact_binning))
            check(run, img)
            rec["grads"] = run.backward(vp)
            rec["grads"] = [g.clone() for g in rec["grads"][:5]] + list(rec["grads"][5:])
            out.append(rec)
        run.rast.close()
    return out


def _assert_same_view(a, b):
    assert a["n_rendered"] == b["n_rendered"]
    for k in ("img", "T", "ranges", "ids"):
        assert torch.equal(a[k], b[k]), k
    for ga, gb in zip(a["grads"][:5], b["grads"][:5]):
        assert torch.equal(ga, gb)


@pytest.mark.parametrize("deg", DEGREES)
@pytest.mark.parametrize("name", list(SCENES))
def test_walk_classes_match_the_oracle_in_every_form(pkg, orc, name, deg):
    s, cam, st, vp, g = _oracle(pkg, orc, name, deg)
    vis = st.radii > 0
    views = {}
    for exact in (False, True):
        for cell, (f, budget) in CELLS.items():
            # reference lists: n_rendered, ranges, sorted ids, per-Gaussian tile counts exactly the oracle's; image within parity
            check = (lambda run, img: None) if exact else (lambda run, img: compare_forward(st, run, img, s.opacities))
            views[exact, cell] = _run_cell(pkg, cam, s, deg, vp, exact, f, budget, check)
            assert views[exact, cell][-1]["compact"] == budget, cell   # fitted bins, or the count -> scan -> SCATTER passes
        first = views[exact, "direct"][0]
        for cell in CELLS:
            for v in views[exact, cell]:
                _assert_same_view(first, v)
        compare_backward(g, first["grads"], vis)
    ref, cul = views[False, "direct"][0], views[True, "direct"][0]
    assert ref["n_rendered"] == st.n_rendered and cul["n_rendered"] < ref["n_rendered"]
    assert torch.equal(ref["img"], cul["img"]) and torch.equal(ref["T"], cul["T"])
    rr, rc = ref["ranges"].cpu().numpy(), cul["ranges"].cpu().numpy()
    vr, vc = ref["ids"].cpu().numpy(), cul["ids"].cpu().numpy()
    for t in range(rr.shape[0]):
        a, b = vr[rr[t, 0]:rr[t, 1]], vc[rc[t, 0]:rc[t, 1]]
        assert np.array_equal(a[np.isin(a, b)], b), "culled list must be an order-preserving subsequence"
