"""-m gpu: the HIP forward against the per-pixel float64 definition (tests/definition_ref.py) — the
stages every other parity test holds kernel-against-oracle only: culling, radius and tile rect, duplication, sort order, ranges,
n_contrib, the alpha < 1/255 skip and the T < 1e-4 stop.

Scenes (definition_ref.GPU_SCENES, each filtered by robust_scene; their premises are held in tests/test_definition_cpu.py): one of
each mode, two edge scenes with cutting near / far planes and fx != fy, a single-tile and a ragged image, exact fp32 depth ties,
and lists above the 1024 and the 4096 sort tier.  The definition of a scene is computed once and shared read-only.

  reference lists (exact_tile_cull=False): direct form, aggregating form, forced compact binning (bins_budget_bytes=1), two views
      per handle (the second with fitted bins): radii, rects, tiles_touched, n_rendered, sorted ids and ranges EXACTLY the
      definition's; n_contrib equal on every non-fragile pixel; image and T of the non-fragile pixels within 1e-4 · max(1, fmax)
      but for at most 1e-4 of them (hardware exp), those and the fragile ones within 2 / 255 · fmax — hip_helpers.compare_forward's
      numbers, with the definition in place of the oracle.
  default handle (exact tile cull), both forms: radii, rects and tiles_touched exact; every list an order-preserving subsequence of
      the definition's that holds every entry which surely blends somewhere in its tile; n_contrib names the definition's last
      blended entry; image and T as above.
  forward-only: the same image, T and n_contrib bits as the state-keeping call.
  covisibility / uncertainty on one :rgb scene."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import definition_ref as dr
from hip_helpers import HipRun
from test_definition_cpu import oracle_got
from test_gpu_preprocess_forms import form

pytestmark = pytest.mark.gpu

CELLS = {"direct": (0, 0), "aggregating": (1, 0), "compact": (1, 1)}   # (gsr_preprocess_form, bins_budget_bytes)
OUTLIERS = 1e-4
_oracle = {}


def oracle_figures(pkg, orc, name, side=False):
    """The oracle's own distance from the definition on this scene (no outliers allowed), once per scene."""
    if name not in _oracle:
        defn = dr.definition(pkg, name, side)
        _oracle[name] = dr.check_against_definition(defn, oracle_got(orc, defn.fs)[1], lists="reference", outliers=0.0)
    return _oracle[name]


def hip_run(pkg, defn, exact, budget=0, **kw):
    fs = defn.fs
    arrays = [np.array(a) for a in (fs.means, fs.shs, fs.opac, fs.scales, fs.rots)]   # writable copies: the shared ones are read-only
    return HipRun(pkg, *arrays, fs.cam, fs.deg, fs.bg, fs.mode, exact_tile_cull=exact,
                  bins_budget_bytes=budget, **kw)


def hip_got(run, img):
    r = run.rast
    rect = r.geometry()["rect"].cpu().numpy().astype(np.int64)
    radii = r.radii.cpu().numpy()
    rect[radii <= 0] = 0                                       # records of culled Gaussians are stale, as in the reference
    n = int(r.stats.n_rendered)
    return SimpleNamespace(radii=radii, rect=rect, tiles_touched=(rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]), n_rendered=n,
                           values_sorted=r.values_sorted.cpu().numpy() if n else np.zeros(0, np.int64), ranges=r.ranges.cpu().numpy(),
                           image=img.cpu().numpy(), T=r.accum_alpha.cpu().numpy(), n_contrib=r.n_contrib.cpu().numpy())


def _check_views(pkg, orc, name, cell, exact):
    defn = dr.definition(pkg, name)
    ref = oracle_figures(pkg, orc, name)
    f, budget = CELLS[cell]
    with form(pkg, f):
        run = hip_run(pkg, defn, exact, budget)
        for view in range(2):
            img = run.forward()
            assert int(run.rast.stats.n_visible) == int(defn.d.visible.sum())
            m = dr.check_against_definition(defn, hip_got(run, img), lists="culled" if exact else "reference", outliers=OUTLIERS)
            if budget and defn.tl.n_rendered:
                assert int(run.rast.stats.compact_binning) == 1, "the forced compact mode did not run"
            print(f"{name} ({defn.fs.mode}, {cell}, {'exact cull' if exact else 'reference lists'}, view {view}): worst non-fragile "
                  f"|image - definition| HIP {m['worst_image']:.3g} / oracle {ref['worst_image']:.3g} (fmax {defn.fmax:.3g}), "
                  f"|T - definition| HIP {m['worst_T']:.3g} / oracle {ref['worst_T']:.3g}, outliers {m['outliers']}, "
                  f"fragile pixels {m['fragile']} (worst HIP {m['worst_fragile']:.3g} / oracle {ref['worst_fragile']:.3g}), "
                  f"n_rendered {run.rast.stats.n_rendered} of {defn.tl.n_rendered}")
        run.rast.close()


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("name", dr.GPU_SCENES)
def test_reference_lists_are_the_definitions(pkg, orc, name, cell):
    _check_views(pkg, orc, name, cell, exact=False)


@pytest.mark.parametrize("cell", ["direct", "aggregating"])
@pytest.mark.parametrize("name", dr.GPU_SCENES)
def test_default_handle_culls_only_what_cannot_blend(pkg, orc, name, cell):
    _check_views(pkg, orc, name, cell, exact=True)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", dr.GPU_SCENES)
def test_forward_only_call_gives_the_same_bits(pkg, name, exact):
    defn = dr.definition(pkg, name)
    full, only = hip_run(pkg, defn, exact), hip_run(pkg, defn, exact)
    for _ in range(2):
        a = full.forward().clone()
        b = only.rast.forward_raw(*only.t, only.camera, only.deg, only.bg, only.Rd, only.td, only.covis, only.unc, forward_only=True)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        assert torch.equal(full.rast.accum_alpha, only.rast.accum_alpha) and torch.equal(full.rast.n_contrib, only.rast.n_contrib)
        assert torch.equal(full.rast.radii, only.rast.radii) and torch.equal(full.rast.ranges, only.rast.ranges)
    for r in (full, only):
        r.rast.close()


@pytest.mark.parametrize("exact", [False, True])
def test_covisibility_and_uncertainty(pkg, orc, exact):
    defn = dr.definition(pkg, dr.SIDE_SCENE, side=True)
    dr.conditions(defn)
    assert defn.fs.mode == "rgb" and defn.r.covisibility.any() and not defn.r.covisibility.all()
    run = hip_run(pkg, defn, exact, want_covis=True, want_uncert=True)
    for _ in range(2):
        img = run.forward()
        dr.check_against_definition(defn, hip_got(run, img), lists="culled" if exact else "reference", outliers=OUTLIERS)
        unc, cov = run.unc.cpu().numpy().astype(np.float64), run.covis.cpu().numpy().astype(bool)
        ok = ~defn.r.fragile_pixel
        du = np.abs(unc - defn.r.uncertainty)
        print(f"{dr.SIDE_SCENE}: worst non-fragile |uncertainty - definition| {du[ok].max():.3g}, fragile {du[~ok].max() if (~ok).any() else 0:.3g}; "
              f"covisible {int(defn.r.covisibility.sum())} of {defn.d.n}, {int(defn.r.covis_fragile.sum())} with a T ~ 0.5 pixel")
        assert (du[ok] > 1e-4).sum() <= OUTLIERS * ok.sum() and du.max() <= 2.0 / 255.0
        sure = ~defn.r.covis_fragile
        assert np.array_equal(cov[sure], defn.r.covisibility[sure])
        assert not cov[~defn.d.visible].any()
    run.rast.close()
