"""-m gpu: keys of one tile that share their DEPTH BITS.

The reference sorts 64-bit (tile, depth bits) keys with a stable sort over values that arrive by ascending Gaussian id, so equal
depths keep the id order; the library sorts (depth bits, id) words per tile, and the rule holds only as long as the low word takes
part in every compare: wave_bitonic_sort, the merge-path searches and take_a rules of sort_runs_lds and big_merge_kernel, and the
fused forward's own sort (tile_sort_device.h, binning.hip, composite.hip).  tests/list_scenes.py tied_tile_scene draws the front's
depths from 1 or 5 levels — the whole front ONE tie, or five long ones — at the list lengths on which those sorts change path; its
premises are held on the oracle alone by tests/test_list_scenes_cpu.py.  Criteria: those of tests/test_gpu_list_boundaries.py,
unchanged — compare_forward (ids and ranges exact), n_contrib at every pixel, compare_backward and the boundary-row check at 1e-4."""
import numpy as np
import pytest
import torch

import list_scenes as ls
import test_gpu_list_boundaries as lb
from hip_helpers import HipRun, compare_backward, compare_forward
from test_gpu_preprocess_forms import form

pytestmark = pytest.mark.gpu

BG = lb.BG


def tied(orc, L, groups, mode="rgb"):
    return lb.reference_for(orc, ("tied", L, groups, mode), lambda: ls.tied_tile_scene(L, groups, 17), 2000 + L, mode, BG)


def pair(ref, run, L, family):
    lb.check_forward(ref, run, L)
    return lb.check_backward(ref, run, L, family=family)


# ---- 1. one tile: the separate sort (first view of a handle), then the fused kernel's (second view, lists of up to 1024) ----
@pytest.mark.parametrize("groups", ls.TIED_GROUPS)
@pytest.mark.parametrize("L", ls.TIED_LENGTHS)
def test_tied_depths_keep_the_id_order(pkg, orc, L, groups):
    ref = tied(orc, L, groups)
    assert ref.sc.ties == max(0, L - 1 - groups) or L - 1 < 20 * groups
    if groups == 1:
        assert np.array_equal(ref.st.values_sorted, np.arange(L))   # one tie: ascending ids
    lb.check_two_views(ref, lb.hip_run(pkg, ref), L, f"ties, {groups} level(s)")


@pytest.mark.parametrize("groups", ls.TIED_GROUPS)
@pytest.mark.parametrize("L", ls.TIED_MODE_LENGTHS)
def test_tied_depths_in_the_normal_mode(pkg, orc, L, groups):
    ref = tied(orc, L, groups, "rgbdn")
    lb.check_two_views(ref, lb.hip_run(pkg, ref, "rgbdn"), L, "ties :rgbdn")


# ---- 2. the other ways a key reaches its list ----
@pytest.mark.parametrize("L", ls.TIED_MODE_LENGTHS)
def test_exact_cull_handle_keeps_the_id_order(pkg, orc, L):
    """The culled list is a sub-list of the tie: the same image and transmittance bit for bit, the same gradients."""
    ref = tied(orc, L, 1)
    lists, cull = lb.hip_run(pkg, ref), lb.hip_run(pkg, ref, exact_tile_cull=True)
    for _ in range(2):
        a, b = lists.forward().clone(), cull.forward().clone()
        assert torch.equal(a, b) and torch.equal(lists.rast.accum_alpha, cull.rast.accum_alpha)
        assert 0 < cull.rast.stats.n_rendered <= lists.rast.stats.n_rendered == L
        ids = cull.rast.values_sorted.cpu().numpy()
        assert (np.diff(ids.astype(np.int64)) > 0).all(), "one tie: the culled list ascends by id as well"
        out = cull.backward(ref.vp)
        compare_backward(ref.g, out, ref.st.radii > 0)
        lb.boundary_rows(ref, out, L, family="ties, exact cull")


@pytest.mark.parametrize("L", ls.TIED_MODE_LENGTHS)
def test_forced_compact_binning(pkg, orc, L):
    """bins_budget_bytes = 1: count -> scan -> scatter, no bins; the keys arrive in the scatter's order."""
    ref = tied(orc, L, 1)
    run = lb.hip_run(pkg, ref, bins_budget_bytes=1)
    for _ in range(2):
        pair(ref, run, L, "ties, compact")
        assert run.rast.stats.compact_binning == 1


@pytest.mark.parametrize("L,L1", sorted(ls.TIED_BIN_FIRST_VIEWS.items()))
def test_bins_too_small_for_the_tie(pkg, orc, L, L1):
    """The three-view walk of test_gpu_list_boundaries._bins_walk with the tied list as its third view: two views of L1 distinct
    depths settle the bins' capacity (equal to gsr_bins_capacity_after), the tied list is longer than that and leaves the capacity
    as it is.  Bins of fewer than 1024 keys finish the view compactly (compact_binning 1), larger ones scatter the overflowing list
    a second time (2); the view after it has bins that hold the list."""
    cap = lb._bins_walk(pkg, orc, L1, "full", None, third=(tied(orc, L, 1), L, "ties, overflow"))
    assert (cap >= 1024) == (L > 1024)


def _record(run, out):
    r = run.rast
    return [t.clone() for t in (r.accum_alpha, r.n_contrib, r.values_sorted, r.ranges, r.grad_means_2d)] + [o.clone() for o in out[:5]]


@pytest.mark.parametrize("L", ls.TIED_MODE_LENGTHS)
def test_aggregating_form_changes_the_arrival_order_only(pkg, orc, L):
    """gsr_preprocess_form(1): a workgroup hands out its bin positions in address order, so the unsorted keys of a bin arrive in
    another order than under form 0.  A sort that left equal depths in arrival order would show it; every output must be
    bit-identical."""
    ref = tied(orc, L, 1)
    recs = {}
    for f in (0, 1):
        with form(pkg, f):
            run = lb.hip_run(pkg, ref)
            recs[f] = []
            for _ in range(2):
                img = lb.check_forward(ref, run, L).clone()
                out = lb.check_backward(ref, run, L, family=f"ties, form {f}")
                recs[f].append([img] + _record(run, out))
            run.rast.close()
    for va, vb in zip(recs[0], recs[1]):
        for k, (a, b) in enumerate(zip(va, vb)):
            assert torch.equal(a, b), k


# ---- 3. Gaussians of several tiles each, tied inside many tiles ----
def tied_cloud(pkg, n, W, H, levels, seed, deg=1):
    """pkg.synthetic.make_scene with the depths rounded to `levels` values (identity pose: the depth bits are those of z)."""
    s = pkg.synthetic.make_scene(n, W, H, deg, seed, sigma_px=3.0)
    k = np.clip(np.floor((s.means[:, 2].astype(np.float64) - 2.0) / 10.0 * levels), 0, levels - 1)
    s.means[:, 2] = (2.0 + 10.0 * (k + 0.5) / levels).astype(np.float32)
    return s


def test_tied_cloud_across_tiles(pkg, orc):
    W, H, deg = 96, 64, 1
    s = tied_cloud(pkg, 3000, W, H, 8, 6100, deg)
    cam = orc.Camera(W, H, s.focal)
    args = (s.means, s.shs, s.opacities, s.scales, s.rotations)
    st = orc.forward(*args, cam, deg, background=BG)
    # premises, on the oracle, before any HIP call
    assert np.unique(s.means[:, 2]).size == 8
    assert np.array_equal(st.depths[st.radii > 0].view(np.uint32), s.means[st.radii > 0, 2].view(np.uint32))
    same = st.keys_sorted[1:] == st.keys_sorted[:-1]
    in_pair = np.zeros(st.n_rendered, bool)
    in_pair[1:] |= same
    in_pair[:-1] |= same
    assert in_pair.mean() >= 0.1, in_pair.mean()
    assert (np.diff(st.values_sorted.astype(np.int64))[same] > 0).all(), "the reference keeps equal keys in id order"
    per_gauss = np.bincount(st.values_sorted, minlength=s.n)               # instances of a Gaussian ...
    tied_per_gauss = np.bincount(st.values_sorted[in_pair], minlength=s.n)   # ... and those of them that sit in a tied pair
    assert ((per_gauss >= 2) & (tied_per_gauss == per_gauss)).any(), "a Gaussian of several tiles, tied in each of them"
    assert np.array_equal(per_gauss, st.tiles_touched * (st.radii > 0))
    vp = np.random.default_rng(6101).standard_normal(st.image.shape).astype(np.float32)
    g = orc.backward(st, vp, *args, cam, deg, background=BG)
    run = HipRun(pkg, *args, cam, deg, BG)
    for _ in range(2):
        compare_forward(st, run, run.forward(), s.opacities)
        compare_backward(g, run.backward(vp), st.radii > 0)
