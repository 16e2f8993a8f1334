"""-m gpu: views with MORE THAN 256 tier tiles — where gsr_policy_bwd_split moves the backward's cut.

While at most bwd_split_max_tiles = 256 tiles have a list beyond 1024 entries, all of them leave the one-wave backward for
composite_bwd_long_kernel (split_len 1024).  Beyond that the cut moves to 4096, to 8192, or nothing is split, and then
  * the default composite_bwd_kernel<.., ACC = false> walks lists of up to 4096, up to 8192 or of any length;
  * composite_bwd_long_kernel reads a PARTIAL GsrTierLists (n_mid4 = 0, or n_mid4 = n_mid8 = 0): the list offsets;
  * the forward sorts hundreds of listed tiles (tile_sort_runs_kernel), its speculative mid-tier grid is capped at "every tile"
    (gsr_policy_begin_view: 256 + 64 + 16 > 280) and long_state holds 256 tiles.
tests/list_scenes.py many_tile_scene gives every tile of a 20 x 14 grid a list of a chosen length (premises: the oracle alone,
tests/test_list_scenes_cpu.py); ls.MANY_TILE_CASES are the tier counts and the split each must produce.  Per case: two views on
one handle, then the NEIGHBOURING case on the same handle, which must equal that case's views on a fresh handle bit for
bit; the whole sequence again on buffers filled with NaN, bit-identical.  Every view: compare_forward, n_contrib at every pixel,
tier_tiles, the split, compare_backward, and the boundary-row check (1e-4) per tile CLASS — the pinned rows of the mid4, mid8,
big, 1024-entry and 10-entry tiles each by themselves; the 10-entry tiles' rows are 10 to 100 times larger than the others."""
import ctypes as C

import numpy as np
import pytest
import torch

import list_scenes as ls
import test_gpu_list_boundaries as lb
from hip_helpers import compare_backward, compare_forward, rel_l2
from test_gpu_poisoned_buffers import debug_fill

pytestmark = pytest.mark.gpu

BG = lb.BG
GX, GY = ls.MANY_GRID
CASES = list(ls.MANY_TILE_CASES)
NEIGHBOUR = {c: CASES[(i + 1) % len(CASES)] for i, c in enumerate(CASES)}
CLASS_LENGTH = {"mid4": 4096, "mid8": 8192, "big": 8193, "1024": 1024, "ten": 10}   # (names the boundary-row check's table row)
_clean = {}


def many(orc, case, mode="rgb", bg=BG):
    lengths, cls = ls.many_tile_lengths(case)
    ref = lb.reference_for(orc, ("many", case, mode, bg), lambda: ls.many_tile_scene(GX, GY, lengths, 23), 3000 + sum(case),
                           mode, bg, deterministic="parallel")   # (every Gaussian is in ONE tile: no sum crosses tiles)
    return ref, lengths, cls


def view(pkg, orc, run, case, mode, bg, check, family):
    """One forward + backward of `case` on `run`; returns every output, cloned."""
    ref, lengths, cls = many(orc, case, mode, bg)
    img = run.forward()
    s = run.rast.stats
    if check:
        compare_forward(ref.st, run, img, ref.sc.opac)
        nc = run.rast.n_contrib.cpu().numpy().astype(np.uint32)
        assert np.array_equal(nc, ref.st.n_contrib), "n_contrib must equal the oracle's at every pixel"
        assert s.n_rendered == lengths.sum() and s.max_tile_instances == lengths.max()
        assert tuple(s.tier_tiles) == case
        # the split launch_composite_bwd will obtain: the policy function it calls, on this view's tier counts
        L = pkg._lib
        cfg, sp = L.PolicyConfig(), L.BwdSplit()
        L.load().gsr_policy_config_init(C.byref(cfg), 16 * GX, 16 * GY, 0, -1)
        L.load().gsr_policy_bwd_split(C.byref(cfg), *s.tier_tiles, C.byref(sp))
        assert (sp.n_mid4, sp.n_mid8, sp.n_big, sp.split_len) == ls.MANY_TILE_CASES[case]
    rec = [img.clone(), run.rast.accum_alpha.clone(), run.rast.n_contrib.clone(), run.rast.values_sorted.clone(),
           run.rast.ranges.clone()]
    out = run.backward(ref.vp)
    rec += [run.rast.grad_means_2d.clone()] + [o.clone() for o in out[:5]]
    if check:
        compare_backward(ref.g, out, ref.st.radii > 0)
        assert rel_l2(rec[5].cpu().numpy(), ref.g.vmeans2d) <= 1e-4
        host = [o.cpu() for o in out[:5]]
        for c in ls.MANY_CLASSES:
            if cls[c].size:
                lb.boundary_rows(ref, host, CLASS_LENGTH[c], family=f"{family}, {c} tiles", ids=ls.tile_rows(ref.sc, cls[c]))
    return rec


def run_case(pkg, orc, case, mode="rgb", bg=BG, fill=None, neighbour=True):
    """Two views of `case` on a fresh handle, then its neighbour on the same handle.  fill = None: every view is checked against
    the oracle; "nan": the handle's float buffers start as NaN and the caller compares the records with the clean run's."""
    check = fill is None
    family = "tier routing" if mode == "rgb" else f"tier routing :{mode} bg0"
    with debug_fill(fill):
        ref, _, _ = many(orc, case, mode, bg)
        run = lb.hip_run(pkg, ref, mode, bg)
        recs = [view(pkg, orc, run, case, mode, bg, check, family) for _ in range(2)]
        s = run.rast.stats
        # (the first view's bins are an estimate — 7 616 keys per bin, which an 8 193-entry list overflows; the second view's hold every list)
        assert s.compact_binning == 0 and s.bin_capacity >= max(ref.sc.lengths), (s.compact_binning, s.bin_capacity)
        held = int(s.held_views)
        assert held >= 1, "the second view had tier tiles before it: its fused launch is held for their sorts"
        if neighbour:
            lb.show(many(orc, NEIGHBOUR[case], mode, bg)[0], run)
            recs.append(view(pkg, orc, run, NEIGHBOUR[case], mode, bg, check, family))
            assert int(run.rast.stats.held_views) > held
        run.rast.close()
    return recs


def clean(pkg, orc, case):
    if case not in _clean:
        _clean[case] = run_case(pkg, orc, case)
    return _clean[case]


def same(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), f"output {k} differs"


@pytest.mark.parametrize("case", CASES, ids=str)
def test_tier_counts_around_the_split_limit(pkg, orc, case):
    recs = clean(pkg, orc, case)
    fresh = clean(pkg, orc, NEIGHBOUR[case])
    # the neighbouring case as this handle's third view == the same case on a fresh handle: its second view (the held fused
    # launch beside the tier walk) and its first (separate sort, strip forward over every tile), which give the same bits
    same(recs[2], fresh[1])
    same(recs[2], fresh[0])


@pytest.mark.parametrize("case", CASES, ids=str)
def test_tier_counts_on_nan_filled_buffers(pkg, orc, case):
    """GSR_DEBUG_FILL=nan: a row, pixel or segment state that no kernel wrote is a NaN, not a zero."""
    for a, b in zip(clean(pkg, orc, case), run_case(pkg, orc, case, fill="nan")):
        same(a, b)
        assert not any(torch.isnan(t).any() for t in b if t.is_floating_point())


@pytest.mark.parametrize("case", [(257, 0, 0), (250, 6, 1)], ids=str)
def test_depth_mode_with_a_zero_background(pkg, orc, case):
    """:rgbd, background 0: the BG0 instantiations of the main kernel (lists beyond 1024 in it) and of the long kernel."""
    run_case(pkg, orc, case, "rgbd", (0.0, 0.0, 0.0), neighbour=False)
