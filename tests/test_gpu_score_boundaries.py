"""-m gpu: the contribution scores of gsr_forward_scored on tile lists of a CHOSEN length — every edge of the scored kernels' own
code: the 64-entry ballot groups, the 256-entry chunk with its flush and re-zeroing, the 1024 cut between the fused
launch and the tier walk, the walk's 64-entry batches, and a walk that saturates in the middle of a chunk.

The scenes are those of tests/list_scenes.py as definitions (tests/score_scenes.py; premises in tests/test_scores_cpu.py): the
filter removes nothing, so a list has exactly the length asked for, and the hit interval of (almost) every Gaussian is ONE value —
"inside the interval" is "the exact hit count per Gaussian".  Every case: default handle and reference lists, two consecutive views
on one handle into separate sets (the first view of a handle runs the separate sort and the strip forward, the second the fused
launch), each inside the intervals with the project's TOL, the two sets torch.equal, and the path asserted from gsr_stats.

  full walk      23 lengths :rgb; :rgbd / :rgbdn (six waves in the fused kernel, a fourth stream plane in the walk) at 256 .. 1025
  early stop     walls end every pixel's walk inside a chunk, on its edge, inside a batch of the walk, on the 1024 cut: nothing
                 behind the stop has a word set; image, final_T and n_contrib are the unscored forward's
  two tiles      a list of the fused launch's and one of the tier walk's beside ten entries: both kernels write one set in one call
  equal depths   groups of 5 depth levels: scores are per Gaussian id, whatever the tie order
  mixed grid     4 x 3 tiles, all three tiers beside fused tiles
  257 long tiles no definition (270 k Gaussians): the same bits on every path, and the file's identities
  redo paths     a view whose early fused launch finds the instance buffers too small, with an empty and with a pre-filled set"""
import numpy as np
import pytest
import torch

import list_scenes as ls
import score_scenes as ss
import scores_ref as sr
from hip_helpers import HipRun, dev
from test_gpu_contribution_scores import arrays, new_scores, same, score
from test_gpu_definition import hip_run
from test_gpu_list_boundaries import tier_of
from test_gpu_preprocess_forms import form

pytestmark = pytest.mark.gpu


def expected_path(defn, exact):
    """(tier_tiles, max_tile_instances) the view must report, or None where the definition does not decide it: reference lists are
    the definition's; the default handle drops the instances that reach alpha >= 1/255 nowhere in their tile, so its lists are
    the definition's only where every entry surely blends (definition_ref.blendable)."""
    if exact and not all((b > 0).all() for b in defn.blend):
        return None
    tiers = [sum(tier_of(L)[k] for L in defn.lengths) for k in range(3)]
    return tiers, max(defn.lengths)


def check_path(defn, run, exact):
    s = run.rast.stats
    want = expected_path(defn, exact)
    if want is not None:
        assert list(s.tier_tiles) == want[0] and int(s.max_tile_instances) == want[1], (list(s.tier_tiles), s.max_tile_instances, want)
        assert int(s.n_rendered) == sum(defn.lengths)
        return
    # the default handle on a scene with entries that blend nowhere: every list holds its surely blending entries and may hold
    # the others (the cull is conservative: tests/test_gpu_definition.py asks for a subsequence with every sure entry, no more)
    lo = [int((b > 0).sum()) for b in defn.blend]
    hi = list(defn.lengths)
    assert sum(lo) <= int(s.n_rendered) <= sum(hi) and max(lo) <= int(s.max_tile_instances) <= max(hi)
    for k, (a, b) in enumerate(((1024, 4096), (4096, 8192), (8192, 1 << 30))):
        sure = sum(a < x and y <= b for x, y in zip(lo, hi))
        maybe = sum(x <= b and y > a for x, y in zip(lo, hi))
        assert sure <= int(s.tier_tiles[k]) <= maybe, (k, list(s.tier_tiles), lo, hi)


def check_case(pkg, case, mode="rgb"):
    """Two scored views per handle, default handle and reference lists; returns the (equal) score sets of both handles' second views."""
    defn, iv = ss.definition(case, mode), ss.intervals(case)
    stop = case[2] if case[0] == "walled" else None
    out = []
    for exact in (True, False):
        run = hip_run(pkg, defn, exact)
        sets = [new_scores(pkg, run), new_scores(pkg, run)]
        for view, sc in enumerate(sets):
            img = score(run, sc).clone()
            check_path(defn, run, exact)
            s = run.rast.stats
            assert int(s.compact_binning) == 0 and int(s.fused_relaunches) == 0
            m = sr.check_scores(iv, *arrays(sc))
            print(f"{defn.name} ({mode}, {'default' if exact else 'reference lists'}, view {view}): lists {list(defn.lengths)}, tiers "
                  f"{list(s.tier_tiles)}, longest {s.max_tile_instances}; hits {int(sc.hits.sum())} in [{int(iv.hits_lo.sum())}, "
                  f"{int(iv.hits_hi.sum())}], worst |max_weight - definition| {m['worst_max_weight']:.3g}, worst |weight_sum - "
                  f"definition| / hits {m['worst_weight_sum_per_hit']:.3g} over {m['exact']} Gaussians with exact hits")
            assert sc.n_views == 1
            if stop is not None:
                behind = torch.as_tensor(np.array(defn.tl.lists[0][stop:]), device="cuda")    # (a copy: the shared list is read-only)
                assert not sc.hits[behind].any() and not sc.bits[behind].any() and not sc.q[behind].any(), "a word behind the stop"
                T, nc = run.rast.accum_alpha.clone(), run.rast.n_contrib.clone()
                if not exact:
                    assert (nc == stop).all(), "every pixel's walk ends at the stop"
        assert same(*sets), "the first view (separate sort, strip forward) and the second (fused launch) must give the same scores"
        if stop is not None:
            plain = run.forward()
            assert torch.equal(plain, img) and torch.equal(run.rast.accum_alpha, T) and torch.equal(run.rast.n_contrib, nc)
        out.append(sets[1])
        run.rast.close()
    assert same(*out), "default handle and reference lists"
    return out[0]


@pytest.mark.parametrize("L", ss.FULL_LENGTHS)
def test_full_walk_rgb(pkg, L):
    check_case(pkg, ("full", L))


@pytest.mark.parametrize("L", ss.MODE_LENGTHS)
@pytest.mark.parametrize("mode", ["rgbd", "rgbdn"])
def test_full_walk_depth_and_normal_modes(pkg, mode, L):
    sc = check_case(pkg, ("full", L), mode)
    rgb = check_case(pkg, ("full", L))
    assert same(sc, rgb), "the scores read no feature channel"


@pytest.mark.parametrize("L,stop", ss.WALLED)
def test_early_stop(pkg, L, stop):
    check_case(pkg, ("walled", L, stop))


@pytest.mark.parametrize("L", ss.TWO_LENGTHS)
def test_two_tiles(pkg, L):
    check_case(pkg, ("two", L))


@pytest.mark.parametrize("L", ss.TIED_LENGTHS)
def test_equal_depths(pkg, L):
    defn = ss.definition(("tied", L))
    z = defn.d.z[defn.tl.lists[0]]
    assert int((np.diff(z) == 0).sum()) == L - 1 - ss.TIED_GROUPS, "the list must hold its equal-depth runs"
    check_case(pkg, ("tied", L))


def test_mixed_grid(pkg):
    defn = ss.definition(("grid",))
    assert expected_path(defn, False) == ([2, 1, 1], 8193)    # 1025 and 2049 | 4097 | 8193, beside seven fused tiles
    check_case(pkg, ("grid",))


def test_more_than_256_long_tiles(pkg):
    """257 lists of 1025 .. 4096 entries beside a 1024-entry one and ten entries everywhere else: the tier walk over more tiles than
    one launch's worth of single-wave workgroups per CU, scored.  No definition: bit equality across the paths, and the identities."""
    case = (257, 0, 0)
    lengths, _ = ls.many_tile_lengths(case)
    scene = ls.many_tile_scene(*ls.MANY_GRID, lengths, 23)
    base = None
    for f, exact, only in ((0, False, False), (0, True, False), (1, False, False), (0, False, True)):
        with form(pkg, f):
            run = HipRun(pkg, *scene.args, scene.cam, scene.deg, ss.BG, "rgb", exact_tile_cull=exact, want_uncert=True)
            sets = [new_scores(pkg, run), new_scores(pkg, run)]
            for sc in sets:
                score(run, sc, forward_only=only, unc=run.unc)
                s = run.rast.stats
                if not exact:   # (the default handle drops what blends nowhere: most of its 1025-entry lists fall under the cut)
                    assert tuple(s.tier_tiles) == case and int(s.max_tile_instances) == lengths.max() and int(s.n_rendered) == lengths.sum()
                assert int(s.compact_binning) == 0
            assert same(*sets)
            if base is None:
                base = sets[1]
                zero = base.hits == 0
                assert torch.equal(zero, base.bits == 0) and torch.equal(zero, base.q == 0)
                pixels = run.unc.numel()
                total_g, total_p = float(base.weight_sum.sum()), float(run.unc.double().sum())
                print(f"257 long tiles: hits {int(base.hits.sum())}, sum of weight_sum {total_g:.6f}, sum of uncertainties {total_p:.6f}, "
                      f"pixels {pixels}")
                assert int(base.hits.sum()) > 0 and abs(total_g - total_p) <= 1e-4 * pixels
                assert int(base.hits.sum()) <= int(run.rast.n_contrib.long().sum())
            assert same(sets[1], base), (f, exact, only)
            run.rast.close()


# ---- the redo paths: a scored view on a handle whose buffers an earlier, smaller view sized ----
REDO = (("walled", 1000, 512), ("walled", 2500, 1025))
_room = {}


def with_room(pkg, case, exact):
    """The scores of the case on a handle that had room: the second view of a fresh one (computed once, never written again)."""
    if (case, exact) not in _room:
        run = hip_run(pkg, ss.definition(case), exact)
        sc = new_scores(pkg, run)
        score(run, new_scores(pkg, run))
        score(run, sc)
        assert int(run.rast.stats.fused_relaunches) == 0 and int(run.rast.stats.compact_binning) == 0
        _room[case, exact] = sc
        run.rast.close()
    return _room[case, exact]


@pytest.mark.parametrize("prefilled", [False, True], ids=["empty-set", "prefilled-set"])
@pytest.mark.parametrize("exact", [True, False], ids=["default", "reference-lists"])
def test_redone_views_are_scored_exactly_once(pkg, exact, prefilled):
    """A first view of 100 entries sizes the handle (bins of ls.BIN_FIRST_VIEWS[100] keys, instance buffers for some 100); the
    1000-entry and the 2500-entry scenes that follow overflow them: the early fused launch returns at once and the view is redone
    behind the read-back (gsr_stats.fused_relaunches), or its overflowing list is scattered again (compact_binning == 2)."""
    first = ls.single_tile_scene(100, 7)
    run = HipRun(pkg, *first.args, first.cam, first.deg, ss.BG, "rgb", exact_tile_cull=exact)
    run.forward()
    assert int(run.rast.stats.bin_capacity) == ls.BIN_FIRST_VIEWS[100]
    half = int(np.float32(0.5).view(np.int32))
    for case in REDO:
        defn, iv = ss.definition(case), ss.intervals(case)
        fs = defn.fs
        run.t = [dev(np.array(a)) for a in (fs.means, fs.shs, np.asarray(fs.opac).reshape(-1, 1), fs.scales, fs.rots)]
        sc = new_scores(pkg, run)
        if prefilled:
            sc.bits.fill_(half); sc.hits.fill_(5); sc.q.fill_(7)
        before = int(run.rast.stats.fused_relaunches)
        score(run, sc)
        s = run.rast.stats
        print(f"redo {defn.name} ({'default' if exact else 'reference lists'}): fused_relaunches {before} -> {s.fused_relaunches}, "
              f"compact_binning {s.compact_binning}, bin_capacity {s.bin_capacity}, n_rendered {s.n_rendered}")
        assert int(s.fused_relaunches) > before or int(s.compact_binning) == 2, "the view was not redone: the case is mis-built"
        room = with_room(pkg, case, exact)
        if prefilled:
            assert torch.equal(sc.bits, torch.clamp(room.bits, min=half)) and torch.equal(sc.hits, room.hits + 5)
            assert torch.equal(sc.q, room.q + 7)
        else:
            assert same(sc, room), "a redone view's scores are those of a handle that had room"
            sr.check_scores(iv, *arrays(sc))
        sr.check_scores(iv, *arrays(room))
    run.rast.close()
