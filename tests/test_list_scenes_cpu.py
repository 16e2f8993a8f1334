"""The premises of tests/test_gpu_list_boundaries.py, test_gpu_sort_ties.py and test_gpu_tier_routing.py, held on the CPU oracle
alone (no GPU): for every list length, stop position, tie pattern and tier count the GPU files use, the builders of
tests/list_scenes.py give the lists they promise — their lengths and order, where their walks end, how far every saturation
decision stays from its threshold, and gradient rows with signal on the list boundaries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import list_scenes as ls

BG = (0.3, 0.1, 0.6)


def _run(orc, sc, mode="rgb", seed=0):
    st = orc.forward(*sc.args, sc.cam, sc.deg, background=BG, mode=mode)
    vp = np.random.default_rng(seed).standard_normal(st.image.shape).astype(np.float32)
    return st, orc.backward(st, vp, *sc.args, sc.cam, sc.deg, background=BG)


def _full_walk(orc, L):
    sc = ls.single_tile_scene(L, 7)
    st, g = _run(orc, sc, seed=L)
    assert st.n_rendered == L and int((st.radii > 0).sum()) == L
    assert np.array_equal(ls.list_positions(st), sc.order), "sorted position p holds Gaussian order[p]"
    assert sc.order[-1] == L - 1, "the backdrop is the last id and the last entry"
    assert (st.n_contrib == L).all(), "every pixel walks the list to its end"
    assert st.accum_alpha.min() >= 3e-4, st.accum_alpha.min()
    # a wrong visit on a boundary would move a row that is not zero: {0, b-2 .. b+2, L-1} for every boundary b <= L
    rows = g.vmeans[sc.order[ls.boundary_positions(L)]]
    assert (np.abs(rows).max(1) > 0).all()


@pytest.mark.parametrize("L", ls.FULL_WALK_LENGTHS)
def test_single_tile_scene_walks_the_whole_list(orc, L):
    _full_walk(orc, L)


@pytest.mark.parametrize("L", sorted({c + d for c in ls.BIN_FIRST_VIEWS.values() for d in (-1, 0, 1)} | set(ls.BIN_FIRST_VIEWS)
                                     | set(ls.TIED_BIN_FIRST_VIEWS.values())))
def test_single_tile_scene_at_the_bin_capacities(orc, L):
    _full_walk(orc, L)


def test_boundary_positions():
    assert ls.boundary_positions(1).tolist() == [0] and ls.boundary_positions(2).tolist() == [0, 1]
    assert ls.boundary_positions(65).tolist() == [0, 62, 63, 64]
    assert ls.boundary_positions(2049).tolist()[-4:] == [1026, 2046, 2047, 2048]
    P = ls.boundary_positions(70000, stop=5000)
    for b in ls.BOUNDARIES + (5000,):
        assert set(range(b - 2, b + 3)) <= set(P.tolist())
    assert P[0] == 0 and P[-1] == 69999 and (np.diff(P) > 0).all()


@pytest.mark.parametrize("L,stop", ls.EARLY_STOPS)
def test_walled_scene_stops_the_walk_at_the_chosen_entry(orc, L, stop):
    sc = ls.walled_scene(L, stop, 11)
    st, g = _run(orc, sc, seed=stop)
    assert st.n_rendered == L and np.array_equal(ls.list_positions(st), sc.order)
    assert sc.walls == (stop - 2, stop - 1, stop)
    assert np.array_equal(sc.order, ls.walled_scene(L, 500, 11).order), "position -> Gaussian does not depend on the stop"
    assert (st.n_contrib == stop).all(), "the second wall is every pixel's last contributor"
    # margins of the two decisions around the stop, from the transmittance the walk ended with (T behind the second wall):
    # it blended with a factor >= 2 to spare, and the third wall's test fails by a factor >= 2
    a3 = 0.965   # alpha of a wall at the pixel centre farthest from its centre (0.97 · exp(-112.5 / (2 · 144²)) = 0.9674)
    assert st.accum_alpha.min() >= 2e-4 and st.accum_alpha.max() * (1.0 - a3) <= 5e-5
    behind = sc.order[stop:]
    for t in (g.vmeans, g.vshs, g.vopacities, g.vscales, g.vrots):
        assert not np.asarray(t)[behind].any(), "nothing behind the stop receives a gradient"
    for t in (g.vmeans, g.vshs, g.vopacities):
        assert np.asarray(t)[sc.order[[stop - 2, stop - 1]]].reshape(2, -1).any(1).all(), "both walls that blend do"
    front = ls.boundary_positions(L, stop)
    assert (np.abs(g.vmeans[sc.order[front[front < stop]]]).max(1) > 0).all()


@pytest.mark.parametrize("L1", sorted(ls.TWO_TILE_FIRST_VIEWS))
def test_two_tile_scene_keeps_every_splat_in_its_own_tile(orc, L1):
    n2 = ls.TWO_TILE_SECOND
    cap = ls.TWO_TILE_FIRST_VIEWS[L1]
    for L in (L1, cap - 1, cap, cap + 1):
        sc = ls.two_tile_scene(L, n2, 13)
        st, g = _run(orc, sc)
        assert st.n_rendered == L + n2 and (st.tiles_touched == 1).all()
        assert st.ranges.tolist() == [[0, L], [L, L + n2]]
        assert np.array_equal(st.values_sorted, sc.order)
        assert st.accum_alpha.min() >= 3e-4 and st.n_contrib[:, :16].max() <= L and 0 < st.n_contrib[:, 16:].max() <= n2
        # the rows the GPU file reads by themselves carry signal: the first list's boundary positions, all of the second list
        rows = g.vmeans[np.concatenate([sc.order[ls.boundary_positions(L)], sc.order[L:]])]
        assert (np.abs(rows).max(1) > 0).all()


# ---- equal depth bits: tests/test_gpu_sort_ties.py ----
def adjacent_ties(st):
    """Adjacent list entries with the same (tile, depth bits): equal 64-bit keys of the reference's sort."""
    k = np.asarray(st.keys_sorted)
    return int((k[1:] == k[:-1]).sum())


@pytest.mark.parametrize("groups", ls.TIED_GROUPS)
@pytest.mark.parametrize("L", ls.TIED_LENGTHS)
def test_tied_tile_scene_orders_equal_depths_by_id(orc, L, groups):
    sc = ls.tied_tile_scene(L, groups, 17)
    st, g = _run(orc, sc, seed=L)
    n = L - 1
    assert st.n_rendered == L and np.array_equal(ls.list_positions(st), sc.order)
    assert np.array_equal(st.depths.view(np.uint32), sc.means[:, 2].view(np.uint32)), "identity pose: depth bits == bits of z"
    levels = np.unique(sc.means[:n, 2]).size
    assert levels == min(groups, levels) and adjacent_ties(st) == sc.ties == n - levels
    if n >= 20 * groups:
        assert levels == groups, "every level is in use: L - 1 - groups tied pairs"
    # inside a level the ids ascend; groups = 1: the whole front is ONE tie and the list is 0, 1, 2, ...
    z = sc.means[sc.order[:n], 2]
    same = z[1:] == z[:-1]
    assert (np.diff(z) >= 0).all() and (np.diff(sc.order[:n])[same] > 0).all()
    if groups == 1:
        assert np.array_equal(sc.order, np.arange(L))
    assert (st.n_contrib == L).all() and st.accum_alpha.min() >= 3e-4, st.accum_alpha.min()
    rows = g.vmeans[sc.order[ls.boundary_positions(L)]]
    assert (np.abs(rows).max(1) > 0).all()


@pytest.mark.parametrize("L", ls.TIED_MODE_LENGTHS)
def test_tied_tile_scene_in_the_normal_mode(orc, L):
    sc = ls.tied_tile_scene(L, 5, 17)
    st, g = _run(orc, sc, mode="rgbdn", seed=L)
    assert np.array_equal(ls.list_positions(st), sc.order) and adjacent_ties(st) == sc.ties == L - 6
    assert (st.n_contrib == L).all() and st.accum_alpha.min() >= 3e-4


# ---- more than 256 tier tiles: tests/test_gpu_tier_routing.py ----
def test_many_tile_lengths():
    for case in ls.MANY_TILE_CASES:
        lengths, cls = ls.many_tile_lengths(case)
        assert sorted(np.concatenate([cls[c] for c in ls.MANY_CLASSES]).tolist()) == list(range(280))
        assert [int(((lengths > a) & (lengths <= b)).sum()) for a, b in ((1024, 4096), (4096, 8192), (8192, 1 << 30))] == list(case)
        assert (lengths == 1024).sum() == 1 and (lengths[cls["ten"]] == 10).all() and cls["ten"].size == 279 - sum(case)
        assert (lengths == 4096).sum() == min(case[0], 2) and (lengths == 8192).sum() == min(case[1], 2)
        assert (lengths == 4096).sum() + (lengths == 8192).sum() <= 8, "few tiles at the upper edge lengths"
        assert set(lengths.tolist()) <= {10, 1024, 1025, 4096, 4097, 8192, 8193}


@pytest.mark.parametrize("case", list(ls.MANY_TILE_CASES), ids=str)
def test_many_tile_scene_gives_every_tile_its_length(orc, case):
    """Every list has exactly the requested length and order, every splat stays inside its own tile, the deepest contributor of
    every tile is its last entry (the front splats reach alpha = 1/255 within ~3 px of their centre, so `n_contrib == length`
    holds at the pixels the last entry blends into, and nowhere is it larger), and the walk saturates nowhere.
    Two deliberate departures from the premises the issue listed for this builder, both because they cannot hold: "n_contrib
    equals the list length at EVERY pixel" (no splat of sigma 1.05 px reaches a whole tile; the per-tile maximum is asserted
    here, and the GPU file compares n_contrib with the oracle's pixel by pixel), and "opacity 0.05 in lists of up to 1024"
    (a 1024-entry list at 0.05 saturates after some 300 entries; the faint front starts beyond ls.MANY_FAINT_ABOVE = 64)."""
    gx, gy = ls.MANY_GRID
    lengths, cls = ls.many_tile_lengths(case)
    sc = ls.many_tile_scene(gx, gy, lengths, 23)
    st = orc.forward(*sc.args, sc.cam, sc.deg, background=BG)
    vp = np.random.default_rng(sum(case)).standard_normal(st.image.shape).astype(np.float32)
    g = orc.backward(st, vp, *sc.args, sc.cam, sc.deg, background=BG, deterministic="parallel")
    assert st.n_rendered == lengths.sum() == sc.means.shape[0] and (st.tiles_touched == 1).all()
    assert np.array_equal(st.ranges[:, 1].astype(np.int64) - st.ranges[:, 0], lengths)
    assert np.array_equal(st.values_sorted, sc.order) and adjacent_ties(st) == 0
    deepest = st.n_contrib.reshape(gy, 16, gx, 16).max((1, 3)).reshape(-1)
    assert np.array_equal(deepest, lengths), "the last entry of every list blends somewhere"
    assert st.accum_alpha.min() >= 3e-4, st.accum_alpha.min()
    for c in ls.MANY_CLASSES:      # the rows the GPU file reads class by class carry signal
        rows = g.vmeans[ls.tile_rows(sc, cls[c])]
        assert rows.shape[0] >= (1 if cls[c].size else 0) and (np.abs(rows).max(1) > 0).all(), c


def test_backward_split_of_the_tier_routing_cases(pkg, tmp_path):
    """gsr_policy.cpp built with g++ alone (as tests/test_policy.py does): the split of a default 320 x 224 configuration for the
    tier counts of every case, and the counts right beside them."""
    L = pkg._lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "libgsr_policy_only.so"
    src = os.path.join(root, "gaussiansplatting.jl_amd", "csrc", "gsr_policy.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", src, "-o", str(out)], check=True)
    lib = L.bind_policy(C.CDLL(str(out)))
    cfg = L.PolicyConfig()
    lib.gsr_policy_config_init(C.byref(cfg), 16 * ls.MANY_GRID[0], 16 * ls.MANY_GRID[1], 0, -1)
    assert cfg.bwd_split_max_tiles == 256

    def split(*tiers):
        sp = L.BwdSplit()
        lib.gsr_policy_bwd_split(C.byref(cfg), *tiers, C.byref(sp))
        return sp.n_mid4, sp.n_mid8, sp.n_big, sp.split_len

    for case, want in ls.MANY_TILE_CASES.items():
        assert split(*case) == want, case
    assert split(255, 1, 0) == (255, 1, 0, 1024) and split(0, 255, 1) == (0, 255, 1, 1024)
