"""The premises of tests/test_gpu_list_boundaries.py, held on the CPU oracle alone (no GPU): for every list length and stop
position the GPU file uses, the builders of tests/list_scenes.py give the list they promise — its length, where its walk
ends, how far every saturation decision stays from its threshold, and gradient rows with signal on the list boundaries."""
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


@pytest.mark.parametrize("L", sorted({c + d for c in ls.BIN_FIRST_VIEWS.values() for d in (-1, 0, 1)} | set(ls.BIN_FIRST_VIEWS)))
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
