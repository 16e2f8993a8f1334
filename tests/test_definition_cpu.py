"""The float64 definition of the forward (tests/definition_ref.py) on the CPU:
  1. known answers for the definition itself, from closed forms and the reference's own get_rect vectors — not from the oracle;
  2. the oracle (oracle/gsr_oracle.c) against the definition on the filtered scenes: culling, radii, rects, duplication, order,
     ranges and n_contrib exactly, image and T within the forward tolerance with no outliers;
  3. the comparator fails on every corruption it is there to catch;
  4. gradient_rows.f64_gradients stands on the definition's structure as well as on the oracle's."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import definition_ref as dr
import fuzz_scenes as fz
from oracle.oracle import Camera

SH0 = 0.28209479177387814


def _scene(means, opac, colours, scale=0.1, W=64, H=48, f=50.0, mode="rgb", bg=(0.25, 0.5, 0.75)):
    """Isotropic Gaussians of degree-0 colour `colours` (what max(0, SH0 · sh + 0.5 + eps) gives back), identity pose."""
    n = len(means)
    shs = ((np.asarray(colours, np.float64) - 0.5 - dr.EPS32) / SH0).reshape(n, 1, 3).astype(np.float32)
    rots = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    return fz.FuzzScene(np.asarray(means, np.float32), shs, np.asarray(opac, np.float32), np.full((n, 3), scale, np.float32), rots,
                        Camera(W, H, (np.float32(f), np.float32(f))), 0, mode, bg, np.random.default_rng(0))


def _colour(fs):
    return np.maximum(0.0, SH0 * fs.shs[:, 0, :].astype(np.float64) + 0.5 + dr.EPS32)


# ---- 1. known answers ----
def test_one_isotropic_gaussian_on_the_optical_axis():
    fs = _scene([[0, 0, 4]], [0.7], [[0.9, 0.2, 0.4]])
    defn = dr.define(fs)
    d = defn.d
    var = (50.0 * float(np.float32(0.1)) / 4.0) ** 2 + float(np.float32(0.3))          # Sigma_2 = (f s / z)^2 + 0.3, isotropic
    assert np.allclose(d.cov2[0], var * np.eye(2), rtol=1e-12) and np.allclose(d.mu[0], (32.0, 24.0), atol=1e-12)
    assert np.isclose(d.lam[0], var + np.sqrt(0.1), rtol=1e-12)                        # mid^2 - det = 0 -> the 0.1 floor
    assert 4.0 < d.r3[0] < 5.0 and d.radii[0] == 5                                     # 3 sqrt(1.8625 + 0.3162) = 4.43
    # floor((32 - 5) / 16) = 1, floor((32 + 5 + 15) / 16) = 3;  floor((24 - 5) / 16) = 1, floor((24 + 5 + 15) / 16) = 2
    assert tuple(d.rect[0]) == (1, 1, 3, 2) and d.tiles_touched[0] == 2
    assert defn.tl.n_rendered == 2 and list(defn.tl.values_sorted) == [0, 0]
    # A.7: tiles 5 and 6 of the 4 x 3 grid hold one entry each, every other range stays (0, 0)
    want = np.zeros((12, 2), np.uint32)
    want[5], want[6] = (0, 1), (1, 2)
    assert np.array_equal(defn.tl.ranges, want)
    c, bg = _colour(fs)[0], np.array(fs.bg)
    for x, y in ((30, 23), (32, 24), (35, 26), (28, 24), (32, 28)):
        alpha = min(0.99, float(np.float32(0.7)) * np.exp(-0.5 * ((32 - x) ** 2 + (24 - y) ** 2) / var))
        assert alpha >= 1 / 255
        assert np.allclose(defn.r.image[y, x], c * alpha + (1 - alpha) * bg, rtol=1e-12)
        assert np.isclose(defn.r.T[y, x], 1 - alpha, rtol=1e-12) and defn.r.n_contrib[y, x] == 1
    # 5 px from the centre alpha = 0.7 exp(-25 / 3.725) < 1/255: skipped, not counted; tile 4 is outside the rect: nothing to look at
    assert 0.7 * np.exp(-0.5 * 25 / var) < 1 / 255
    for x, y in ((36, 27), (15, 24)):
        assert np.array_equal(defn.r.image[y, x], bg) and defn.r.T[y, x] == 1.0 and defn.r.n_contrib[y, x] == 0


def test_two_gaussians_one_occluding_the_other():
    fs = _scene([[0, 0, 6], [0, 0, 4]], [0.5, 0.6], [[0.1, 0.8, 0.3], [0.9, 0.2, 0.4]], mode="rgbd")
    defn = dr.define(fs)
    assert list(defn.tl.lists[5]) == [1, 0]                      # the nearer one first, whatever its id
    c, bg = _colour(fs), np.array(fs.bg + (0.0, 0.0))
    feat = np.concatenate([c, [[6.0, 1.0], [4.0, 1.0]]], 1)     # rgb | depth | 1
    v1 = (50.0 * float(np.float32(0.1)) / 4.0) ** 2 + float(np.float32(0.3))
    v2 = (50.0 * float(np.float32(0.1)) / 6.0) ** 2 + float(np.float32(0.3))
    x, y = 31, 25
    r2 = (32 - x) ** 2 + (24 - y) ** 2
    a1 = float(np.float32(0.6)) * np.exp(-0.5 * r2 / v1)
    a2 = float(np.float32(0.5)) * np.exp(-0.5 * r2 / v2)
    T = (1 - a1) * (1 - a2)
    assert np.allclose(defn.r.image[y, x], feat[1] * a1 + feat[0] * a2 * (1 - a1) + T * bg, rtol=1e-12)
    assert np.isclose(defn.r.T[y, x], T, rtol=1e-12) and defn.r.n_contrib[y, x] == 2


def test_the_entry_that_crosses_the_stop_is_not_blended():
    # a wall of alpha = 0.8 at the centre pixel: T = 0.2, 0.04, 0.008, 0.0016, 0.00032, then T' = 0.000064 < 1e-4
    n = 9
    fs = _scene([[0, 0, 3 + 0.5 * k] for k in range(n)][::-1], [0.8] * n, np.linspace(0.1, 0.9, 3 * n).reshape(n, 3))
    defn = dr.define(fs, want_uncertainty=True)
    x, y = 32, 24
    o = float(np.float32(0.8))
    assert list(defn.tl.lists[5]) == list(range(n))[::-1]
    assert defn.r.n_contrib[y, x] == 5 and np.isclose(defn.r.T[y, x], (1 - o) ** 5, rtol=1e-12)
    c = _colour(fs)[::-1]                                        # in list order
    want = sum(c[k] * o * (1 - o) ** k for k in range(5)) + (1 - o) ** 5 * np.array(fs.bg)
    assert np.allclose(defn.r.image[y, x], want, rtol=1e-12)
    assert np.isclose(defn.r.uncertainty[y, x], 1 - (1 - o) ** 5, rtol=1e-12)


def test_get_rect_vectors_of_the_reference():
    # K1 (test_oracle_math.test_get_rect): pixel (0, 0) on a 64 x 64 grid, radius 1 and radius 17
    rmin, rmax, _, _ = dr.tile_rect(np.zeros((2, 2)), np.array([1.0, 17.0]), (64, 64))
    assert rmin.tolist() == [[0, 0], [0, 0]] and rmax.tolist() == [[1, 1], [2, 2]]
    # and the clamp to the grid
    rmin, rmax, _, _ = dr.tile_rect(np.array([[1000.0, -40.0]]), np.array([17.0]), (4, 3))
    assert rmin.tolist() == [[4, 0]] and rmax.tolist() == [[4, 0]]


def test_culls_and_margins():
    # behind the near plane / beyond the far plane / sub-pixel (radius <= 3) / off-screen: culled; one z on the near plane: fragile
    fs = _scene([[0, 0, 4], [0, 0, 0.1], [0, 0, 2000], [0, 0, 4], [30, 0, 4], [0, 0, float(np.float32(0.2)) * (1 + 5e-5)]],
                [0.5] * 6, [[0.5] * 3] * 6)
    fs.scales[3] = 1e-3
    d = dr.decide(fs.means, fs.scales, fs.rots, fs.cam)
    assert d.visible.tolist() == [True, False, False, False, False, True]
    assert d.radii[3] == 0 and d.radius[3] == 3                 # ceil(3 sqrt(0.3 + 0.316)) = 3: not above the clip
    assert d.fragile_gaussian.tolist() == [False, False, False, False, False, True]
    assert dr.robust_scene(fs).means.shape[0] == 5


# ---- 2. the oracle against the definition ----
def oracle_got(orc, fs):
    st = orc.forward(fs.means, fs.shs, fs.opac, fs.scales, fs.rots, fs.cam, fs.deg, background=fs.bg, mode=fs.mode)
    rect = np.zeros((fs.means.shape[0], 4), np.int64)
    P = lambda a, ct: a.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    g = np.asarray(fs.cam.grid, np.int32)
    rmin, rmax = np.zeros(2, np.int32), np.zeros(2, np.int32)
    for i in np.flatnonzero(st.radii > 0):
        px = np.ascontiguousarray(st.means2d[i], np.float32)
        orc.lib().orc_get_rect(P(px, C.c_float), int(st.radii[i]), P(g, C.c_int), P(rmin, C.c_int), P(rmax, C.c_int))
        rect[i] = (rmin[0], rmin[1], rmax[0], rmax[1])
    return st, SimpleNamespace(radii=st.radii, tiles_touched=st.tiles_touched, rect=rect, n_rendered=st.n_rendered,
                               values_sorted=st.values_sorted, ranges=st.ranges, image=st.image, T=st.accum_alpha, n_contrib=st.n_contrib)


@pytest.mark.parametrize("name", dr.CPU_SCENES)
def test_oracle_matches_the_definition(pkg, orc, name):
    defn = dr.definition(pkg, name)
    dr.conditions(defn)
    _, got = oracle_got(orc, defn.fs)
    m = dr.check_against_definition(defn, got, lists="reference", outliers=0.0)
    print(f"{name} ({defn.fs.mode}): oracle worst non-fragile |image - definition| = {m['worst_image']:.3g} (fmax {defn.fmax:.3g}), "
          f"|T - definition| = {m['worst_T']:.3g}; worst fragile {m['worst_fragile']:.3g}")


def test_oracle_side_outputs_match_the_definition(pkg, orc):
    defn = dr.definition(pkg, dr.SIDE_SCENE, side=True)
    dr.conditions(defn)
    fs, r = defn.fs, defn.r
    assert fs.mode == "rgb" and r.covisibility.any() and not r.covisibility[defn.d.visible].all()
    st = orc.forward(fs.means, fs.shs, fs.opac, fs.scales, fs.rots, fs.cam, fs.deg, background=fs.bg, mode=fs.mode, want_covis=True,
                     want_uncert=True)
    ok = ~r.fragile_pixel
    du = np.abs(st.uncertainties - r.uncertainty)
    print(f"{dr.SIDE_SCENE}: oracle worst non-fragile |uncertainty - definition| = {du[ok].max():.3g}; covisible "
          f"{int(r.covisibility.sum())} of {defn.d.n}, {int(r.covis_fragile.sum())} with a T ~ 0.5 pixel")
    assert du[ok].max() <= 1e-4 and du.max() <= 2.0 / 255.0
    sure = ~r.covis_fragile
    assert np.array_equal(st.covisibilities.astype(bool)[sure], r.covisibility[sure])


def test_scene_premises(pkg):
    longest = {nm: dr.definition(pkg, nm).shares["longest"] for nm in dr.DEEP}
    assert 1024 < longest[dr.DEEP[0]] <= 4096 < longest[dr.DEEP[1]] <= 5500, longest
    assert dr.definition(pkg, "single-tile").d.grid == (1, 1)
    rag = dr.definition(pkg, "ragged").d
    assert rag.W % 16 and rag.H % 16 and rag.grid[0] > 1 and rag.grid[1] > 1
    ties = dr.definition(pkg, "ties")
    z = ties.d.z
    assert np.unique(z[ties.d.visible]).size == dr.TIE_LEVELS
    assert np.array_equal(z.astype(np.float32).view(np.uint32), ties.fs.means[:, 2].view(np.uint32))   # identity pose: z exact in fp32
    tied = sum(int((np.diff(z[l]) == 0).sum()) for l in ties.tl.lists)
    assert tied >= 0.5 * ties.tl.n_rendered
    for l in ties.tl.lists:
        assert (np.diff(l)[np.diff(z[l]) == 0] > 0).all()        # A.6: equal depths in id order
    assert {dr.definition(pkg, nm).fs.mode for nm in dr.GPU_SCENES} == {"rgb", "rgbd", "rgbdn"}
    for nm in ("edge-0", "edge-4"):
        cam = dr.definition(pkg, nm).fs.cam
        assert cam.near_plane > 0.2 and cam.far_plane < 1000 and cam.focal[0] != cam.focal[1]
        z = dr.decide(*[getattr(dr.build_scene(pkg, nm), k) for k in ("means", "scales", "rots")], cam).z
        assert ((z > 0.2) & (z < cam.near_plane)).any() and ((z > cam.far_plane) & (z < 1000)).any()   # both planes cut


# ---- 3. the comparator can fail ----
MUTATION_SCENE = "sweep-5"


def _tile_with(defn, pred):
    return next(t for t, l in enumerate(defn.tl.lists) if pred(t, l))


def _swap_adjacent(defn, got, lists):
    t = _tile_with(defn, lambda t, l: (np.diff(defn.d.z[l]) > 0).any())
    k = int(np.flatnonzero(np.diff(defn.d.z[defn.tl.lists[t]]) > 0)[0]) + int(got.ranges[t, 0])
    got.values_sorted[[k, k + 1]] = got.values_sorted[[k + 1, k]]


def _drop_last_entry(defn, got, lists):
    t = _tile_with(defn, lambda t, l: len(l) > 1 and (lists == "reference" or defn.blend[t][-1] > 0))
    e = int(got.ranges[t, 1])
    got.values_sorted = np.delete(got.values_sorted, e - 1)
    got.ranges[got.ranges >= e] -= 1
    got.n_rendered -= 1


def _move_range_boundary(defn, got, lists):
    t = _tile_with(defn, lambda t, l: len(l) > 1 and t + 1 < len(defn.tl.lists) and len(defn.tl.lists[t + 1]) > 1)
    got.ranges[t, 1] -= 1
    got.ranges[t + 1, 0] -= 1


def _radius(delta):
    def f(defn, got, lists):
        got.radii[np.flatnonzero(defn.d.visible)[3]] += delta
    return f


def _widen_rect(defn, got, lists):
    i = int(np.flatnonzero(defn.d.visible & (defn.d.rect[:, 2] < defn.d.grid[0]))[0])
    got.rect[i, 2] += 1
    got.tiles_touched[i] = (got.rect[i, 2] - got.rect[i, 0]) * (got.rect[i, 3] - got.rect[i, 1])


def _n_contrib_off_by_one(defn, got, lists):
    ys, xs = np.nonzero(~defn.r.fragile_pixel & (defn.r.n_contrib > 1))
    got.n_contrib[ys[0], xs[0]] -= 1


def _leave_out_a_contributor(defn, got, lists):
    """One pixel re-blended without its heaviest entry (weight above 1e-3): what a walk that skipped it would write."""
    d, gx = defn.d, defn.d.grid[0]
    for t, w in enumerate(defn.r.weights):
        ys, xs = dr._tile_pixels(d, t)
        ok = ~defn.r.fragile_pixel[ys, xs]
        if w.size and (w[ok] > 1e-3).any():
            p = int(np.flatnonzero(ok & (w > 1e-3).any(1))[0])
            j = int(np.argmax(w[p]))
            ids = defn.tl.lists[t]
            alpha_j = w[p, j] / (np.prod(1 - _alphas(w[p])[:j]))
            wp = w[p].copy()
            wp[j + 1:] /= (1 - alpha_j)
            wp[j] = 0.0
            Tp = defn.r.T[ys[p], xs[p]] / (1 - alpha_j)
            bg = np.zeros(defn.feat.shape[1])
            bg[:3] = defn.fs.bg
            got.image[ys[p], xs[p]] = wp @ defn.feat[ids] + Tp * bg
            got.T[ys[p], xs[p]] = Tp
            return
    raise AssertionError("no contributor above 1e-3")


def _alphas(w):
    """alpha_k of one pixel from its blend weights w_k = alpha_k prod_{j<k} (1 - alpha_j)."""
    a, T = np.zeros_like(w), 1.0
    for k, wk in enumerate(w):
        a[k] = wk / T
        T *= 1 - a[k]
    return a


def _remove_a_sure_entry(defn, got, lists):
    t = _tile_with(defn, lambda t, l: (defn.blend[t] > 0).sum() > 2)
    k = int(np.flatnonzero(defn.blend[t] > 0)[1]) + int(got.ranges[t, 0])
    got.values_sorted = np.delete(got.values_sorted, k)
    got.ranges[got.ranges > k] -= 1
    got.n_rendered -= 1


CORRUPTIONS = {"reference": {"adjacent entries swapped": _swap_adjacent, "last entry of a list dropped": _drop_last_entry,
                             "range boundary moved": _move_range_boundary, "radius + 1": _radius(1), "radius - 1": _radius(-1),
                             "rect widened": _widen_rect, "n_contrib off by one": _n_contrib_off_by_one,
                             "contributor left out": _leave_out_a_contributor},
               "culled": {"sure entry removed": _remove_a_sure_entry, "entries reordered": _swap_adjacent,
                          "radius + 1": _radius(1), "rect widened": _widen_rect, "n_contrib off by one": _n_contrib_off_by_one,
                          "contributor left out": _leave_out_a_contributor}}


def culled_got(defn):
    """A definition-made record of an exact-cull forward: the `surely not` entries left out of every list; image, T and the last
    blended entry are unchanged by that (alpha < 1/255 everywhere in the tile)."""
    got = dr.got_from_definition(defn)
    lists = [l[b >= 0] for l, b in zip(defn.tl.lists, defn.blend)]
    lengths = np.array([len(l) for l in lists])
    ends = np.cumsum(lengths)
    got.ranges = np.stack([ends - lengths, ends], 1).astype(np.int64)
    got.values_sorted = np.concatenate(lists).astype(np.int64)
    got.n_rendered = int(lengths.sum())
    for t, (l, full) in enumerate(zip(lists, defn.tl.lists)):
        ys, xs = dr._tile_pixels(defn.d, t)
        cnt = defn.r.n_contrib[ys, xs]
        if len(full):
            last = np.where(cnt > 0, full[np.maximum(cnt, 1) - 1], -1)
            got.n_contrib[ys, xs] = _positions(l, last)
    return got


def _positions(lst, ids):
    """1-based position in `lst` of each of `ids` (-1 -> 0)."""
    pos = {int(v): k + 1 for k, v in enumerate(lst)}
    return np.array([pos.get(int(i), 0) for i in ids])


@pytest.mark.parametrize("lists", ["reference", "culled"])
def test_comparator_accepts_the_definition_and_catches_every_corruption(pkg, lists):
    defn = dr.definition(pkg, MUTATION_SCENE)
    make = dr.got_from_definition if lists == "reference" else culled_got
    clean = make(defn)
    got_int = lambda g: (setattr(g, "ranges", g.ranges.astype(np.int64)), setattr(g, "values_sorted", g.values_sorted.astype(np.int64)))  # noqa: E731
    got_int(clean)
    m = dr.check_against_definition(defn, clean, lists=lists)
    assert m["worst_image"] == 0.0 and m["worst_T"] == 0.0
    if lists == "culled":
        assert clean.n_rendered < defn.tl.n_rendered, "the culled record must differ from the reference lists"
    for what, corrupt in CORRUPTIONS[lists].items():
        got = make(defn)
        got_int(got)
        corrupt(defn, got, lists)
        with pytest.raises(AssertionError):
            dr.check_against_definition(defn, got, lists=lists)
            print(f"NOT CAUGHT under {lists}: {what}")


# ---- 4. the float64 gradients stand on the definition ----
@pytest.mark.parametrize("name", ["sweep-4", "edge-1"])
def test_f64_gradients_on_the_definitions_structure_equal_those_on_the_oracles(pkg, orc, name):
    import gradient_rows as gr
    defn = dr.definition(pkg, name)
    fs = defn.fs
    st, _ = oracle_got(orc, fs)
    assert st.n_rendered > 0
    mine = SimpleNamespace(values_sorted=defn.tl.values_sorted, ranges=defn.tl.ranges, radii=defn.d.radii)
    vp = np.random.default_rng(5).standard_normal((fs.cam.height, fs.cam.width, fs.channels)).astype(np.float32)
    arrays = (fs.means, fs.shs, fs.opac, fs.scales, fs.rots)
    a = gr.f64_gradients(arrays, fs.cam, fs.deg, fs.mode, fs.bg, mine, vp)
    b = gr.f64_gradients(arrays, fs.cam, fs.deg, fs.mode, fs.bg, st, vp)
    for nm in gr.ALL_NAMES:
        assert np.array_equal(a[nm], b[nm]), nm
        assert nm == "vrots" or np.abs(a[nm]).sum() > 0
