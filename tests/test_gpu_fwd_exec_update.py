"""The forward's blend-state update under EXEC (composite.hip fwd_blend_selected / fwd_update_under_exec).

A visit updates T, the last contributor and the colour sums of the lanes of ONE wave-level mask, ok = touch & ~done & ~small,
and `done` itself is a 64-bit mask of the wave.  What can go wrong is a lane updated under a wrong mask: a stopped lane that
blends on, a lane outside the image that wakes up, a whole wave whose mask is empty, a `done` bit set for the wrong lane.
Scenes, on buffers poisoned with GSR_DEBUG_FILL=nan and guarded with GSR_DEBUG_GUARD=1:
  * FULL-TILE STOPS: list_scenes.walled_scene(L, stop) for (65, 2), (130, 64), (130, 65), (300, 256), (300, 257), one tile of
    16 x 16: every pixel stops at the same entry, on either side of a 64-entry ballot and of a 256-entry LDS chunk; every visit
    after it runs with an empty mask; n_contrib == stop at every pixel;
  * A PARTIAL-MASK SCENE (partial_mask_scene): opaque walls over the left columns only, and over the lower-left quadrant only,
    between faint front splats.  Lanes of one wave stop at different entries and one quadrant is finished while its neighbours
    walk on — asserted on the oracle, without a GPU, by test_partial_mask_scene_conditions;
  * PARTIAL TILES: the partial-mask scene and walled (130, 65) behind a 40 x 24 camera: lanes outside the image are `done`
    from the start, nothing outside W x H is written.
Each scene in :rgb, :rgbd and :rgbdn through every instantiation: a state-keeping forward (KEEP), forward_only (KEEP = false),
covisibilities + uncertainties (AUX), each as the first view of a handle (the separate sort and composite_fwd_strip_kernel) and
as the second (sort_composite_fwd_kernel).  The state-keeping forward is held to the oracle by hip_helpers.compare_forward plus
n_contrib and final T; the others, a handle with exact_tile_cull and the second view must be torch.equal to it."""
import numpy as np
import pytest

import list_scenes as ls

W, H = 40, 24
BG = (0.3, 0.1, 0.6)
MODES = ("rgb", "rgbd", "rgbdn")
WALLED = ((65, 2), (130, 64), (130, 65), (300, 256), (300, 257))
SCENES = tuple(f"walled-{L}-{s}" for L, s in WALLED) + ("walled-130-65-wide", "partial", "partial-wide")

PARTIAL_L = 300
# sorted positions of the column walls (left columns of the tile) and of the lower-left walls: on both sides of the 64-entry
# ballots and of the 256-entry chunk, the last ones in the second chunk
COLUMN_WALLS = (21, 41, 62, 63, 65, 66, 101, 131, 201, 254, 255, 256, 257, 281)
LOWER_LEFT_WALLS = tuple(range(8, 8 + 4 * 30, 4))


def _wall(depth, centre, sigma_xy, fx, colour, deg):
    """An opaque axis-aligned splat: sigma_xy px along x and y around `centre` (pixel coordinates of the 16 x 16 tile)."""
    s = np.array([sigma_xy[0], sigma_xy[1], min(sigma_xy)]) * depth / fx
    mean = np.array([(centre[0] - 8.0) * depth / fx, (centre[1] - 8.0) * depth / fx, depth])
    shs = np.zeros(((deg + 1) ** 2, 3))
    shs[0] = (np.asarray(colour) - 0.5) / ls.SH0
    return mean, shs, s, np.array([1.0, 0.0, 0.0, 0.0])


def partial_mask_scene(L=PARTIAL_L, seed=23, deg=0):
    """One tile, L entries, the last one the full-tile backdrop of single_tile_scene (whoever has not stopped ends with
    n_contrib == L).  Column walls: sigma 2 px in x around column 1.5, 160 px in y, opacity 0.97 — alpha 0.94 on columns 1-2,
    0.73 on 0 and 3, 0.44 / 0.21 / 0.08 / 0.02 on columns 4-7: the left columns of the two left quadrants stop after 4 to 9 of
    them, at different entries, and columns 6-7 never do.  Lower-left walls: sigma 4 px around (3.5, 11.5), alpha 0.45 to 0.97
    inside that quadrant: it is finished after about sixteen of them while the three others walk on.  Everything else is the
    faint front of single_tile_scene, in front of, between and behind the walls."""
    rng = np.random.default_rng([int(seed), int(L)])
    cam = ls._camera()
    fx = float(cam.focal[0])
    depths = ls._unique_depths(rng, L - 1)
    kind = np.zeros(L - 1, np.int64)
    kind[list(COLUMN_WALLS)] = 1
    kind[list(LOWER_LEFT_WALLS)] = 2
    assert not set(COLUMN_WALLS) & set(LOWER_LEFT_WALLS) and max(COLUMN_WALLS + LOWER_LEFT_WALLS) < L - 1
    front = np.flatnonzero(kind == 0)
    K = (deg + 1) ** 2
    means, shs, opac = np.zeros((L, 3)), np.zeros((L, K, 3)), np.zeros(L)
    scales, rots = np.zeros((L, 3)), np.zeros((L, 4))
    pinned = np.isin(front, ls.boundary_positions(L))
    fm, fs, fo, fsc, fr = ls._front(rng, front.size, depths[front], 1.5, 0.008, fx, pinned, deg)
    means[front], shs[front], opac[front], scales[front], rots[front] = fm, fs, fo, fsc, fr
    for p in np.flatnonzero(kind):
        colour = rng.uniform(0.1, 0.9, 3)
        centre, sig = ((1.5, 7.5), (2.0, 160.0)) if kind[p] == 1 else ((3.5, 11.5), (4.0, 4.0))
        means[p], shs[p], scales[p], rots[p] = _wall(depths[p], centre, sig, fx, colour, deg)
        opac[p] = 0.97
    means[L - 1], shs[L - 1], scales[L - 1], rots[L - 1] = ls._full_tile(9.0, 40.0, fx, (0.8, 0.3, 0.6), deg)
    opac[L - 1] = 0.9
    order = np.concatenate([rng.permutation(L - 1), [L - 1]]).astype(np.int64)
    return ls._pack([means, shs, opac, scales, rots], order, cam, deg, tuple(np.flatnonzero(kind)))


def _build(name):
    from test_gpu_bwd_instance_trims import wide
    if name.startswith("walled"):
        L, stop = (int(x) for x in name.split("-")[1:3])
        sc = ls.walled_scene(L, stop, 19)
    else:
        sc = partial_mask_scene()
    return wide(sc) if name.endswith("wide") else sc


_refs = {}


def reference(orc, name, mode):
    """Scene and oracle forward (with the side outputs) of a case: computed once, shared, read-only."""
    if (name, mode) not in _refs:
        sc = _build(name)
        st = orc.forward(*sc.args, sc.cam, sc.deg, background=BG, mode=mode, want_covis=True, want_uncert=True)
        for a in (st.image, st.n_contrib, st.accum_alpha, st.values_sorted, st.covisibilities, st.uncertainties):
            a.setflags(write=False)
        _refs[(name, mode)] = (sc, st)
    return _refs[(name, mode)]


def _quadrants(nc):
    """n_contrib of the four 8 x 8 quadrants of the first tile, in the kernels' order (qx = q & 1, qy = q >> 1)."""
    return [nc[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8] for q in range(4)]


# ------------------------------------------------------------------------------------------------------------------
# CPU: the scenes are what the GPU cases need them to be, on the oracle
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["partial", "partial-wide"])
def test_partial_mask_scene_conditions(orc, name):
    sc, st = reference(orc, name, "rgb")
    L = PARTIAL_L
    first = ls.list_positions(st)
    assert np.array_equal(first, sc.order), "one instance per Gaussian in the first tile's list, in the built order"
    quads = _quadrants(np.asarray(st.n_contrib).reshape(sc.cam.height, sc.cam.width))
    stopped = [np.unique(q[q < L]) for q in quads]
    # lanes of one wave stop at different entries, while other lanes of that wave walk to the end: partial masks
    mixed = [q for q in range(4) if stopped[q].size >= 2 and (quads[q] == L).any()]
    assert mixed, [s.tolist() for s in stopped]
    # ... some of them on either side of a 64-entry ballot and in the second 256-entry chunk
    every = np.concatenate(stopped)
    assert (every < 64).any() and ((every >= 64) & (every < 256)).any() and (every > 256).any(), np.unique(every)
    # a whole quadrant is finished (well before the list ends) while another quadrant of the tile goes on
    finished = [q for q in range(4) if (quads[q] < L).all()]
    assert finished and max(int(quads[q].max()) for q in finished) < 256, [int(q.max()) for q in quads]
    assert any((quads[q] == L).any() for q in range(4) if q not in finished)
    print(f"{name}: stop entries per quadrant {[s.tolist() for s in stopped]}, finished {finished}")


@pytest.mark.parametrize("L,stop", WALLED)
def test_walled_scene_conditions(orc, L, stop):
    sc, st = reference(orc, f"walled-{L}-{stop}", "rgb")
    assert (np.asarray(st.n_contrib) == stop).all() and st.n_rendered == L


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _forward(run, forward_only=False, image_out=None):
    import torch
    img = run.rast.forward_raw(*run.t, run.camera, run.deg, run.bg, run.Rd, run.td, run.covis, run.unc, image_out=image_out,
                               forward_only=forward_only)
    torch.cuda.synchronize()
    return img


def _outputs(run, img):
    return dict(image=img.clone(), final_T=run.rast.accum_alpha.clone(), n_contrib=run.rast.n_contrib.clone())


def _same(a, b, what):
    import torch
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_every_forward_path_against_the_oracle(pkg, orc, name, mode):
    import torch
    from hip_helpers import HipRun, compare_forward, frac_bad
    from test_gpu_bwd_instance_trims import env
    from test_gpu_guarded_handle import guards_ok
    sc, st = reference(orc, name, mode)
    h, w = sc.cam.height, sc.cam.width
    C = st.image.shape[2]
    walled = name.startswith("walled")
    stop = int(name.split("-")[2]) if walled else None
    with env("GSR_DEBUG_FILL", "nan"), env("GSR_DEBUG_GUARD", "1"):
        def handle(**kw):
            return HipRun(pkg, *sc.args, sc.cam, sc.deg, BG, mode, **kw)

        # the state-keeping forward, into an image with a poisoned tail: first view (strip kernel), second view (fused kernel)
        keep = handle()
        arena = torch.full((h * w * C + 4096,), float("nan"), device="cuda")
        views = []
        for view in range(2):
            arena.fill_(float("nan"))
            img = _forward(keep, image_out=arena[:h * w * C].view(h, w, C))
            assert torch.isnan(arena[h * w * C:]).all(), "written behind the image"
            compare_forward(st, keep, img, sc.opac)
            out = _outputs(keep, img)
            nc = out["n_contrib"].cpu().numpy().astype(np.uint32)
            differ = int((nc != np.asarray(st.n_contrib).reshape(h, w)).sum())
            print(f"{name} {mode} view {view}: n_contrib differs from the oracle's at {differ} pixels")
            for k, v in out.items():
                assert torch.isfinite(v.float()).all(), f"{k}: a pixel inside the image was not written"
            if walled:
                assert differ == 0
                assert (nc[:16, :16] == stop).all(), "every pixel of the first tile stops at the walls"
            guards_ok(pkg, keep.rast)
            views.append(out)
        _same(views[0], views[1], "two forwards of one view")
        want = views[0]

        # KEEP = false
        only = handle()
        for view in range(2):
            _same(want, _outputs(only, _forward(only, forward_only=True)), f"forward_only, view {view}")
        guards_ok(pkg, only.rast)

        # AUX: the same pixels, and the side outputs against the oracle's
        aux = handle(want_covis=True, want_uncert=True)
        for view in range(2):
            aux.covis.zero_()
            aux.unc.fill_(float("nan"))
            _same(want, _outputs(aux, _forward(aux)), f"covisibilities + uncertainties, view {view}")
            assert (aux.covis.cpu().numpy() != st.covisibilities).mean() <= 5e-3
            assert frac_bad(aux.unc.cpu().numpy(), st.uncertainties, 0, 1e-4) <= 1e-4
        aux_only = handle(want_covis=True, want_uncert=True)
        for view in range(2):
            _same(want, _outputs(aux_only, _forward(aux_only, forward_only=True)), f"AUX forward_only, view {view}")
            assert torch.equal(aux_only.covis, aux.covis) and torch.equal(aux_only.unc, aux.unc)
        guards_ok(pkg, aux.rast)
        guards_ok(pkg, aux_only.rast)

        # the library's default lists: shorter lists (other positions in n_contrib), the same pixels bit for bit
        cull = handle(exact_tile_cull=True)
        for view in range(2):
            got = _outputs(cull, _forward(cull))
            assert torch.equal(got["image"], want["image"]) and torch.equal(got["final_T"], want["final_T"]), f"exact_tile_cull, view {view}"
        guards_ok(pkg, cull.rast)
