"""-m gpu: a scored forward (gsr_forward_scored) is a valid forward for gsr_backward.

The scored twin of the fused kernel also does the tile sort: it writes values_sorted, ranges and the instance stream and re-zeroes
the tile counters — everything the backward reads.  tests/test_gpu_contribution_scores.py compares image, final_T and n_contrib with
the unscored forward's; here two handles get the same inputs, one runs scored forwards, the other plain ones, over two views each
(the first view of a handle runs the separate sort and the strip forward, the second the fused launch):

  state        values_sorted, ranges, radii, final_T, n_contrib, the GSR_BUF_GEOM records of the visible rows: torch.equal; n_rendered,
               tier_tiles, compact_binning equal
  backward     the same cotangent: torch.equal on all five gradients and grad_means_2d — default precision on every scene,
               "accurate" and "fp32_reference" on two; no tolerance: the same lists, the same bits
  trainer      gsr_backward_trainer_tail behind a scored forward and behind a plain one: θ, μ, ν of every group, the activated copies
               and grad_means_2d torch.equal over 2 steps
  generations  a scored forward advances gsr_stats.generation and supersedes an earlier plain one like a plain one would;
               gsr_drop_forward behind it refuses the backward; a scored forward-only view refuses it like an unscored one
  other handle features   an antialiased handle scores what a plain handle scores on the opacities o · rho; a device-side pose
               scores what the host pose does"""
import dataclasses

import numpy as np
import pytest
import torch

import definition_ref as dr
import score_scenes as ss
import scores_ref as sr
import test_gpu_antialias as ta
from hip_helpers import HipRun, dev
from test_gpu_contribution_scores import arrays, new_scores, same, score
from test_gpu_definition import hip_run

pytestmark = pytest.mark.gpu

GRADS = ("vmeans", "vshs", "vopacities", "vscales", "vrotations")
SCENES = {"sweep-3": None, "single-tile": None, "ragged": None, "deep-276": None,
          "walled-2500-1025": ("walled", 2500, 1025), "grid": ("grid",)}
CASES = [(name, None) for name in SCENES] + [(name, p) for name in ("sweep-3", "deep-276") for p in ("accurate", "fp32_reference")]


def scene_definition(pkg, name):
    return ss.definition(SCENES[name]) if SCENES[name] else dr.definition(pkg, name)


def geom_records(run):
    L = run.pkg._lib
    n = int(run.t[0].shape[0])
    return run.rast._buffer(L.BUF_GEOM, torch.int32, (n, 16))


def state(run):
    r = run.rast
    visible = r.radii > 0
    rec = dict(values_sorted=r.values_sorted.clone(), ranges=r.ranges.clone(), radii=r.radii.clone(), final_T=r.accum_alpha.clone(),
               n_contrib=r.n_contrib.clone(), geom=geom_records(run)[visible])
    s = r.stats
    return rec, (int(s.n_rendered), tuple(s.tier_tiles), int(s.compact_binning), int(s.max_tile_instances))


@pytest.mark.parametrize("name,precision", CASES)
def test_state_and_backward_behind_a_scored_forward_are_the_plain_ones(pkg, name, precision):
    defn = scene_definition(pkg, name)
    fs = defn.fs
    vp = np.random.default_rng(77).standard_normal((fs.cam.height, fs.cam.width, fs.channels)).astype(np.float32)
    # the fuzz scenes on the default handle; the list scenes on reference lists, where the lists have the lengths they were built for
    exact = SCENES[name] is None
    scored, plain = (hip_run(pkg, defn, exact, grad_precision=precision) for _ in range(2))
    sc = new_scores(pkg, scored)
    for view in range(2):
        a, b = score(scored, sc).clone(), plain.forward().clone()
        assert torch.equal(a, b), view
        (sa, na), (sb, nb) = state(scored), state(plain)
        assert na == nb and na[0] > 0, (view, na, nb)
        for k in sa:
            assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), (k, view)
        ga, gb = scored.backward(vp), plain.backward(vp)
        for k, x, y in zip(GRADS, ga, gb):
            assert torch.equal(x, y), (k, view)
            assert bool(x.abs().sum() > 0), k
        assert torch.equal(scored.rast.grad_means_2d, plain.rast.grad_means_2d), view
    assert sc.n_views == 2 and int(sc.hits.sum()) > 0
    if SCENES[name]:
        assert na[1] == {"walled-2500-1025": (1, 0, 0), "grid": (2, 1, 1)}[name] and na[3] == max(defn.lengths)
    elif name == "deep-276":
        assert sum(na[1]) > 0, "the tier walk did not run on a scene with lists above 1024"
    for r in (scored, plain):
        r.rast.close()


def test_trainer_tail_behind_a_scored_forward(pkg):
    """tests/test_gpu_trainer.py::test_backward_with_the_tail_in_its_epilogue_equals_backward_then_tail's comparison, between a
    handle that scores every training view and one that does not."""
    W, H, n, deg, mode = 112, 80, 1000, 2, "rgb"
    s = pkg.synthetic.make_scene(n, W, H, deg, 77, sigma_px=5.0)
    cam = pkg.Camera(W, H, tuple(s.focal))
    R, O = pkg.rasterizer, pkg.optim
    target = dev(np.random.default_rng(3).uniform(0, 1, (H, W, 3)).astype(np.float32))
    s.means[::7, 2] = -1.0   # behind the camera: culled, zero gradient
    host = dict(points=s.means, features_dc=s.shs[:, :1].copy(), features_rest=s.shs[:, 1:].copy(),
                opacities=s.opacities_raw.reshape(-1, 1), scales=s.scales_raw, rotations=s.rotations)
    lrs = dict(points=1.6e-3, features_dc=2.5e-2, features_rest=2.5e-3, opacities=5e-2, scales=5e-3, rotations=1e-2)
    bg = (0.1, 0.2, 0.3)

    def make():
        raw = {k: dev(np.ascontiguousarray(v)) for k, v in host.items()}
        opts = {k: O.Adam(raw[k], lrs[k], eps=1e-15) for k in O.GROUPS}
        act = list(R.prologue_forward(raw["features_dc"], raw["features_rest"], raw["opacities"], raw["scales"]))
        return raw, opts, act, R.GaussianRasterizer(W, H, mode=mode)

    raw_a, opt_a, act_a, rast_a = make()   # plain forwards
    raw_b, opt_b, act_b, rast_b = make()   # scored forwards
    sc = pkg.contribution.ContributionScores(n, "cuda")
    for step in range(1, 3):
        img_a = rast_a.forward_raw(raw_a["points"], *act_a, raw_a["rotations"], cam, deg, bg)
        img_b = rast_b.forward_raw(raw_b["points"], *act_b, raw_b["rotations"], cam, deg, bg, scores=sc)
        assert torch.equal(img_a, img_b), step
        vp = (img_a - target) * (2.0 / img_a.numel())
        vp_b = vp.clone()
        O.fused_backward_tail_step(rast_a, vp, opt_a, raw_a, *act_a, cam, deg, bg, forward_generation=rast_a.stats.generation)
        O.fused_backward_tail_step(rast_b, vp_b, opt_b, raw_b, *act_b, cam, deg, bg, forward_generation=rast_b.stats.generation)
        torch.cuda.synchronize()
        for k in O.GROUPS:
            assert torch.equal(raw_a[k], raw_b[k]), (k, step)
            assert torch.equal(opt_a[k].mu, opt_b[k].mu) and torch.equal(opt_a[k].nu, opt_b[k].nu), (k, step)
            assert opt_b[k].current_step == step
        for x, y in zip(act_a, act_b):
            assert torch.equal(x, y), step
        assert torch.equal(rast_a.gstate.grad_means_2d, rast_b.gstate.grad_means_2d), step
    assert sc.n_views == 2 and int(sc.hits.sum()) > 0
    assert not torch.equal(raw_b["points"], dev(host["points"]))   # it did train
    for r in (rast_a, rast_b):
        r.close()


def test_generations_drop_and_forward_only_behind_a_scored_forward(pkg):
    L = pkg._lib
    defn = dr.definition(pkg, "sweep-3")
    fs = defn.fs
    run = hip_run(pkg, defn, True)
    vp = np.zeros((fs.cam.height, fs.cam.width, fs.channels), np.float32)
    sc = new_scores(pkg, run)

    def backward(gen=0):
        out = run.rast.backward_raw(dev(vp), *run.t, run.camera, run.deg, run.bg, forward_generation=gen)
        torch.cuda.synchronize()
        return out

    def refused(word, gen=0):
        with pytest.raises(L.GsrError) as e:
            backward(gen)
        assert e.value.code == L.GSR_E_STATE and word in str(e.value), str(e.value)
        return str(e.value)

    run.forward()
    plain_gen = int(run.rast.stats.generation)
    score(run, sc)
    assert int(run.rast.stats.generation) == plain_gen + 1, "a scored forward is a forward: it advances the generation"
    # a fresh handle's two PLAIN forwards carry the same two generations: the same call gets the same refusal, word for word
    other = hip_run(pkg, defn, True)
    other.forward()
    assert int(other.rast.stats.generation) == plain_gen
    other.forward()
    with pytest.raises(L.GsrError) as e:
        other.rast.backward_raw(dev(vp), *other.t, other.camera, other.deg, other.bg, forward_generation=plain_gen)
    assert e.value.code == L.GSR_E_STATE
    assert refused("", plain_gen) == str(e.value)
    backward(plain_gen + 1)                     # the scored forward's own generation is accepted
    # gsr_drop_forward behind a scored forward
    score(run, sc)
    L.check(L.load().gsr_drop_forward(run.rast._h))
    refused("gsr_drop_forward")
    # a scored forward-only view keeps no backward state, like an unscored one
    score(run, sc, forward_only=True)
    assert sc.n_views == 3
    refused("FORWARD_ONLY")
    score(run, sc)
    backward()
    for r in (run, other):
        r.rast.close()


# ---- the other handle features ----
@pytest.mark.parametrize("name", ["sweep-3", "single-tile"])
def test_antialiased_handle_scores_the_effective_opacities(pkg, name):
    defn = dr.definition(pkg, name)
    fs = defn.fs
    means, shs, opac, scales, rots = (np.array(a) for a in (fs.means, fs.shs, fs.opac, fs.scales, fs.rots))
    opac = np.asarray(opac, np.float32).reshape(-1)
    d_eff = None
    for exact in (True, False):
        aa = ta.AARun(pkg, means, shs, opac, scales, rots, fs.cam, fs.deg, fs.bg, fs.mode, exact_tile_cull=exact)
        sa = new_scores(pkg, aa)
        score(aa, sa)
        rho, radii = ta.rho_of(aa)
        assert np.array_equal(radii, defn.d.radii), "radii do not change under antialiasing"
        assert (rho[radii > 0] <= 1).all() and (rho[radii > 0] >= 0).all() and (rho[radii > 0] < 1).any()
        o_eff = (opac * rho).astype(np.float32)
        plain = HipRun(pkg, means, shs, o_eff, scales, rots, fs.cam, fs.deg, fs.bg, fs.mode, exact_tile_cull=exact)
        sp = new_scores(pkg, plain)
        score(plain, sp)
        assert same(sa, sp), "an antialiased handle scores the plain render of o · rho"
        assert int(sa.hits.sum()) > 0
        # ... which lies inside the intervals of the definition of the scene with that opacity (the same lists: the filter and
        # the radii read no opacity)
        if d_eff is None:
            d_eff = dr.define(dataclasses.replace(fs, opac=o_eff.reshape(np.asarray(fs.opac).shape)))
            assert not d_eff.d.fragile_gaussian.any() and np.array_equal(d_eff.tl.values_sorted, defn.tl.values_sorted)
            iv = sr.intervals(d_eff)
            sr.conditions(iv, f"{name}, o · rho")
        m = sr.check_scores(iv, *arrays(sa))
        print(f"antialiased {name} ({'default' if exact else 'reference lists'}): hits {int(sa.hits.sum())} in [{int(iv.hits_lo.sum())}, "
              f"{int(iv.hits_hi.sum())}], worst |max_weight - definition| {m['worst_max_weight']:.3g}")
        for r in (aa, plain):
            r.rast.close()


def test_antialiased_edge_rows_stay_unscored(pkg):
    """The edge scene of tests/test_gpu_antialias.py::test_edge_rows: Gaussians 0 .. 17 (rho == 0, o · rho < 1/255, rho ~ 1e-19)
    emit nothing and keep all three words 0 on an antialiased handle; Gaussian 256, the lone thread of the second workgroup, is hit."""
    sc = ta.edge_scene()
    aa = ta.AARun(pkg, *sc.arrays, sc.cam, sc.deg, sc.bg, sc.mode, exact_tile_cull=True, radius_clip=2)
    scores = new_scores(pkg, aa)
    for view in range(2):
        score(aa, scores)
        assert not scores.hits[:18].any() and not scores.bits[:18].any() and not scores.q[:18].any(), view
        assert int(scores.hits[256]) > 0 and int(scores.bits[256]) > 0 and int(scores.q[256]) > 0
        culled = aa.rast.radii <= 0
        assert bool(culled.any()) and not scores.hits[culled].any()
    aa.rast.close()


def test_device_side_pose_scores_what_the_host_pose_does(pkg):
    defn = dr.definition(pkg, "ragged")          # an arbitrary pose (synthetic.view_pose(2)), :rgbdn
    host, devp = hip_run(pkg, defn, True), hip_run(pkg, defn, True, pose_dev=True)
    assert devp.Rd is not None
    for view in range(2):
        a, b = new_scores(pkg, host), new_scores(pkg, devp)
        ia, ib = score(host, a).clone(), score(devp, b).clone()
        assert torch.equal(ia, ib) and same(a, b), view
        assert int(a.hits.sum()) > 0
    for r in (host, devp):
        r.rast.close()
