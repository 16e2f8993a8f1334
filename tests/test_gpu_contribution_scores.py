"""-m gpu: the per-Gaussian contribution scores of gsr_forward_scored (include/gsr.h) and pruning by them.

  against the definition   every scene of scores_ref.SCENES (one per mode, exact depth ties, lists above the 1024 and the 4096 sort
                           tier), default handle and reference lists, two views on one handle into separate sets: each inside the
                           per-Gaussian intervals of tests/scores_ref.py (so hits == lo exactly where hi == lo);
  path independence        torch.equal on all three arrays against the default handle's: reference lists, direct / aggregating /
                           compact binning, forward-only, covisibility + uncertainty in the same call, a second run; the deep scenes
                           must have taken the tier walk, the small ones not;
  accumulation             view A then view B into one set == (max, +, +) of the two single-view sets; pre-filled arrays are
                           accumulated into; NULL members leave the others' results alone; culled Gaussians are untouched;
  identities               hits == 0 <=> max_weight == 0 <=> weight_sum == 0; covisible => hit; sum of weight_sum against the sum of
                           uncertainties; image, final_T and n_contrib bit-identical to the unscored forward's;
  mask and prune           gsr_contribution_mask against numpy at and around stored values; prune_by_contribution end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

import definition_ref as dr
import scores_ref as sr
from hip_helpers import dev
from test_gpu_definition import CELLS, hip_run
from test_gpu_preprocess_forms import form

pytestmark = pytest.mark.gpu


def new_scores(pkg, run):
    return pkg.contribution.ContributionScores(int(run.t[0].shape[0]), "cuda")


def score(run, sc, camera=None, forward_only=False, covis=None, unc=None):
    img = run.rast.forward_raw(*run.t, camera or run.camera, run.deg, run.bg, run.Rd, run.td, covis, unc, forward_only=forward_only,
                               scores=sc)
    torch.cuda.synchronize()
    return img


def arrays(sc):
    return sc.bits.cpu().numpy().view(np.uint32), sc.hits.cpu().numpy(), sc.q.cpu().numpy()


def same(a, b):
    return torch.equal(a.bits, b.bits) and torch.equal(a.hits, b.hits) and torch.equal(a.q, b.q)


class Partial:
    """A score set with some members NULL, as forward_raw takes one."""

    def __init__(self, pkg, sc, max_weight=True, hits=True, weight_sum=True):
        self.L, self.sc, self.keep, self.n_views = pkg._lib, sc, (max_weight, hits, weight_sum), 0

    def as_struct(self, n, device):
        s = self.sc.as_struct(n, device)
        for on, k in zip(self.keep, ("max_weight", "hits", "weight_sum")):
            if not on:
                setattr(s, k, None)
        return s


_base = {}


def base_scores(pkg, name):
    """The default handle's scores of one view of the scene (and its stats): once per scene, shared, never written again."""
    if name not in _base:
        run = hip_run(pkg, dr.definition(pkg, name), True)
        sc = new_scores(pkg, run)
        score(run, sc)
        _base[name] = (sc, tuple(int(t) for t in run.rast.stats.tier_tiles), int(run.rast.stats.compact_binning))
        run.rast.close()
    return _base[name]


@pytest.mark.parametrize("exact", [True, False], ids=["default", "reference-lists"])
@pytest.mark.parametrize("name", sr.SCENES)
def test_scores_lie_inside_the_definitions_intervals(pkg, name, exact):
    defn, iv = dr.definition(pkg, name), sr.scene_intervals(pkg, name)
    run = hip_run(pkg, defn, exact)
    sets = [new_scores(pkg, run), new_scores(pkg, run)]
    for view, sc in enumerate(sets):
        score(run, sc)
        m = sr.check_scores(iv, *arrays(sc))
        print(f"{name} ({defn.fs.mode}, {'default' if exact else 'reference lists'}, view {view}): worst |max_weight - definition| "
              f"{m['worst_max_weight']:.3g}, worst |weight_sum - definition| / hits {m['worst_weight_sum_per_hit']:.3g} over "
              f"{m['exact']} Gaussians with exact hits; hits {int(sc.hits.sum())} in [{int(iv.hits_lo.sum())}, {int(iv.hits_hi.sum())}]")
        assert sc.n_views == 1
    assert same(*sets)
    run.rast.close()


@pytest.mark.parametrize("name", sr.SCENES)
def test_scores_do_not_depend_on_the_path(pkg, name):
    defn = dr.definition(pkg, name)
    base, tiers, compact = base_scores(pkg, name)
    assert int(base.hits.sum()) > 0 and compact == 0
    if name in dr.DEEP:
        assert sum(tiers) > 0, "the tier walk did not run on a scene with lists above 1024"
    else:
        assert sum(tiers) == 0, tiers
    for cell, (f, budget) in CELLS.items():
        for exact in (True, False):
            with form(pkg, f):
                run = hip_run(pkg, defn, exact, budget)
                sc = new_scores(pkg, run)
                score(run, sc)
                if budget:
                    assert int(run.rast.stats.compact_binning) == 1, "the forced compact mode did not run"
                assert same(sc, base), (name, cell, exact)
                run.rast.close()
    run = hip_run(pkg, defn, True, want_covis=True, want_uncert=True)
    only, side, again = new_scores(pkg, run), new_scores(pkg, run), new_scores(pkg, run)
    score(run, only, forward_only=True)
    assert same(only, base), "forward-only"
    score(run, side, covis=run.covis, unc=run.unc)
    assert same(side, base), "with covisibility and uncertainty in the same call"
    score(run, again, forward_only=True, covis=run.covis, unc=run.unc)
    assert same(again, base), "a later run, forward-only with side outputs"
    run.rast.close()


def shifted(pkg, run):
    c = run.camera
    return pkg.Camera(c.width, c.height, tuple(c.focal), tuple(c.principal), np.asarray(c.R),
                      (np.asarray(c.t, np.float32) + np.float32([0.21, -0.13, 0.4])).astype(np.float32))


@pytest.mark.parametrize("name", ["sweep-3", "ragged", "deep-276"])
def test_accumulation_null_members_and_culled_rows(pkg, name):
    defn = dr.definition(pkg, name)
    run = hip_run(pkg, defn, True)
    cam_b = shifted(pkg, run)
    a, b, ab = new_scores(pkg, run), new_scores(pkg, run), new_scores(pkg, run)
    score(run, a)
    radii_a = run.rast.radii.clone()
    score(run, b, camera=cam_b)
    radii_b = run.rast.radii.clone()
    assert not same(a, b) and int(b.hits.sum()) > 0, "view B must differ from view A"
    score(run, ab)
    score(run, ab, camera=cam_b)
    assert ab.n_views == 2
    assert torch.equal(ab.bits, torch.maximum(a.bits, b.bits))      # bits of non-negative floats: integer order
    assert torch.equal(ab.hits, a.hits + b.hits) and torch.equal(ab.q, a.q + b.q)
    for sc, radii in ((a, radii_a), (b, radii_b)):
        culled = radii <= 0
        assert not sc.hits[culled].any() and not sc.bits[culled].any() and not sc.q[culled].any()
    # accumulated into, never cleared: pre-filled words
    pre = new_scores(pkg, run)
    half = int(np.float32(0.5).view(np.int32))
    pre.bits.fill_(half); pre.hits.fill_(5); pre.q.fill_(7)
    score(run, pre)
    assert torch.equal(pre.bits, torch.clamp(a.bits, min=half)) and torch.equal(pre.hits, a.hits + 5) and torch.equal(pre.q, a.q + 7)
    # NULL members: the others get what they get in a full set, the NULL ones' arrays are not touched
    for keep in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        part = new_scores(pkg, run)
        part.bits.fill_(-1); part.hits.fill_(-1); part.q.fill_(-1)
        for on, t in zip(keep, (part.bits, part.hits, part.q)):
            if on:
                t.zero_()
        score(run, Partial(pkg, part, *keep))
        for on, got, want in zip(keep, (part.bits, part.hits, part.q), (a.bits, a.hits, a.q)):
            assert torch.equal(got, want if on else torch.full_like(got, -1)), keep
    # every member NULL: the plain forward
    img = score(run, Partial(pkg, new_scores(pkg, run), False, False, False)).clone()
    assert torch.equal(img, run.forward())
    run.rast.close()


@pytest.mark.parametrize("name", ["sweep-3", "single-tile", "ragged", "deep-5911"])
def test_identities_and_unchanged_outputs(pkg, name):
    defn = dr.definition(pkg, name)
    run = hip_run(pkg, defn, True, want_covis=True, want_uncert=True)
    plain = run.forward().clone()
    T, nc, unc0, cov0 = run.rast.accum_alpha.clone(), run.rast.n_contrib.clone(), run.unc.clone(), run.covis.clone()
    run.covis.zero_()
    sc = new_scores(pkg, run)
    img = score(run, sc, covis=run.covis, unc=run.unc)
    assert torch.equal(img, plain) and torch.equal(run.rast.accum_alpha, T) and torch.equal(run.rast.n_contrib, nc)
    assert torch.equal(run.unc, unc0) and torch.equal(run.covis, cov0)
    zero = sc.hits == 0
    assert torch.equal(zero, sc.bits == 0) and torch.equal(zero, sc.q == 0)
    # w = alpha T with alpha >= 1/255 and T >= 1e-4 (T' = T (1 - alpha) did not stop the pixel), up to the hardware exp's rounding
    assert (sc.max_weight[~zero] >= (1.0 - dr.BLEND_MARGIN) * 1e-4 / 255.0).all() and (sc.max_weight <= 0.99).all()
    assert (sc.q[~zero] >= 6 * sc.hits[~zero]).all() and (sc.weight_sum <= sc.hits.double() * sc.max_weight.double() + 2.0 ** -25 * sc.hits).all()
    assert (sc.hits[run.covis.bool()] > 0).all()
    pixels = run.unc.numel()
    total_g, total_p = float(sc.weight_sum.sum()), float(run.unc.double().sum())
    print(f"{name}: sum of weight_sum {total_g:.6f}, sum of uncertainties {total_p:.6f}, pixels {pixels}")
    assert abs(total_g - total_p) <= 1e-4 * pixels
    assert int(sc.hits.sum()) <= int((run.rast.n_contrib.long()).sum())   # a pixel blends at most the entries up to its last one
    run.rast.close()


def test_contribution_mask_against_numpy(pkg):
    K, L = pkg.contribution, pkg._lib
    rng = np.random.default_rng(2207)
    n = 1000
    sc = K.ContributionScores(n, "cuda")
    w = rng.uniform(0.0, 0.99, n).astype(np.float32)
    w[::7] = 0.0
    w[3], w[4] = np.float32(0.01), np.nextafter(np.float32(0.01), np.float32(0))
    w[5] = np.nextafter(np.float32(0.01), np.float32(1))
    hits = rng.integers(0, 50, n).astype(np.int64)
    hits[11] = (1 << 40) + 3
    q = rng.integers(0, 1 << 30, n).astype(np.int64)
    q[12], q[13], q[14] = (1 << 24) * 3, (1 << 24) * 3 - 1, (1 << 24) * 3 + 1
    q[15] = (1 << 45) + 1
    sc.bits.copy_(torch.from_numpy(w.view(np.int32))); sc.hits.copy_(torch.from_numpy(hits)); sc.q.copy_(torch.from_numpy(q))
    wb = w.view(np.uint32).astype(np.uint64)
    for thr in (0.01, 0.0, 0.5, float(np.nextafter(np.float32(0.01), np.float32(1))), 0.99, 1.5):
        want = wb >= np.float32(thr).view(np.uint32)
        assert np.array_equal(K.prune_mask(sc, "max_weight", thr).cpu().numpy().astype(bool), want), thr
        assert np.array_equal(want, w >= np.float32(thr))
    for thr in (3.0, 3.0 - 2.0 ** -24, 3.0 + 2.0 ** -24, 3.0 + 2.0 ** -25, 0.0, 1e-9, 2.0 ** 21):
        want = q >= int(np.ceil(thr * 2.0 ** 24))
        assert np.array_equal(K.prune_mask(sc, "weight_sum", thr).cpu().numpy().astype(bool), want), thr
    for thr in (0, 1, 0.5, 1.5, 7, 49, 50, float(1 << 40), float((1 << 40) + 3), float((1 << 40) + 4)):
        want = hits >= int(np.ceil(thr))
        assert np.array_equal(K.prune_mask(sc, "hits", thr).cpu().numpy().astype(bool), want), thr
    # only the rule's own array is read
    lib = L.load()
    valid = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.gsr_contribution_mask(n, L.SCORE_HITS, 7.0, None, sc.hits.data_ptr(), None, valid.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(valid.cpu().numpy().astype(bool), hits >= 7)


def test_prune_by_contribution_end_to_end(pkg):
    K, Dn, O, R = pkg.contribution, pkg.densification, pkg.optim, pkg.rasterizer
    W, H, deg, n = 64, 48, 1, 300
    s = pkg.synthetic.make_scene(n, W, H, deg, 4107, sigma_px=3.0)
    # Gaussians no view can use, of the three kinds a trained model has: below the alpha threshold everywhere (sigmoid(-8) < 1/255),
    # outside every frustum, and hidden behind a front layer of large opaque splats (which makes stopping entries of them)
    s.opacities_raw[0:30] = -8.0
    s.means[30:50, 0] += 100.0
    s.means[50:80, 2] = 1.5
    s.means[50:80, :2] *= 1.5 / 12.0
    s.opacities_raw[50:80] = 8.0
    s.scales_raw[50:80] = np.log(0.25)
    gs = Dn.GaussianModel(dev(s.means), dev(s.shs[:, :1]), dev(s.shs[:, 1:]), dev(s.scales_raw), dev(s.rotations),
                          dev(s.opacities_raw.reshape(n, 1)))
    rng = np.random.default_rng(5)
    opt = {k: O.Adam(getattr(gs, k), 1e-3) for k in Dn.PARAMS}
    for k, a in opt.items():                       # recognisable moments: row r of every array carries r
        rows = getattr(gs, k).reshape(n, -1).shape[1]
        for m in (a.mu, a.nu):
            m.copy_(dev((np.arange(n, dtype=np.float32)[:, None] + rng.uniform(0, 0.5, (n, rows)).astype(np.float32)).reshape(-1)))
    strategy = Dn.DefaultStrategy(gs)
    strategy.max_radii.copy_(torch.arange(n, dtype=torch.int32, device="cuda"))
    cams = []
    for j in (1, 3, 6):
        Rm, t = pkg.synthetic.view_pose(j)
        cams.append(pkg.Camera(W, H, s.focal, (0.5, 0.5), Rm, t))
    bg = (0.2, 0.4, 0.1)
    rast = R.GaussianRasterizer(W, H, mode="rgb")

    def tensors():
        shs, oa, sa = R.prologue_forward(gs.features_dc, gs.features_rest, gs.opacities, gs.scales)
        return (gs.points, shs, oa, sa, gs.rotations)

    def renders(sc=None):
        out = []
        for cam in cams:
            img = rast.forward_raw(*tensors(), cam, deg, bg, forward_only=True, scores=sc).clone()
            out.append((img, rast.accum_alpha.clone()))
        return out

    before = renders()
    sc = K.score_views(rast, tensors(), cams, deg, bg)
    assert sc.n_views == 3
    valid = K.prune_mask(sc, "hits", 1).bool()
    assert torch.equal(valid, sc.hits >= 1)
    keep = valid.nonzero().flatten()
    assert 0 < keep.numel() < n, "the scene must have both used and unused Gaussians"
    old = {k: getattr(gs, k).clone() for k in Dn.PARAMS}
    old_m = {k: (a.mu.clone(), a.nu.clone()) for k, a in opt.items()}
    old_hits = sc.hits.clone()
    with pytest.raises(TypeError, match="MCMCStrategy"):
        K.prune_by_contribution(pkg.mcmc.MCMCStrategy(max_cap=n), gs, opt, sc, "hits", 1)
    removed = K.prune_by_contribution(strategy, gs, opt, sc, rule="hits", threshold=1)
    m = keep.numel()
    assert removed == n - m and len(gs) == m
    for k in Dn.PARAMS:
        assert torch.equal(getattr(gs, k), old[k][keep]), k
        rows = old[k].reshape(n, -1).shape[1]
        for got, was in zip((opt[k].mu, opt[k].nu), old_m[k]):
            assert torch.equal(got.reshape(m, rows), was.reshape(n, rows)[keep]), k
    assert torch.equal(strategy.max_radii, keep.to(torch.int32))
    # a never-blended Gaussian can only have been a pixel's stopping entry, with at most T <= 1e-4 / (1 - 0.99) left there
    fmax = max(1.0, float(max(img.abs().max() for img, _ in before)))
    bound = dr.T_MIN / (1.0 - dr.ALPHA_MAX) * max(fmax, max(abs(b) for b in bg))
    resc = K.ContributionScores(m, "cuda")
    after = renders(resc)
    identical = True
    for (i0, t0), (i1, t1) in zip(before, after):
        di, dT = float((i0 - i1).abs().max()), float((t0 - t1).abs().max())
        print(f"prune by hits: removed {removed} of {n}; max |image change| {di:.3g} (bound {bound:.3g}), max |final_T change| {dT:.3g}")
        assert di <= bound and dT <= dr.T_MIN / (1.0 - dr.ALPHA_MAX)
        identical = identical and torch.equal(i0, i1) and torch.equal(t0, t1)
    if identical:       # nothing that was blended was removed: the survivors are hit exactly as before
        assert torch.equal(resc.hits, old_hits[keep])
    else:
        assert (resc.hits >= old_hits[keep]).all()   # (a removed stopping entry lets the pixel blend on)
    rast.close()
