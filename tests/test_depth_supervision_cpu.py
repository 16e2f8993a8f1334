"""Anchored depth supervision without a GPU: the reference's own tests of the anchor fits (test/runtests.jl:326-452)
re-expressed on the numpy host code, `fit_depth_anchors` on a synthetic cloud, and the restatement of the loss
(depth_torch.py) against finite differences and the reference's one-sided sky test."""
import numpy as np
import pytest
import torch

import depth_torch as dt

f32 = np.float32


@pytest.fixture(scope="module")
def DS(pkg):
    return pkg.depth_supervision


def test_ls_affine_fit(DS):
    ts = np.arange(1, 101, dtype=f32)
    a, b = DS.ls_affine_fit(ts, 2 * ts + 3)
    assert abs(a - 2) <= 1e-3 and abs(b - 3) <= 1e-3
    a, b = DS.ls_affine_fit(np.full(100, 5, f32), np.full(100, 7, f32))   # zero variance: the ridge gives a flat fit
    assert abs(a) <= 1e-4 and abs(b - 7) <= 1e-4


def test_ransac_affine_fit(DS):
    ts = np.arange(1, 1001, dtype=f32)
    f = DS.ransac_affine_fit(ts, 2 * ts + 3, rng=np.random.default_rng(0))
    assert abs(f.a - 2) <= 1e-3 and abs(f.b - 3) <= 1e-3 and abs(f.corr - 1) <= 1e-3 and abs(f.inlier_fraction - 1) <= 1e-3
    assert f.usable
    # the support bracket: quantiles, so a stray inlier cannot stretch it
    assert abs(f.t_lo - np.quantile(ts, 0.02)) <= 1 and abs(f.t_hi - np.quantile(ts, 0.98)) <= 1
    # 25 % gross outliers
    r = np.random.default_rng(0)
    ys = 2 * ts + 3
    ys[::4] = r.random(250, dtype=f32) * 3000 - 1000
    f = DS.ransac_affine_fit(ts, ys, rng=np.random.default_rng(1))
    assert abs(f.a - 2) <= 1e-1 and f.corr > 0.8 and f.inlier_fraction > 0.6 and f.usable
    # pure noise: rejected by the correlation gate
    f = DS.ransac_affine_fit(ts, np.random.default_rng(1).random(1000, dtype=f32), rng=np.random.default_rng(2))
    assert abs(f.corr) < 0.35 and not f.usable
    # fewer than 256 samples are never usable
    small = np.arange(1, 101, dtype=f32)
    assert not DS.ransac_affine_fit(small, 2 * small + 3, rng=np.random.default_rng(3)).usable
    # the draws are the caller's: the same generator state gives the same fit
    assert DS.ransac_affine_fit(ts, ys, rng=np.random.default_rng(5)) == DS.ransac_affine_fit(ts, ys, rng=np.random.default_rng(5))


def test_depth_anchor_extrapolation(DS):
    a, b, fl, disp = 1.0, 0.05, 0.1, 1.0
    an = DS.DepthAnchor.from_support(a, b, fl, disp, 0.3, 0.9)
    assert np.isclose(an.p_far, an.target(0.3)) and an.p_far < an.target(0.9)
    flipped = DS.DepthAnchor.from_support(-a, 1.0, fl, disp, 0.3, 0.9)   # a negative slope flips which end is far
    assert np.isclose(flipped.p_far, flipped.target(0.9))
    assert DS.DepthAnchor.from_support(a, b, fl, disp, 0.0, 0.0).p_far == 0
    flat = DS.DepthAnchor.from_support(a, b, fl, disp, 0.5, 0.5)
    assert flat.p_far == 0
    # the depth model: the far end is the larger affine value
    dep = DS.DepthAnchor.from_support(2.0, 1.0, fl, 0.0, 0.3, 0.9)
    assert np.isclose(dep.p_far, 1.0 / (2.0 * 0.9 + 1.0 + fl)) and np.isclose(dep.p_far, dep.target(0.9))
    # the restatement agrees with the host code on p_far, and flags only the sky pixel of the reference's prior
    assert f32(an.p_far) == dt.anchor_p_far(a, b, fl, disp, 0.3, 0.9)
    none = dt.depth_target(dt.Anchor(a, b, fl, disp, flat.p_far), np.array([[0.5, 0.005]], f32), dt.QSTEP)
    assert not none[3].any()
    ran, prior, _ = dt.reference_2x2()
    target, half, valid, far = dt.depth_target(ran, prior, dt.QSTEP)
    assert valid.all() and np.array_equal(far, np.array([[0, 0], [0, 1]], bool))
    assert np.isfinite(1 / target[1, 1] - ran.floor)
    assert np.array_equal(half, np.full((2, 2), f32(0.5) * f32(dt.QSTEP) * f32(1), f32))


def _sky_loss(z, far_on, dtype=torch.float64):
    an, prior, on_target = dt.reference_2x2()
    target, half, valid, far = dt.depth_target(an, prior, dt.QSTEP)
    if not far_on:
        far = np.zeros_like(far)
    D = torch.tensor(on_target.astype(np.float64), dtype=dtype)
    zt = torch.tensor(float(z), dtype=dtype, requires_grad=True)
    sel = torch.tensor([[0.0, 0.0], [0.0, 1.0]], dtype=dtype)
    loss, _ = dt.ssi_depth_loss(D * (1 - sel) + zt * sel, torch.ones(2, 2, dtype=dtype), target, half, valid, far, an.floor)
    loss.backward()
    return float(loss.detach()), float(zt.grad)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_one_sided_sky_supervision(dtype):
    _, _, on_target = dt.reference_2x2()
    sky_z = float(on_target[1, 1])
    loss, grad = _sky_loss(2.0, True, dtype)             # nearer than the extrapolated target: penalised, pushed away
    assert loss > 0 and grad < 0
    loss, grad = _sky_loss(10 * sky_z, True, dtype)      # farther: free
    assert abs(loss) <= 1e-8 and grad == 0
    loss, grad = _sky_loss(10 * sky_z, False, dtype)     # without the flag it is pulled back onto the extrapolation
    assert loss > 0 and grad > 0


def test_depth_weight(DS):
    assert DS.depth_weight(0) == 2.0
    assert np.isclose(DS.depth_weight(30000), 0.04) and np.isclose(DS.depth_weight(10 ** 6), 0.04)
    assert np.isclose(DS.depth_weight(15000), 2.0 * 0.02 ** 0.5, rtol=1e-6)
    assert DS.depth_weight(-5) == 2.0
    assert DS.depth_weight(15000) == float(f32(2.0) * np.power(f32(0.02), f32(0.5), dtype=f32))


def _cloud(pkg, DS):
    """3072 points on the plane z = 4 + 0.5x + 0.3y, one on each pixel-centre ray of the (shared) camera pose; the
    exact-disparity prior of that pose needs the floor fit_depth_anchors will use: 5 % of the median sample depth."""
    W, H, f = 64, 48, 40.0
    cam = pkg.Camera(W, H, (f, f))
    rx = (np.arange(W) + 0.5 - 0.5 * W) / f
    ry = (np.arange(H) + 0.5 - 0.5 * H) / f
    z = 4.0 / (1.0 - 0.5 * rx[None, :] - 0.3 * ry[:, None])
    pts = np.stack([rx[None, :] * z, ry[:, None] * z, z], -1).reshape(-1, 3).astype(f32)
    lo, hi = DS.robust_aabb(pts)
    ts, zs = DS.collect_anchor_samples(pts, cam, np.ones((H, W), f32), lo, hi)
    assert ts.size > 2500 and np.all(ts == 1)
    # every sample's depth is the depth of the pixel it fell into (to the rounding of the projection)
    floor = max(f32(1e-8), f32(0.05) * f32(np.median(zs)))
    return cam, pts, z.astype(f32), floor


def test_fit_depth_anchors_on_a_synthetic_cloud(pkg, DS):
    cam, pts, z, floor = _cloud(pkg, DS)
    disp = f32(1) / (z + floor)
    truth = [(0.05, 0.02), (0.04, 0.03), (0.08, 0.01), (0.05, 0.02)]
    priors = [((disp - f32(b)) / f32(a)).astype(f32) for a, b in truth]
    priors.append((f32(8) - priors[0]).astype(f32))                  # a flipped slope: outvoted
    priors.append(np.full_like(disp, 0.5))                            # a constant prior: no signal
    priors.append(None)                                               # a camera without a prior
    anchors = DS.fit_depth_anchors(pts, [cam] * len(priors), priors, mode="ssi", rng=np.random.default_rng(0))
    assert [a is None for a in anchors] == [False] * 4 + [True] * 3
    for an, (a, b) in zip(anchors, truth):
        assert an.disparity == 1.0                                    # the mode vote: the priors are affine in disparity
        assert an.floor == float(floor)
        assert abs(an.a / a - 1) <= 1e-3 and abs(an.b - b) <= 1e-3
        assert disp.min() < an.p_far < np.quantile(disp, 0.1)        # the 2 % quantile of the support, not its extreme
    # forced modes; the flipped camera alone keeps its (negative) slope
    dep = DS.fit_depth_anchors(pts, [cam] * 2, [z * f32(2) + f32(1)] * 2, mode="ssi_depth", rng=np.random.default_rng(0))
    assert all(a is not None and a.disparity == 0.0 and abs(a.a - 0.5) <= 1e-3 and abs(a.b + 0.5) <= 1e-3 for a in dep)
    alone = DS.fit_depth_anchors(pts, [cam], [priors[4]], mode="ssi_disparity", rng=np.random.default_rng(0))
    assert alone[0] is not None and alone[0].a < 0
    with pytest.raises(ValueError, match="Invalid depth loss mode"):
        DS.fit_depth_anchors(pts, [cam], [priors[0]], mode="l1")


def _gradcheck_frame():
    """5 x 4 (W x H) with every branch: invalid priors, far_extrap nearer and farther, residuals inside and outside the
    deadband, alpha < 1e-3 — and nothing within 1e-4 of a kink (the finite differences step by 1e-6)."""
    an = dt.DISPARITY
    H, W = 4, 5
    e = np.array([[4.5, 4.7, 5.0, 5.2, 3.0],
                  [4.6, 4.8, 5.1, 5.3, 500.0],
                  [4.7, 4.9, 5.2, 5.4, 5.6],
                  [4.8, 5.0, 5.3, 5.5, 5.7]])
    t = ((1.0 / (e + dt.FLOOR) - float(an.b)) / float(an.a)).astype(f32)
    t[0, 4] = t[1, 4] = 0.005          # sky: rendered nearer (3.0) and farther (500) than its target
    e_r = e.copy()
    e_r[0, :3] *= 1.0004               # inside the deadband (half = 7.8e-4 in p; this moves p by about 7e-5)
    e_r[1, :3] *= 1.02                 # outside
    e_r[2, 1:4] *= 0.97
    t[3, 0] = -0.2                     # invalid
    t[3, 1] = np.nan
    alpha = np.full((H, W), 0.8)
    alpha[2, 0] = 5e-4                 # below the weight threshold
    alpha[0, 1] = alpha[1, 1] = 1.0
    alpha[3, 3] = 0.3
    return an, t, e_r * alpha, alpha


def test_restatement_against_finite_differences():
    an, prior, D, A = _gradcheck_frame()
    target, half, valid, far = dt.depth_target(an, prior, dt.QSTEP)
    D0, A0 = torch.tensor(D), torch.tensor(A)
    _, info = dt.ssi_depth_loss(D0, A0, target, half, valid, far, an.floor)
    w, r = info["w"], np.abs(info["p"] - info["target"]) - info["band"]
    live = w > 0
    assert (~valid).any() and (live & info["far"]).sum() == 2 and (valid & ~live).any()
    assert (live & ~info["far"] & (r < -1e-4)).any() and (live & ~info["far"] & (r > 1e-4)).any()
    assert not (live & (np.abs(r) < 1e-4)).any()
    sky = info["p"] - info["target"]
    assert sky[0, 4] > 1e-3 and sky[1, 4] < -1e-3
    fn = lambda d, a: dt.ssi_depth_loss(d, a, target, half, valid, far, an.floor, 1.0, frozen=(D0, A0))[0]  # noqa: E731
    d = D0.clone().requires_grad_(True)
    a = A0.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(fn, (d, a), eps=1e-7, atol=1e-9, rtol=1e-5)
    # the frozen statistics are the detached ones: same loss, same gradient
    l0, _ = dt.ssi_depth_loss(d, a, target, half, valid, far, an.floor)
    l1 = fn(d, a)
    assert float(l0.detach()) == float(l1.detach())
    g0 = torch.autograd.grad(l0, (d, a))
    g1 = torch.autograd.grad(l1, (d, a))
    assert all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert g0[0][1, 4] == 0 and g0[0][0, 4] != 0 and g0[0][3, 0] == 0 and g0[1][2, 0] == 0


@pytest.mark.parametrize("model", ["disparity", "depth"])
def test_frame_family_populates_every_branch(model):
    an = dt.ANCHORS[model]
    frame, prior = dt.make_frame(97, 61, 5, model, seed=3)
    ref = dt.evaluate(frame, prior, an, dt.QSTEP)
    live = ref["w"] > 0
    assert 0.3 <= ref["valid"].mean() <= 0.9
    r = ref["p"] - ref["target"]
    assert (ref["far"] & (r > ref["band"])).sum() > 20 and (ref["far"] & (r < -ref["band"])).sum() > 20
    two = live & ~ref["far"]
    assert (two & (np.abs(r) < ref["band"])).sum() > 100 and (two & (np.abs(r) > ref["band"])).sum() > 100
    assert np.isnan(prior).any() and (prior <= 0).any() and (frame[..., 4] == 0).any() and (frame[..., 4] == 1).any()
    assert ref["loss"] > 0 and np.abs(ref["vimage"][..., 3]).max() > 0 and np.abs(ref["vimage"][..., 4]).max() > 0
    assert not ref["vimage"][..., :3].any()
    # NaN / Inf at w = 0 pixels cost nothing (the intended deviation)
    bad, bad_prior = frame.copy(), prior.copy()
    dead = np.argwhere(~live)
    bad[tuple(dead[0])][3] = np.nan
    bad[tuple(dead[1])][3] = np.inf
    bad[tuple(np.argwhere(frame[..., 4] == 0)[0])][4] = np.nan        # alpha was 0: a non-finite alpha counts as 0
    bad_prior[tuple(np.argwhere(~live & (frame[..., 4] > 0.5))[0])] = np.inf
    again = dt.evaluate(bad, bad_prior, an, dt.QSTEP)
    assert np.isfinite(again["loss"]) and np.isfinite(again["vimage"]).all()
    assert abs(again["loss"] - ref["loss"]) <= 1e-12 * ref["loss"]
