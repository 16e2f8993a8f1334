"""Geometry regularisation on the MI355X: the gsr_normal_loss_* / gsr_flatten_loss kernels against the float64 restatement
(geometry_ref.py), their determinism, and the :rgbdn training path end to end with the term on.

Accuracy bar of the depth-normal term (no tolerance fixed in advance): the YARDSTICK is the same formulation evaluated in
float32 by torch on the CPU (geometry_torch.py) against its float64 result, computed here per case; the GPU must be within
4x of that error (floor 1e-6 relative for the loss).  The tangents are differences of nearly equal depths, so the error
grows with the focal length; the factor covers another equally valid association of the same fp32 operations (reciprocals,
the reduction tree), not a wrong term, which is off by orders of magnitude."""
import os
import sys

import numpy as np
import pytest
import torch

import geometry_ref as gr
import geometry_torch as gt
import scenes
from hip_helpers import HipRun, compare_backward, dev, rel_l2

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHT = 0.05
GROUPS = (("depth", slice(3, 4)), ("alpha", slice(4, 5)), ("normal", slice(5, 8)))


@pytest.fixture(scope="module")
def G(pkg):
    return pkg.geometry_regularization


def _bits(t):
    return t.contiguous().view(torch.int32)


def _frame(W, H, f):
    if (W, H) in ((1920, 1080), (97, 61)):
        return gt.noisy_frame(W, H, f, seed=W + H)
    return gt.plane_frame(W, H, f, normals=(0.0, 0.0, -1.0))   # the exact plane against a fronto-parallel guess


def _run(G, pkg, img, f, vp0=None, scratch=None, weight=WEIGHT):
    H, W = img.shape[:2]
    cam = pkg.Camera(W, H, (f, f))
    ti = dev(img)
    loss, wmap, stats = G.depth_normal_loss(ti, cam, weight, weights=True, stats=True, scratch=scratch)
    vp = torch.zeros_like(ti) if vp0 is None else dev(vp0)
    G.depth_normal_loss_backward_(ti, cam, vp, weight, scratch=scratch)
    torch.cuda.synchronize()
    return loss, wmap, stats, vp


@pytest.mark.parametrize("W,H,f", [(1920, 1080, 1000.0), (97, 61, 100.0), (64, 48, 100.0), (3, 3, 100.0), (2, 5, 100.0)])
def test_depth_normal_vs_float64_and_determinism(G, pkg, W, H, f):
    img = _frame(W, H, f)
    ref = gr.depth_normal(img, (f, f), weight=WEIGHT)
    noisy = (W, H) in ((1920, 1080), (97, 61))
    if noisy:
        # conditions on the restatement alone: both branches exercised, and no centre near the two thresholds whose
        # decision depends on the association of an fp32 sum
        assert 0.3 <= ref["valid"].mean() <= 0.7
        assert not ((ref["nr_sq"] >= 0.0081) & (ref["nr_sq"] <= 0.0121)).any()
        assert not (ref["n_sq"] < 1e-20).any()
    nb = G.normal_loss_scratch_bytes(W, H)
    scratch = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    loss, wmap, stats, vp = _run(G, pkg, img, f, scratch=scratch)
    # the weight map bit for bit, no pixel left out; count equal
    assert tuple(wmap.shape) == (H, W)
    assert np.array_equal(wmap.cpu().numpy().view(np.uint32), ref["weights"].view(np.uint32))
    sum_w, count = (float(v) for v in stats.cpu().numpy())
    assert count == ref["count"]
    assert abs(sum_w - ref["sum_w"]) <= 1e-6 * max(ref["sum_w"], 1.0)
    v = vp.cpu().numpy().astype(np.float64)
    assert not v[..., :3].any()
    if ref["loss"] == 0.0:   # the gated views (3x3: one valid centre; 2x5: no interior)
        assert ref["count"] < 64 and loss.item() == 0.0 and not v.any()
    else:
        l64, g64, ok64, _, _ = gt.gradient(img, (f, f))
        l32, g32, ok32, _, _ = gt.gradient(img, (f, f), dtype=torch.float32)
        assert np.array_equal(ok64, ref["valid"]) and np.array_equal(ok32, ref["valid"])
        yard_loss = abs(l32 - l64) / abs(l64)
        err_loss = abs(loss.item() - ref["loss"]) / abs(ref["loss"])
        print(f"\n[{W}x{H} f={f:g}] valid {ref['valid'].mean():.3f} loss {loss.item():.9g} rel.err {err_loss:.3g} "
              f"(yardstick {yard_loss:.3g})")
        figures = []
        for name, ch in GROUPS:
            yard = gt.rel_l2(g32[..., ch], g64[..., ch])
            err = gt.rel_l2(v[..., ch], ref["vimage"][..., ch])
            figures.append((name, ch, err, yard))
            print(f"    grad {name}: rel.L2 err {err:.3g}, yardstick {yard:.3g}, ratio {err / yard:.2f}")
        assert err_loss <= max(4.0 * yard_loss, 1e-6)
        for name, ch, err, yard in figures:
            assert np.abs(ref["vimage"][..., ch]).max() > 0
            assert err <= 4.0 * yard, (name, err, yard)
    # determinism: a second run, and a run on poisoned scratch and output buffers, give the same bits
    loss2, wmap2, stats2, vp2 = _run(G, pkg, img, f, scratch=scratch)
    dirty = torch.full((max(nb, 4),), 0xFF, dtype=torch.uint8, device="cuda")
    loss3, wmap3, stats3, vp3 = _run(G, pkg, img, f, scratch=dirty)
    for a, b in ((loss, loss2), (loss, loss3), (wmap, wmap2), (wmap, wmap3), (stats, stats2), (stats, stats3), (vp, vp2), (vp, vp3)):
        assert torch.equal(_bits(a), _bits(b))
    # the backward ADDS: onto a non-zero buffer it gives buffer + gradient to the rounding of that one add, and leaves
    # channels 0..2 bit-unchanged
    r = np.random.default_rng(3)
    base = (r.standard_normal((H, W, 8)) * 1e-4).astype(np.float32)
    base[0, 0, 0] = np.nan   # a colour value the term must not even read-modify-write
    _, _, _, vp4 = _run(G, pkg, img, f, vp0=base, scratch=scratch)
    out = vp4.cpu().numpy()
    assert np.array_equal(out[..., :3].view(np.uint32), base[..., :3].view(np.uint32))
    expect = (base[..., 3:] + vp.cpu().numpy()[..., 3:]).astype(np.float32)   # one fp32 add
    assert np.array_equal(out[..., 3:].view(np.uint32), expect.view(np.uint32))


def test_nonfinite_values_at_invalid_centres_cost_nothing(G, pkg):
    W, H, f = 97, 61, 100.0
    clean = gt.noisy_frame(W, H, f, seed=11)
    clean[10:14, 10:14, 4] = 0.2            # transparent patches: their centres and their neighbours' are invalid
    clean[20:23, 30:33, 4] = 0.1
    bad = clean.copy()
    bad[11:13, 11:13, 3] = np.nan
    bad[11, 11, 4] = np.nan
    bad[12, 12, 5:8] = np.inf
    bad[21, 31, 3] = np.inf
    bad[21, 31, 5] = -np.inf
    ref = gr.depth_normal(bad, (f, f), weight=WEIGHT)
    assert np.array_equal(ref["vimage"], gr.depth_normal(clean, (f, f), weight=WEIGHT)["vimage"])
    loss_c, wmap_c, stats_c, vp_c = _run(G, pkg, clean, f)
    loss_b, wmap_b, stats_b, vp_b = _run(G, pkg, bad, f)
    assert np.isfinite(loss_b.item()) and torch.isfinite(vp_b).all().item()
    for a, b in ((loss_c, loss_b), (wmap_c, wmap_b), (stats_c, stats_b), (vp_c, vp_b)):
        assert torch.equal(_bits(a), _bits(b))
    assert np.array_equal(wmap_b.cpu().numpy().view(np.uint32), ref["weights"].view(np.uint32))
    l64, g64, _, _, _ = gt.gradient(clean, (f, f))
    l32, g32, _, _, _ = gt.gradient(clean, (f, f), dtype=torch.float32)
    assert abs(loss_b.item() - ref["loss"]) <= max(4.0 * abs(l32 - l64) / abs(l64), 1e-6) * abs(ref["loss"])
    v = vp_b.cpu().numpy().astype(np.float64)
    for name, ch in GROUPS:
        assert gt.rel_l2(v[..., ch], ref["vimage"][..., ch]) <= 4.0 * gt.rel_l2(g32[..., ch], g64[..., ch]), name


def test_autograd_form_and_refused_buffers(G, pkg):
    W, H, f = 64, 48, 100.0
    img = gt.plane_frame(W, H, f, normals=(0.0, 0.0, -1.0))
    cam = pkg.Camera(W, H, (f, f))
    ref = gr.depth_normal(img, (f, f), weight=1.0)
    t = dev(img).requires_grad_(True)
    loss = G.depth_normal_consistency_loss(t, cam)
    (2.0 * loss).backward()
    assert abs(loss.item() - ref["loss"]) <= 1e-5 * ref["loss"]
    assert rel_l2(t.grad.cpu().numpy(), 2.0 * ref["vimage"]) <= 1e-4
    # wrong-shaped caller buffers are refused before any launch, not overrun
    ti = dev(img)
    with pytest.raises(ValueError, match="vpixels must have"):
        G.depth_normal_loss_backward_(ti, cam, torch.zeros((H - 1, W, 8), device="cuda"))
    with pytest.raises(ValueError, match=":rgbdn frame"):
        G.depth_normal_loss_backward_(ti, cam, torch.zeros((H, W, 5), device="cuda"))
    with pytest.raises(ValueError, match=":rgbdn frame"):
        G.depth_normal_loss(torch.zeros((H, W, 5), device="cuda"), cam)
    with pytest.raises(ValueError, match="must not be the image"):
        G.depth_normal_loss_backward_(ti, cam, ti)
    with pytest.raises(ValueError, match="resolution"):
        G.depth_normal_loss(ti, pkg.Camera(W + 1, H, (f, f)))
    with pytest.raises(ValueError, match="scratch must be"):
        G.depth_normal_loss(ti, cam, scratch=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="vscales must be"):
        G.flatten_loss(torch.zeros((10, 3), device="cuda"), vscales=torch.zeros((9, 3), device="cuda"))
    with pytest.raises(ValueError, match="vscales must be"):
        G.flatten_loss(torch.zeros((10, 1), device="cuda"), vscales=torch.zeros((10, 1), device="cuda"))
    with pytest.raises(ValueError, match="scales must be"):
        G.flatten_loss(torch.zeros((10, 2), device="cuda"))


# ---- flatten loss ----

@pytest.mark.parametrize("n", [0, 1, 1000, 1_000_003])
@pytest.mark.parametrize("sd", [1, 3])
def test_flatten_loss_and_gradient(G, pkg, n, sd):
    """Bounds: the loss sums fp32 expf values (<= 2 ulp each) per 2048-Gaussian workgroup in a tree (<= 11 roundings) and the
    partials in double: 1e-6 relative.  The gradient is ONE fp32 add of the constant fl(weight / n): bit-exact."""
    weight = 0.005
    r = np.random.default_rng(n + sd)
    s = r.normal(-3.0, 1.0, (n, sd)).astype(np.float32)
    if n >= 1000 and sd == 3:
        s[::3, 1] = s[::3, 0]                       # ties: first-two, last-two, all three
        s[1::7, 2] = s[1::7, 1]
        s[5::11] = s[5::11, :1]
    ref_loss, _, g_act = gr.flatten(s, weight)
    ts = dev(s).reshape(n, sd)
    loss = G.flatten_loss(ts, weight)
    torch.cuda.synchronize()
    assert abs(loss.item() - ref_loss) <= 1e-6 * ref_loss
    # the gradient added onto a given ∇scales (N, 3)
    base = r.standard_normal((n, 3)).astype(np.float32)
    vs = dev(base).reshape(n, 3)
    dirty = torch.full((max(int(pkg._lib.load().gsr_flatten_loss_scratch_bytes(n)), 4),), 0xFF, dtype=torch.uint8, device="cuda")
    loss2 = G.flatten_loss(ts, weight, vscales=vs, scratch=dirty)
    torch.cuda.synchronize()
    assert loss2.item() == loss.item()
    expect = base.copy()
    if n:
        arg = np.argmin(s, axis=1)
        expect[np.arange(n), arg] = base[np.arange(n), arg] + np.float32(weight) / np.float32(n)
        assert np.allclose(g_act[np.arange(n), arg], weight / n)
    assert np.array_equal(vs.cpu().numpy().view(np.uint32), expect.view(np.uint32))
    if n == 0:
        return
    # after the prologue's pullback: weight · exp(s) / n on the winning axis of the RAW scale
    R = pkg.rasterizer
    dc, op = torch.zeros((n, 1, 3), device="cuda"), torch.zeros((n, 1), device="cuda")
    shs, oa, sa = R.prologue_forward(dc, None, op, ts)
    va = torch.zeros((n, 3), device="cuda")
    G.flatten_loss(ts, weight, vscales=va)
    _, _, _, vraw = R.prologue_backward(oa, sa, torch.zeros_like(shs), torch.zeros_like(oa), va, scale_dims=sd)
    torch.cuda.synchronize()
    _, g_raw, _ = gr.flatten(s, weight)
    got = vraw.cpu().numpy().astype(np.float64)
    assert np.array_equal(got != 0, g_raw != 0)
    assert np.abs(got - g_raw).max() <= 1e-6 * np.abs(g_raw).max()
    # the autograd form
    t = dev(s).reshape(n, sd).requires_grad_(True)
    G.flatten_loss_autograd(t, weight).backward()
    assert np.abs(t.grad.cpu().numpy() - g_raw).max() <= 1e-6 * np.abs(g_raw).max()


# ---- end to end ----

def _e2e_inputs(pkg, orc, which):
    if which == "grid":
        sc, cam = scenes.grid_scene_rgbdn()
        return (sc["means"], sc["shs"], sc["opac"], sc["scales"], sc["rots"]), cam, 0, (0.0, 0.0, 0.0)
    # the :rgbdn case of test_gpu_parity.test_forward_backward_vs_oracle
    W, H, deg = 64, 48, 2
    s = pkg.synthetic.make_scene(300, W, H, deg, 104, sigma_px=4.0)
    R, t = pkg.synthetic.view_pose(3)
    return (s.means, s.shs, s.opacities, s.scales, s.rotations), orc.Camera(W, H, s.focal, R=R, t=t), deg, (0.3, 0.1, 0.6)


@pytest.mark.parametrize("which", ["grid", "random"])
def test_rgbdn_end_to_end_vs_oracle(G, pkg, orc, which):
    """forward -> l1_ssim_normal_loss -> backward_raw(color_cotangent=False): the parameter gradients against the CPU oracle's
    backward fed the loss head's cotangent + the restatement's cotangent of the term (both taken on the rendered frame),
    at the tolerances of the :rgbdn parity tests (hip_helpers.compare_backward); and the term really reaches ∇rotations and
    ∇scales."""
    params, cam, deg, bg = _e2e_inputs(pkg, orc, which)
    W, H = cam.width, cam.height
    st = orc.forward(*params, cam, deg, background=bg, mode="rgbdn")
    run = HipRun(pkg, *params, cam, deg, bg, "rgbdn")
    img = run.forward()
    tgt = pkg.synthetic.make_target(W, H, 21)
    scales_raw = dev(np.log(params[3]))
    photo, normal_term, flatten_term, vpix = G.l1_ssim_normal_loss(run.rast, img, dev(tgt), run.camera, scales_raw)
    torch.cuda.synchronize()
    frame = img.cpu().numpy()
    ref = gr.depth_normal(frame, cam.focal, cam.principal, weight=G.NORMAL_CONSISTENCY_WEIGHT)
    assert ref["count"] >= 64 and np.abs(ref["vimage"]).max() > 0
    assert abs(normal_term.item() - ref["loss"]) <= 1e-5 * max(abs(ref["loss"]), 1e-6) + 1e-9
    assert abs(flatten_term.item() - gr.flatten(np.log(params[3]), G.NORMAL_FLATTEN_WEIGHT)[0]) <= 1e-6 * flatten_term.item()
    loss_o, vp_o = orc.loss_head(frame, tgt)
    assert abs(photo.item() - float(loss_o)) <= 1e-5 * max(1.0, abs(float(loss_o)))
    vp_ref = np.zeros((H, W, 8), np.float32)
    vp_ref[..., :3] = vp_o[..., :3]
    vp_ref += ref["vimage"].astype(np.float32)
    assert vpix[:, :, 3:].any().item()
    with_term = [g.clone() for g in run.rast.backward_raw(vpix, *run.t, run.camera, deg, run.bg, color_cotangent=False)[:5]]
    torch.cuda.synchronize()
    g = orc.backward(st, vp_ref, *params, cam, deg, background=bg)
    compare_backward(g, with_term + [None, None], st.radii > 0)
    # without the term: the loss head's cotangent alone
    _, vp_plain = pkg.fused_ssim.l1_ssim_loss(run.rast, img, dev(tgt))
    without = [g.clone() for g in run.rast.backward_raw(vp_plain, *run.t, run.camera, deg, run.bg)[:5]]
    torch.cuda.synchronize()
    assert not torch.equal(with_term[3], without[3]) and not torch.equal(with_term[4], without[4])   # ∇scales, ∇rotations
    # a flagged backward of this buffer is refused where the library can tell: a copy of it is not the loss head's buffer
    with pytest.raises(pkg._lib.GsrError, match="only valid for the cotangent gsr_loss_l1_ssim wrote"):
        run.rast.backward_raw(vpix.clone(), *run.t, run.camera, deg, run.bg, color_cotangent=True)


def test_color_cotangent_flag_is_refused_by_the_debug_check_in_a_fresh_process(launch_ranks):
    """GSR_CHECK_COLOR_COTANGENT=1 looks INTO the buffer: the term that `l1_ssim_normal_loss` added in place onto the loss
    head's own cotangent is seen, and `color_cotangent=True` fails with GSR_E_INVALID_ARG (geometry_cc_worker.py).  One
    child process."""
    rc, out = launch_ranks([sys.executable, os.path.join(HERE, "geometry_cc_worker.py")], 1,
                           env={"GSR_CHECK_COLOR_COTANGENT": "1"}, timeout=300, raw=True)
    assert rc == [0], out[0]
    assert "refused as expected" in out[0]


def _unfused_steps(pkg, G, steps=5):
    O, Dz, R = pkg.optim, pkg.densification, pkg.rasterizer
    W, H, deg = 128, 80, 1
    gt_scene = pkg.synthetic.make_scene(2000, W, H, deg, 31, sigma_px=4.0)
    rast = R.GaussianRasterizer(W, H, mode="rgbdn", device="cuda:0")
    cam = pkg.Camera(W, H, tuple(gt_scene.focal))
    t = [dev(gt_scene.means), dev(gt_scene.shs), dev(gt_scene.opacities.reshape(-1, 1)), dev(gt_scene.scales), dev(gt_scene.rotations)]
    target = rast.forward_raw(*t, cam, deg, (0.0, 0.0, 0.0))[..., :3].permute(2, 0, 1).contiguous().clone()
    init = pkg.synthetic.make_scene(2000, W, H, deg, 32, sigma_px=4.0)
    shs = init.shs.astype(np.float32)
    gs = Dz.GaussianModel(dev(init.means), dev(shs[:, :1]), dev(shs[:, 1:]), dev(init.scales_raw), dev(init.rotations),
                          dev(init.opacities_raw.reshape(-1, 1)))
    lrs = dict(points=1.6e-4, features_dc=2.5e-3, features_rest=1.25e-4, opacities=5e-2, scales=5e-3, rotations=1e-3)
    opts = {k: O.Adam(getattr(gs, k), lrs[k], eps=1e-15) for k in O.GROUPS}
    raw = {k: getattr(gs, k) for k in O.GROUPS}
    act = R.prologue_forward(gs.features_dc, gs.features_rest, gs.opacities, gs.scales)
    losses = []
    for _ in range(steps):
        img = rast.forward_raw(gs.points, *act, gs.rotations, cam, deg, (0.0, 0.0, 0.0))
        gen = int(rast.stats.generation)
        photo, normal_term, flat_term, vp = G.l1_ssim_normal_loss(rast, img, target, cam, gs.scales)
        vm, vs, vo, vsc, vr = rast.backward_raw(vp, gs.points, *act, gs.rotations, cam, deg, (0.0, 0.0, 0.0),
                                                forward_generation=gen)[:5]
        G.flatten_loss(gs.scales, G.NORMAL_FLATTEN_WEIGHT, vscales=vsc)
        O.trainer_tail_step(opts, raw, dict(vmeans=vm, vshs=vs, vopacities=vo, vscales=vsc, vrot=vr), *act)
        losses.append((photo.item(), normal_term.item(), flat_term.item()))
    torch.cuda.synchronize()
    return losses, [getattr(gs, k).clone() for k in O.GROUPS], [opts[k].mu.clone() for k in O.GROUPS]


def test_five_unfused_trainer_steps_are_bit_identical_run_to_run(pkg, G):
    """gsr_backward + gsr_flatten_loss (onto ∇scales) + gsr_trainer_tail_step with the regulariser on, twice."""
    l1, p1, m1 = _unfused_steps(pkg, G)
    l2, p2, m2 = _unfused_steps(pkg, G)
    assert l1 == l2 and all(np.isfinite(v) for s in l1 for v in s)
    assert any(s[1] > 0 for s in l1) and all(s[2] > 0 for s in l1)      # the terms are live on this scene
    for a, b in zip(p1 + m1, p2 + m2):
        assert torch.equal(_bits(a), _bits(b))
