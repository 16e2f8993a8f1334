"""Anchored depth supervision on the MI355X: the gsr_depth_* kernels against the restatement (depth_torch.py), their
determinism, their ADD semantics, and the :rgbd / :rgbdn training path end to end with the term on.

Accuracy bar (no tolerance fixed in advance; the rule of the depth-normal term's tests): the YARDSTICK is the same
formulation evaluated in float32 by torch on the CPU against its float64 result, computed here per case; the GPU's error
against float64 must be within 4x of it, with a floor of 1e-6 relative on the scalars (the loss and σ).  The factor covers
another equally valid association of the same fp32 operations, not a wrong term, which is off by orders of magnitude."""
import numpy as np
import pytest
import torch

import depth_torch as dt
import scenes
from hip_helpers import HipRun, compare_backward, dev

pytestmark = pytest.mark.gpu

WEIGHT, LAMBDA = 2.0, 1.0
SIZES = [(2, 2), (1, 1), (1, 7), (7, 1), (97, 61), (130, 35)]   # 64x16 tiles: 130 = 2·64 + 2 wide, 35 = 2·16 + 3 high;
#                                                                  97x61: partial tiles both ways; 65x17 is in the refusal test


@pytest.fixture(scope="module")
def DS(pkg):
    return pkg.depth_supervision


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _anchor(DS, an):
    return DS.DepthAnchor(float(an.a), float(an.b), float(an.floor), float(an.disparity), float(an.p_far))


_CASES = {}


def _case(W, H, C, model):
    """(anchor, frame, prior, float64 reference, float32 yardstick) of a case: computed once, shared, never changed."""
    key = (W, H, C, model)
    if key not in _CASES:
        if (W, H, model) == (2, 2, "disparity"):
            an, prior, on_target = dt.reference_2x2()    # the reference's test frame, its sky pixel rendered nearer (z = 2)
            e = on_target.astype(np.float64) * np.array([[1.01, 0.99], [1.02, 1.0]])
            e[1, 1] = 2.0
            frame = np.zeros((2, 2, C), np.float32)
            frame[..., :3] = 0.5
            frame[..., 3], frame[..., 4] = e, 1.0
        else:
            an = dt.ANCHORS[model]
            frame, prior = dt.make_frame(W, H, C, model, seed=W * 1000 + H)
        ref = dt.evaluate(frame, prior, an, dt.QSTEP, WEIGHT, LAMBDA)
        yard = dt.evaluate(frame, prior, an, dt.QSTEP, WEIGHT, LAMBDA, dtype=torch.float32)
        for a in (frame, prior):
            a.setflags(write=False)
        _CASES[key] = (an, frame, prior, ref, yard)
    return _CASES[key]


def _run(DS, an, frame, prior, vp0=None, scratch=None, poison=False):
    ti, tp = dev(frame), dev(prior)
    a = _anchor(DS, an)
    loss, stats, maps = DS.depth_loss(ti, tp, a, dt.QSTEP, WEIGHT, LAMBDA, stats=True, scratch=scratch, maps=True)
    if poison:   # the outputs too: run again into buffers of 0xFF bytes
        H, W = prior.shape
        L = DS.L.load()
        import ctypes as C
        outs = [torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda") for n in (4, 16, 4 * W * H, 4 * W * H, W * H)]
        s = a.struct()
        DS.L.check(L.gsr_depth_loss_forward(W, H, frame.shape[2], ti.data_ptr(), tp.data_ptr(), C.byref(s), dt.QSTEP, LAMBDA, WEIGHT,
                                            *(o.data_ptr() for o in outs), scratch.data_ptr(), scratch.numel(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        loss, stats = outs[0].view(torch.float32).reshape(()), outs[1].view(torch.float32)
        maps = (outs[2].view(torch.float32).reshape(H, W), outs[3].view(torch.float32).reshape(H, W), outs[4].reshape(H, W))
    vp = torch.zeros_like(ti) if vp0 is None else dev(vp0)
    DS.depth_loss_backward_(ti, tp, a, dt.QSTEP, vp, WEIGHT, LAMBDA, scratch=scratch)
    torch.cuda.synchronize()
    return loss, stats, maps, vp


def _same_float_bits(got, want):
    """bit for bit on every pixel; where the restatement holds a NaN (a NaN prior) the kernel must hold a NaN: a NaN's payload
    is not defined by the arithmetic"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.parametrize("model", ["disparity", "depth"])
@pytest.mark.parametrize("C", [5, 8])
@pytest.mark.parametrize("W,H", SIZES)
def test_depth_loss_vs_float64_and_determinism(DS, W, H, C, model):
    an, frame, prior, ref, yard = _case(W, H, C, model)
    live = ref["w"] > 0
    r = ref["p"] - ref["target"]
    if W * H >= 64:
        # on the restatement alone: every branch is populated
        assert 0.3 <= ref["valid"].mean() <= 0.9
        assert (ref["far"] & (r > ref["band"])).any() and (ref["far"] & (r < -ref["band"])).any()
        two = live & ~ref["far"]
        assert (two & (np.abs(r) < ref["band"])).any() and (two & (np.abs(r) > ref["band"])).any()
        assert (frame[..., 4] == 1).any() and (frame[..., 4] == 0).any() and ((frame[..., 4] > 0) & (frame[..., 4] < 1e-3)).any()
        assert np.isnan(prior).any() and (prior <= 0).any()
    nb = DS.depth_loss_scratch_bytes(W, H)
    scratch = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    loss, stats, maps, vp = _run(DS, an, frame, prior, scratch=scratch)
    # 1. masks and maps: bit for bit, no pixel left out
    assert _same_float_bits(maps[0].cpu().numpy(), ref["target_map"])
    assert _same_float_bits(maps[1].cpu().numpy(), ref["half_band_map"])
    assert np.array_equal(maps[2].cpu().numpy(), dt.flags_of(ref["valid"], ref["far_extrap"]))
    tm, hm, fm = DS.depth_target(_anchor(DS, an), dev(prior), dt.QSTEP)
    assert torch.equal(fm, maps[2]) and _same_float_bits(tm.cpu().numpy(), ref["target_map"]) and \
        _same_float_bits(hm.cpu().numpy(), ref["half_band_map"])
    s_a, s_w, mu, sigma = (float(v) for v in stats.cpu().numpy())
    assert abs(s_a - ref["sum_alpha"]) <= 1e-6 * ref["sum_alpha"]
    assert abs(s_w - ref["sum_ws"]) <= 1e-6 * max(ref["sum_ws"], 1e-30)
    # 2. accuracy against float64, in units of the float32 yardstick
    v = vp.cpu().numpy().astype(np.float64)
    figures = [("loss", abs(loss.item() - ref["loss"]) / abs(ref["loss"]), abs(yard["loss"] - ref["loss"]) / abs(ref["loss"]), 1e-6),
               ("sigma", abs(sigma - ref["sigma"]) / ref["sigma"], abs(yard["sigma"] - ref["sigma"]) / ref["sigma"], 1e-6),
               ("mu", abs(mu - ref["mu"]) / abs(ref["mu"]), abs(yard["mu"] - ref["mu"]) / abs(ref["mu"]), 1e-6)]
    for name, ch in (("grad D", 3), ("grad alpha", 4)):
        assert np.abs(ref["vimage"][..., ch]).max() > 0, name
        figures.append((name, dt.rel_l2(v[..., ch], ref["vimage"][..., ch]), dt.rel_l2(yard["vimage"][..., ch], ref["vimage"][..., ch]), 0.0))
    print(f"\n[{W}x{H} C={C} {model}] valid {ref['valid'].mean():.3f} live {live.mean():.3f} loss {loss.item():.9g} sigma {sigma:.9g}")
    for name, err, yd, floor in figures:
        print(f"    {name}: err {err:.3g}, yardstick {yd:.3g}, ratio {err / yd if yd > 0 else float('inf'):.2f}")
    for name, err, yd, floor in figures:
        assert err <= max(4.0 * yd, floor), (name, err, yd)
    assert not v[..., :3].any() and not v[..., 5:].any()
    assert not v[~live][:, 3:5].any()
    # 3. determinism: a second run, and a run on 0xFF-poisoned scratch and outputs, give the same bits
    second = _run(DS, an, frame, prior, scratch=scratch)
    dirty = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    third = _run(DS, an, frame, prior, scratch=dirty, poison=True)
    for other in (second, third):
        for a, b in ((loss, other[0]), (stats, other[1]), (maps[2], other[2][2]), (vp, other[3])):
            assert torch.equal(_bits(a), _bits(b))
        for a, b in ((maps[0], other[2][0]), (maps[1], other[2][1])):
            assert _same_float_bits(b.cpu().numpy(), a.cpu().numpy())
    # 4. the backward ADDS: onto a non-zero buffer it gives buffer + gradient to the rounding of that one add, and leaves
    # every other channel bit-unchanged, a NaN in channel 0 included
    rng = np.random.default_rng(3)
    base = (rng.standard_normal((H, W, C)) * 1e-4).astype(np.float32)
    base[0, 0, 0] = np.nan
    out = _run(DS, an, frame, prior, vp0=base, scratch=scratch)[3].cpu().numpy()
    keep = [0, 1, 2] + list(range(5, C))
    assert np.array_equal(out[..., keep].view(np.uint32), base[..., keep].view(np.uint32))
    expect = (base[..., 3:5] + vp.cpu().numpy()[..., 3:5]).astype(np.float32)
    assert np.array_equal(out[..., 3:5].view(np.uint32), expect.view(np.uint32))


@pytest.mark.parametrize("model,C", [("disparity", 5), ("depth", 8)])
def test_nonfinite_values_at_weightless_pixels_cost_nothing(DS, model, C):
    W, H = 97, 61
    an, frame, prior, ref, _ = _case(W, H, C, model)
    live = ref["w"] > 0
    bad, bad_prior = frame.copy(), prior.copy()
    dead_valid = np.argwhere(~live & ref["valid"])          # valid prior, alpha <= 1e-3
    dead_invalid = np.argwhere(~live & ~ref["valid"] & (frame[..., 4] > 0.5))
    zero_alpha = np.argwhere(frame[..., 4] == 0)
    assert len(dead_valid) >= 3 and len(dead_invalid) >= 3 and len(zero_alpha) >= 1
    bad[tuple(dead_valid[0])][3] = np.nan
    bad[tuple(dead_valid[1])][3] = np.inf
    bad[tuple(dead_invalid[0])][3] = -np.inf
    bad[tuple(zero_alpha[0])][4] = np.nan                   # a non-finite alpha counts as 0: it was 0
    bad_prior[tuple(dead_invalid[1])] = np.inf
    bad_prior[tuple(dead_invalid[2])] = np.nan
    bad_prior[tuple(dead_valid[2])] = np.nan                # was valid with alpha <= 1e-3: w = 0 either way
    clean = _run(DS, an, frame, prior)
    dirty = _run(DS, an, bad, bad_prior)
    assert np.isfinite(dirty[0].item()) and torch.isfinite(dirty[3]).all().item()
    for a, b in ((clean[0], dirty[0]), (clean[1], dirty[1]), (clean[3], dirty[3])):
        assert torch.equal(_bits(a), _bits(b))


def test_autograd_form_and_refused_calls(DS, pkg):
    W, H, C = 65, 17, 5        # one past a tile edge both ways
    an = dt.ANCHORS["disparity"]
    frame, prior = dt.make_frame(W, H, C, "disparity", seed=5)
    ref = dt.evaluate(frame, prior, an, dt.QSTEP)
    a = _anchor(DS, an)
    t, tp = dev(frame).requires_grad_(True), dev(prior)
    loss = DS.ssi_depth_loss(t, tp, a, dt.QSTEP)
    (2.0 * loss).backward()
    assert abs(loss.item() - ref["loss"]) <= 1e-5 * ref["loss"]
    assert dt.rel_l2(t.grad.cpu().numpy(), 2.0 * ref["vimage"]) <= 1e-4
    ti = dev(frame)
    DS.depth_loss(ti, tp, a, dt.QSTEP, 1.0)
    with pytest.raises(ValueError, match="must not be the image"):
        DS.depth_loss_backward_(ti, tp, a, dt.QSTEP, ti, 1.0)
    with pytest.raises(ValueError, match=":rgbd / :rgbdn frame"):
        DS.depth_loss(torch.zeros((H, W, 3), device="cuda"), tp, a, dt.QSTEP, 1.0)
    with pytest.raises(ValueError, match="vpixels must have"):
        DS.depth_loss_backward_(ti, tp, a, dt.QSTEP, torch.zeros((H, W, 8), device="cuda"), 1.0)
    with pytest.raises(ValueError, match="prior must have"):
        DS.depth_loss(ti, torch.zeros((H, W + 1), device="cuda"), a, dt.QSTEP, 1.0)
    with pytest.raises(ValueError, match="scratch must be"):
        DS.depth_loss(ti, tp, a, dt.QSTEP, 1.0, scratch=torch.zeros(64, dtype=torch.uint8, device="cuda"))
    # the C ABI refuses the same, before any launch
    import ctypes as ct
    L, lib = pkg._lib, pkg._lib.load()
    s, st = a.struct(), ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = DS.depth_loss_scratch_bytes(W, H)
    scr, out, v = torch.zeros(nb, dtype=torch.uint8, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros_like(ti)
    fwd = lambda C_, nbytes: lib.gsr_depth_loss_forward(W, H, C_, ti.data_ptr(), tp.data_ptr(), ct.byref(s), dt.QSTEP, 1.0, 1.0,  # noqa: E731
                                                        out.data_ptr(), None, None, None, None, scr.data_ptr(), nbytes, st)
    assert fwd(C, nb) == 0
    assert fwd(3, nb) == L.GSR_E_INVALID_ARG and b":rgbd (5) or :rgbdn (8)" in lib.gsr_last_error_string()
    assert fwd(C, nb - 1) == L.GSR_E_INVALID_ARG and b"scratch of" in lib.gsr_last_error_string()
    bwd = lambda vptr, nbytes: lib.gsr_depth_loss_backward(W, H, C, ti.data_ptr(), tp.data_ptr(), ct.byref(s), dt.QSTEP, 1.0, 1.0,  # noqa: E731
                                                           vptr, scr.data_ptr(), nbytes, st)
    assert bwd(ti.data_ptr(), nb) == L.GSR_E_INVALID_ARG and b"must not be the image" in lib.gsr_last_error_string()
    assert bwd(v.data_ptr(), 16) == L.GSR_E_INVALID_ARG
    assert bwd(v.data_ptr(), nb) == 0
    bad = L.DepthAnchorS(1.0, 0.0, 0.0, 1.0, 0.0)   # floor = 0: 1/floor
    assert lib.gsr_depth_target(W, H, tp.data_ptr(), ct.byref(bad), dt.QSTEP, None, None, None, st) == L.GSR_E_INVALID_ARG
    torch.cuda.synchronize()


# ---- end to end ----

def _synth_prior(e, alpha, floor, seed=0):
    """a prior from the oracle's depth: the disparity of the rendered depth, warped by 2 % and rescaled to [0.3, 0.9], a
    small sky block at t = 0.004 and 5 % invalid values"""
    r = np.random.default_rng(seed)
    H, W = e.shape
    yy, xx = np.mgrid[0:H, 0:W]
    disp = 1.0 / (e * (1.0 + 0.02 * np.sin(xx / 5.0) * np.cos(yy / 7.0)) + floor)
    t = (disp - disp.min()) / (disp.max() - disp.min()) * 0.6 + 0.3
    t[:5, :6] = 0.004
    t[r.random((H, W)) < 0.05] = -1.0
    return t.astype(np.float32)


def _e2e(pkg, DS, orc, mode):
    """The 8x8 grid of flat Gaussians of scenes.py (all centres at z = 3), seen by a camera turned 0.4 rad about the y axis
    through the grid's centre, so that the centres' camera-space depths spread over [2.77, 3.23]: a fit needs a depth range,
    and the parity thresholds of ∇rotations need anisotropic Gaussians (the dome's are spheres)."""
    sc, cam0 = scenes.grid_scene_rgbdn()
    c, s = np.cos(0.4), np.sin(0.4)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    cam = orc.Camera(cam0.width, cam0.height, cam0.focal, R=R, t=np.array([-3 * s, 0, 3 - 3 * c], np.float32))
    params = (sc["means"], sc["shs"], sc["opac"], sc["scales"], sc["rots"])
    st = orc.forward(*params, cam, 0, background=(0, 0, 0), mode=mode)
    e = st.image[..., 3].astype(np.float64) / np.maximum(st.image[..., 4], 1e-6)
    pcam = pkg.Camera(cam.width, cam.height, tuple(cam.focal), tuple(cam.principal), np.asarray(cam.R), np.asarray(cam.t))
    lo, hi = DS.robust_aabb(sc["means"])
    _, zs = DS.collect_anchor_samples(sc["means"], pcam, np.ones((cam.height, cam.width), np.float32), lo, hi)
    prior = _synth_prior(e, st.image[..., 4], 0.05 * float(np.median(zs)))
    # 64 centres: fewer than the default 256 samples
    anchor = DS.fit_depth_anchors(sc["means"], [pcam], [prior], mode="ssi", min_anchor_samples=32, rng=np.random.default_rng(0))[0]
    assert anchor is not None
    return params, cam, st, prior, anchor


@pytest.mark.parametrize("mode", ["rgbd", "rgbdn"])
def test_end_to_end_vs_oracle(DS, pkg, orc, mode):
    """forward -> l1_ssim_depth_loss -> backward_raw(color_cotangent=False) against the CPU oracle's backward fed the loss
    head's cotangent + the restatement's cotangent of the term (both taken on the rendered frame), at the tolerances of
    the parity tests (hip_helpers.compare_backward).  With :rgbdn the depth and the normal term land on one cotangent."""
    params, cam, st, prior, anchor = _e2e(pkg, DS, orc, mode)
    W, H, C = cam.width, cam.height, st.image.shape[2]
    step = 1000
    run = HipRun(pkg, *params, cam, 0, (0.0, 0.0, 0.0), mode)
    img = run.forward()
    tgt, tp = pkg.synthetic.make_target(W, H, 21), dev(prior)
    photo, depth_term, vpix = DS.l1_ssim_depth_loss(run.rast, img, dev(tgt), tp, anchor, dt.QSTEP, step)
    torch.cuda.synchronize()
    frame = img.cpu().numpy()
    w = DS.depth_weight(step)
    ref = dt.evaluate(frame, prior, dt.Anchor(anchor.a, anchor.b, anchor.floor, anchor.disparity, anchor.p_far), dt.QSTEP, w)
    assert ref["loss"] > 0 and np.abs(ref["vimage"][..., 3]).max() > 0 and np.abs(ref["vimage"][..., 4]).max() > 0
    assert abs(depth_term.item() - ref["loss"]) <= 1e-5 * ref["loss"]
    loss_o, vp_o = orc.loss_head(frame, tgt)
    assert abs(photo.item() - float(loss_o)) <= 1e-5 * max(1.0, abs(float(loss_o)))
    vp_ref = np.zeros((H, W, C), np.float32)
    vp_ref[..., :3] = vp_o[..., :3]
    vp_ref += ref["vimage"].astype(np.float32)
    assert vpix[:, :, 3:5].any().item()
    with_term = [g.clone() for g in run.rast.backward_raw(vpix, *run.t, run.camera, 0, run.bg, color_cotangent=False)[:5]]
    torch.cuda.synchronize()
    g = orc.backward(st, vp_ref, *params, cam, 0, background=(0.0, 0.0, 0.0))
    compare_backward(g, with_term + [None, None], st.radii > 0)
    _, vp_plain = pkg.fused_ssim.l1_ssim_loss(run.rast, img, dev(tgt))
    vp_plain = vp_plain.clone()
    without = [g.clone() for g in run.rast.backward_raw(vp_plain, *run.t, run.camera, 0, run.bg)[:5]]
    assert not torch.equal(with_term[0], without[0]) and not torch.equal(with_term[2], without[2])   # ∇means, ∇opacities
    # a camera that lost the vote: the plain head, its cotangent untouched on channels >= 3
    photo2, none_term, vp2 = DS.l1_ssim_depth_loss(run.rast, img, dev(tgt), tp, None, dt.QSTEP, step)
    assert none_term is None and photo2.item() == photo.item() and torch.equal(_bits(vp2), _bits(vp_plain))
    if mode != "rgbdn":
        return
    # depth and normal terms together = the sum of their separate cotangents, to one fp32 add per element
    G = pkg.geometry_regularization
    nw = G.NORMAL_CONSISTENCY_WEIGHT
    terms = {}
    _, d2, both = DS.l1_ssim_depth_loss(run.rast, img, dev(tgt), tp, anchor, dt.QSTEP, step, camera=run.camera, normal_weight=nw,
                                        terms=terms)
    both = both.clone()
    only_d, only_n = torch.zeros_like(img), torch.zeros_like(img)
    DS.depth_loss(img, tp, anchor, dt.QSTEP, w)
    DS.depth_loss_backward_(img, tp, anchor, dt.QSTEP, only_d, w)
    normal_term = G.depth_normal_loss(img, run.camera, nw)
    G.depth_normal_loss_backward_(img, run.camera, only_n, nw)
    torch.cuda.synchronize()
    assert d2.item() == depth_term.item() and terms["normal"].item() == normal_term.item()
    assert only_n[..., 3:].any().item() and only_d[..., 3:5].any().item()
    expect = (vp_plain + only_d) + only_n      # channels >= 3: the head's zero + depth, then + normal
    expect[..., :3] = vp_plain[..., :3]        # the colour channels are not touched at all
    assert torch.equal(_bits(both), _bits(expect))


def _steps(pkg, DS, steps=5):
    O, Dz, R = pkg.optim, pkg.densification, pkg.rasterizer
    W, H, deg = 128, 80, 1
    gt_scene = pkg.synthetic.make_scene(2000, W, H, deg, 31, sigma_px=4.0)
    rast = R.GaussianRasterizer(W, H, mode="rgbd", device="cuda:0")
    cam = pkg.Camera(W, H, tuple(gt_scene.focal))
    t = [dev(gt_scene.means), dev(gt_scene.shs), dev(gt_scene.opacities.reshape(-1, 1)), dev(gt_scene.scales), dev(gt_scene.rotations)]
    truth = rast.forward_raw(*t, cam, deg, (0.0, 0.0, 0.0)).clone()
    target = truth[..., :3].permute(2, 0, 1).contiguous()
    # the prior: the disparity of the true scene's depth where it is opaque, a sky value elsewhere
    e = truth[..., 3] / torch.clamp(truth[..., 4], min=1e-6)
    floor = 0.05 * float(e[truth[..., 4] > 0.5].median())
    disp = 1.0 / (e + floor)
    prior = torch.where(truth[..., 4] > 0.5, disp, torch.full_like(disp, 0.004)).contiguous()
    lo, hi = (float(v) for v in torch.quantile(disp[truth[..., 4] > 0.5], torch.tensor([0.02, 0.98], device="cuda")))
    anchor = DS.DepthAnchor.from_support(1.0, 0.0, floor, 1.0, lo, hi)
    init = pkg.synthetic.make_scene(2000, W, H, deg, 32, sigma_px=4.0)
    shs = init.shs.astype(np.float32)
    gs = Dz.GaussianModel(dev(init.means), dev(shs[:, :1]), dev(shs[:, 1:]), dev(init.scales_raw), dev(init.rotations),
                          dev(init.opacities_raw.reshape(-1, 1)))
    lrs = dict(points=1.6e-4, features_dc=2.5e-3, features_rest=1.25e-4, opacities=5e-2, scales=5e-3, rotations=1e-3)
    opts = {k: O.Adam(getattr(gs, k), lrs[k], eps=1e-15) for k in O.GROUPS}
    raw = {k: getattr(gs, k) for k in O.GROUPS}
    act = R.prologue_forward(gs.features_dc, gs.features_rest, gs.opacities, gs.scales)
    losses = []
    for step in range(steps):
        img = rast.forward_raw(gs.points, *act, gs.rotations, cam, deg, (0.0, 0.0, 0.0))
        gen = int(rast.stats.generation)
        photo, depth_term, vp = DS.l1_ssim_depth_loss(rast, img, target, prior, anchor, 1.0 / 255.0, step)
        vm, vs, vo, vsc, vr = rast.backward_raw(vp, gs.points, *act, gs.rotations, cam, deg, (0.0, 0.0, 0.0),
                                                forward_generation=gen)[:5]
        O.trainer_tail_step(opts, raw, dict(vmeans=vm, vshs=vs, vopacities=vo, vscales=vsc, vrot=vr), *act)
        losses.append((photo.item(), depth_term.item()))
    torch.cuda.synchronize()
    return losses, [getattr(gs, k).clone() for k in O.GROUPS], [opts[k].mu.clone() for k in O.GROUPS]


def test_five_trainer_steps_with_the_term_are_bit_identical_run_to_run(pkg, DS):
    l1, p1, m1 = _steps(pkg, DS)
    l2, p2, m2 = _steps(pkg, DS)
    assert l1 == l2 and all(np.isfinite(v) for s in l1 for v in s)
    assert all(s[1] > 0 for s in l1)      # the term is live on this scene
    for a, b in zip(p1 + m1, p2 + m2):
        assert torch.equal(_bits(a), _bits(b))
