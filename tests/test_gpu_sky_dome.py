"""The sky dome on the MI355X: the gsr_sky_* kernels against the restatement (sky_torch.py) bit for bit, their scalars
against float64, the composite identity and the dome shell of the reference's tests on the device, the training path end
to end against the CPU oracle, trainer steps with a checkpoint resume, and the entry points on guarded buffers.

Accuracy bar of the scalars (the rule of the depth-normal and depth terms' tests): the YARDSTICK is the same formulation
evaluated in float32 by torch on the CPU against its float64 result, computed here per case; the GPU's error against
float64 must be within 4x of it, with a floor of 1e-6 relative.  Everything per pixel is compared bit for bit: the build
is uncontracted and the order of the operations is stated at the kernels."""
import numpy as np
import pytest
import torch

import scenes
import sky_torch as st
from guarded import placements
from hip_helpers import HipRun, compare_backward, dev, rel_l2, stream as _stream

pytestmark = pytest.mark.gpu

LW = 0.7
# one pixel per lane; the forward's workgroup covers 1024 pixels (four per thread), the backward's 256: 1x1, 1x7, 7x1, 17x3
# are no multiple of any vector width; 97x61 (6 / 24 workgroups) and 130x35 (5 / 18) end in a partial one.  The tile is
# larger than 256 pixels, so 320x240 would give 75 partials only: 514x512 = 257 · 1024 pixels is the smallest frame with
# more per-workgroup partials (257) than one round of the final pass's 256 threads
SIZES = [(1, 1), (1, 7), (7, 1), (17, 3), (97, 61), (130, 35), (514, 512)]
U8 = torch.uint8


@pytest.fixture(scope="module")
def SD(pkg):
    return pkg.sky_dome


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


_CASES = {}


def _case(W, H, C):
    """inputs, and per mask kind (None: no mask) the restatement, the float64 truth and the float32 yardstick: computed
    once, shared, never changed"""
    key = (W, H, C)
    if key not in _CASES:
        frame, sky, masks, g = st.make_case(W, H, C, seed=W * 1000 + H + C)
        per = {}
        for kind in (None,) + st.MASKS:
            m = None if kind is None else masks[kind]
            per[kind] = (st.restate(frame, sky, m, LW, g), st.evaluate(frame, sky, m, LW, g),
                         st.evaluate(frame, sky, m, LW, g, dtype=torch.float32))
        _CASES[key] = (frame, sky, masks, g, per)
    return _CASES[key]


def _poisoned(shape_or_bytes, dtype=torch.float32):
    n = int(np.prod(shape_or_bytes)) * (4 if dtype == torch.float32 else 1)
    raw = torch.full((n,), 0xFF, dtype=U8, device="cuda")
    return raw if dtype == U8 else raw.view(torch.float32).view(*shape_or_bytes)


def _run(SD, frame, sky, mask, g, in_place=False):
    """forward into poisoned buffers (or in place), then backward on a copy of g -> (out, loss, inv, vpixels, vsky)"""
    H, W, Cn = frame.shape
    ti, ts, tm = dev(frame), dev(sky), None if mask is None else dev(mask)
    scratch = _poisoned((SD.sky_scratch_bytes(W, H),), U8)
    out = ti if in_place else _poisoned((H, W, Cn))
    res = SD.composite_sky(ti, ts, out, tm, LW, scratch=scratch)
    loss = inv = None
    if mask is not None:
        loss = res[1]
        inv = scratch[:4].view(torch.float32).clone()
    vp, vsky = dev(g), _poisoned((H, W, 3))
    SD.sky_composite_backward_(ti, ts, vp, tm, LW, vsky=vsky, scratch=scratch)   # in place: alpha is the same in both frames
    torch.cuda.synchronize()
    return out, loss, inv, vp, vsky


@pytest.mark.parametrize("C", [5, 8])
@pytest.mark.parametrize("W,H", SIZES)
def test_composite_and_loss_vs_restatement_and_float64(SD, W, H, C):
    frame, sky, masks, g, per = _case(W, H, C)
    alpha = frame[..., 4]
    if W * H >= 51:   # on the inputs alone: alpha spans exact 0, exact 1 and the interior
        assert (alpha == 0).any() and (alpha == 1).any() and ((alpha > 0) & (alpha < 1)).any()
    keep = [0, 1, 2, 3] + list(range(5, C))
    for kind in (None,) + st.MASKS:
        mask = None if kind is None else masks[kind]
        r, ref, yard = per[kind]
        out, loss, inv, vp, vsky = _run(SD, frame, sky, mask, g)
        # 1. per pixel, bit for bit: the composite (a whole frame), vsky, channel 4; the other channels of vpixels untouched
        assert _same_bits(out.cpu().numpy(), r["out"]), kind
        assert _same_bits(vsky.cpu().numpy(), r["vsky"]), kind
        v = vp.cpu().numpy()
        assert _same_bits(v[..., 4], r["v4"]), kind
        assert _same_bits(v[..., keep], g[..., keep]), kind
        # ... and the in-place form gives the same frame and the same gradients
        out2, loss2, inv2, vp2, vsky2 = _run(SD, frame, sky, mask, g, in_place=True)
        assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(vp2), _bits(vp)) and torch.equal(_bits(vsky2), _bits(vsky))
        if mask is None:
            continue
        # 2. the scalars against float64, in units of the float32 yardstick; two runs (the second in place) bit-identical
        assert torch.equal(_bits(loss2), _bits(loss)) and torch.equal(_bits(inv2), _bits(inv))
        got_loss, got_inv = float(loss.item()), float(inv.item())
        if kind == "zero":
            assert got_loss == 0.0 and got_inv == 1.0                 # exactly: no division by zero
            assert _same_bits(v[..., 4], st.restate(frame, sky, None, LW, g)["v4"])   # ... and adds exactly 0 to the gradient
        if kind == "small":
            assert got_inv == 1.0 and masks[kind].sum() < 1           # Σw < 1: the divisor is 1
        for name, got, want, yd in (("loss", got_loss, ref["loss"], yard["loss"]), ("inv", got_inv, ref["inv"], yard["inv"])):
            scale = abs(want) if want != 0 else 1.0
            err, y = abs(got - want) / scale, abs(yd - want) / scale
            print(f"[{W}x{H} C={C} {kind}] {name}: gpu {got:.9g} f64 {want:.9g} err {err:.3g} yardstick {y:.3g}")
            assert err <= max(4.0 * y, 1e-6), (kind, name, got, want, err, y)
        # the stated order of the double sums: the restatement's bits
        assert np.float32(got_loss).tobytes() == np.float32(r["loss"]).tobytes() and np.float32(got_inv).tobytes() == np.float32(r["inv"]).tobytes()
        # the saturated pixel (alpha = 1, on the mask) keeps its gradient: alpha is the raw channel
        if kind == "fractional" and W * H >= 2:
            zero4 = g.copy()
            zero4[..., 4] = 0
            only = st.restate(frame, sky, mask, LW, zero4)["v4"] - st.restate(frame, sky, None, LW, zero4)["v4"]
            assert alpha.reshape(-1)[0] == 1 and only.reshape(-1)[0] > 0


def test_autograd_form_and_refusals(SD):
    W, H, C_ = 33, 9, 5
    frame, sky, masks, g = st.make_case(W, H, C_, seed=5)
    ref = st.evaluate(frame, np.zeros_like(sky), masks["fractional"], 1.0, np.zeros_like(g))
    t = dev(frame).requires_grad_(True)
    loss = SD.sky_opacity_loss(t, dev(masks["fractional"]))
    (2.0 * loss).backward()
    assert abs(loss.item() - ref["loss"]) <= 1e-6 * ref["loss"]
    grad = t.grad.cpu().numpy()
    assert rel_l2(grad[..., 4], 2.0 * ref["valpha"]) <= 1e-6 and not grad[..., :4].any()
    ti, ts = dev(frame), dev(sky)
    with pytest.raises(ValueError, match="no alpha row"):
        SD.composite_sky(torch.zeros((H, W, 3), device="cuda"), ts)
    with pytest.raises(ValueError, match="sky_rgb must be"):
        SD.composite_sky(ti, torch.zeros((H, W + 1, 3), device="cuda"))
    with pytest.raises(ValueError, match="must not be the image"):
        SD.sky_composite_backward_(ti, ts, ti)
    with pytest.raises(ValueError, match="scratch must be"):
        SD.composite_sky(ti, ts, None, dev(masks["zero"]), scratch=torch.zeros(8, dtype=U8, device="cuda"))
    rgb = torch.zeros((H, W, 3), device="cuda")
    assert SD.composite_sky_(rgb, None, None) is rgb       # :rgb has no alpha row: returned as it is (sky_dome.jl:221)


# K14 on the device — runtests.jl:760-797
def test_k14_composite_identity(SD, pkg):
    sc, cam = scenes.sky_test_scene()
    bg = (0.2, 0.7, 0.4)
    params = (sc["means"], sc["shs"], sc["opac"], sc["scales"], sc["rots"])
    in_kernel = HipRun(pkg, *params, cam, 0, bg, "rgbd").forward()[..., :3].clone()
    zeroed = HipRun(pkg, *params, cam, 0, (0, 0, 0), "rgbd").forward().clone()
    sky_rgb = torch.tensor(bg, device="cuda").repeat(cam.height, cam.width, 1).contiguous()
    comp = SD.composite_sky(zeroed, sky_rgb)
    alpha = zeroed[..., 4]
    assert alpha.min().item() < 1e-3 and ((alpha > 0.05) & (alpha < 0.95)).any().item() and alpha.max().item() > 0.3
    assert (comp[..., :3] - in_kernel).abs().max().item() < 1e-5
    assert torch.equal(comp[..., 3:], zeroed[..., 3:])


# K15 on the device — runtests.jl:799-841
def _oracle_dome(orc, sky, cam):
    g = sky.gaussians
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    params = (host(g.points), host(g.features_dc), host(sky._opacities_act).reshape(-1), host(sky._scales_act), host(g.rotations))
    ocam = orc.Camera(cam.width, cam.height, tuple(cam.focal), R=np.asarray(cam.R, np.float32), t=np.asarray(cam.t, np.float32),
                      far_plane=4 * sky.radius)
    return params, ocam, orc.forward(*params, ocam, 0, background=(0, 0, 0), mode="rgb")


def test_k15_dome(SD, pkg, orc):
    cam = pkg.Camera(64, 48, (100.0, 100.0))
    radius = 50.0
    sky = SD.SkyDome(cam, 8192, "sphere", radius=radius, color=(0.2, 0.4, 0.9))
    try:
        assert len(sky) == 8192 and sky.rast.far_plane > radius and sky.memory_usage() > 0
        g = sky.gaussians
        probe = pkg.rasterizer.GaussianRasterizer(64, 48, mode="rgbd", far_plane=4 * radius)
        img = probe.forward_raw(g.points, g.features_dc, sky._opacities_act, sky._scales_act, g.rotations, cam, 0, (0.0, 0.0, 0.0))
        dome_alpha = img[..., 4].clone()
        assert dome_alpha.min().item() > 0.98                      # no holes in the shell
        rgb = SD.render_sky(sky, cam)
        assert tuple(rgb.shape) == (48, 64, 3)
        opaque = dome_alpha > 0.99
        assert opaque.any().item()
        for c, e in enumerate((0.2, 0.4, 0.9)):
            assert (rgb[..., c][opaque] - e).abs().max().item() <= 1e-2
        weights = np.random.default_rng(1).standard_normal((48, 64, 3)).astype(np.float32)
        vdc = SD.sky_backward(sky, cam, dev(weights))
        torch.cuda.synchronize()
        assert vdc.shape == g.features_dc.shape and torch.isfinite(vdc).all().item() and vdc.abs().max().item() > 0
        params, ocam, ost = _oracle_dome(orc, sky, cam)
        go = orc.backward(ost, weights, *params, ocam, 0, background=(0.0, 0.0, 0.0))
        assert rel_l2(vdc.cpu().numpy(), go.vshs) <= 1e-4          # compare_backward's vshs threshold; the spheres have no
        #                                                            meaningful rotation gradient
        view = sky.view_rasterizer(pkg.Camera(32, 24, (50.0, 50.0)))
        small = SD.render_sky(sky, pkg.Camera(32, 24, (50.0, 50.0)), rast=view, forward_only=True)
        assert tuple(small.shape) == (24, 32, 3) and view.far_plane == sky.rast.far_plane
        view.close()
        probe.close()
    finally:
        sky.close()


# ---- end to end ----

def _turned(orc, cam0):
    c, s = np.cos(0.4), np.sin(0.4)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    return orc.Camera(cam0.width, cam0.height, cam0.focal, R=R, t=np.array([-3 * s, 0, 3 - 3 * c], np.float32))


def _mask(H, W, seed=2):
    r = np.random.default_rng(seed)
    m = r.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    m[:, W // 2:] = 0.0
    return m


@pytest.mark.parametrize("mode", ["rgbd", "rgbdn"])
def test_end_to_end_vs_oracle(SD, pkg, orc, mode):
    """forward over a zero background -> l1_ssim_sky_loss -> the scene's backward_raw(color_cotangent=False) and the dome's
    backward, each against the CPU oracle's backward fed the SAME cotangent, at the tolerances of the parity tests
    (hip_helpers.compare_backward).  With :rgbdn the depth-normal term lands on the same cotangent.

    The scene's Gaussians are spheres with identity rotations: under :rgbd nothing depends on their rotations, the oracle's
    ∇rotations is EXACTLY zero, and compare_backward's relative distance to a zero reference admits exact zeros only.  The
    library's reference-parity arithmetic (grad_precision="fp32_reference": the oracle's own fp32 expression tree for
    ∇scales / ∇rotations) gives those zeros (measured: 0.0), so the :rgbd case meets compare_backward in that mode.  The default
    arithmetic evaluates the same chain in float64 and leaves its rounding there (measured |∇rotations| = 7.4e-18 beside
    |∇scales| = 0.43): it is run too, its other four gradients held to compare_backward's thresholds and its ∇rotations to
    1e-12 · |∇scales| — four orders above float64 rounding, twelve below a real gradient.  Under :rgbdn the normal channel
    depends on the rotations and the default arithmetic meets compare_backward as it is."""
    sc, cam0 = scenes.sky_test_scene()
    cam = _turned(orc, cam0)
    params = (sc["means"], sc["shs"], sc["opac"], sc["scales"], sc["rots"])
    ost = orc.forward(*params, cam, 0, background=(0, 0, 0), mode=mode)
    run = HipRun(pkg, *params, cam, 0, (0.0, 0.0, 0.0), mode, grad_precision="fp32_reference" if mode == "rgbd" else None)
    W, H = cam.width, cam.height
    sky = SD.SkyDome(run.camera, 2048, "hemisphere", radius=50.0, up=(0.0, 0.0, 1.0), color=(0.3, 0.5, 0.8))
    try:
        img = run.forward()
        tgt, mask = dev(pkg.synthetic.make_target(W, H, 21)), dev(_mask(H, W))
        nw = pkg.geometry_regularization.NORMAL_CONSISTENCY_WEIGHT if mode == "rgbdn" else None
        terms = {}
        photo, sky_term, vpix, vsky = SD.l1_ssim_sky_loss(run.rast, img, tgt, sky, run.camera, mask, LW, step=600, normal=nw, terms=terms)
        torch.cuda.synchronize()
        frame, sky_rgb = img.cpu().numpy(), sky.rast.image.cpu().numpy()
        ref = st.evaluate(frame, sky_rgb, mask.cpu().numpy(), LW, np.zeros_like(frame))
        assert ref["loss"] > 0 and abs(sky_term.item() - ref["loss"]) <= 1e-6 * ref["loss"]
        comp = st.restate(frame, sky_rgb, None, LW, np.zeros_like(frame))["out"]
        loss_o, _ = orc.loss_head(comp, tgt.cpu().numpy())
        assert abs(photo.item() - float(loss_o)) <= 1e-5 * max(1.0, abs(float(loss_o)))
        assert vpix[..., 4].any().item() and vsky.any().item() and ((mode == "rgbdn") == ("normal" in terms))
        scene_g = [t.clone() for t in run.rast.backward_raw(vpix, *run.t, run.camera, 0, run.bg, color_cotangent=False)[:5]]
        vdc = SD.sky_backward(sky, run.camera, vsky).clone()
        torch.cuda.synchronize()
        go = orc.backward(ost, vpix.cpu().numpy(), *params, cam, 0, background=(0.0, 0.0, 0.0))
        compare_backward(go, scene_g + [None, None], ost.radii > 0)
        if mode == "rgbd":   # the default arithmetic on the same cotangent (see the docstring)
            dflt = HipRun(pkg, *params, cam, 0, (0.0, 0.0, 0.0), mode)
            assert torch.equal(_bits(dflt.forward()), _bits(img))
            vm, vs, vo, vsc, vr = [t.cpu().numpy() for t in dflt.rast.backward_raw(vpix, *dflt.t, dflt.camera, 0, dflt.bg)[:5]]
            for got, want in ((vm, go.vmeans), (vs, go.vshs), (vo.reshape(-1), go.vopacities), (vsc, go.vscales)):
                assert rel_l2(got, want) <= 1e-4
            print(f"[rgbd, default arithmetic] |vrots| {np.linalg.norm(vr):.3g} beside |vscales| {np.linalg.norm(go.vscales):.3g}; oracle |vrots| {np.linalg.norm(go.vrots):.3g}")
            assert not go.vrots.any() and np.linalg.norm(vr) <= 1e-12 * np.linalg.norm(go.vscales)
        dparams, dcam, dst = _oracle_dome(orc, sky, run.camera)
        gd = orc.backward(dst, vsky.cpu().numpy(), *dparams, dcam, 0, background=(0.0, 0.0, 0.0))
        assert np.abs(gd.vshs).max() > 0 and rel_l2(vdc.cpu().numpy(), gd.vshs) <= 1e-4
        # the alpha cotangent matters: the plain head on the same frame gives other ∇opacities
        _, vp_plain = pkg.fused_ssim.l1_ssim_loss(run.rast, img, tgt)
        plain_g = [t.clone() for t in run.rast.backward_raw(vp_plain.clone(), *run.t, run.camera, 0, run.bg)[:5]]
        assert not torch.equal(scene_g[2], plain_g[2])
        # before sky_loss_from_iter: no sky term, and channel 4 carries only -(g · sky)
        p2, none_term, vp2, vsky2 = SD.l1_ssim_sky_loss(run.rast, img, tgt, sky, run.camera, mask, LW, step=499)
        comp_t = SD.composite_sky(img, sky.rast.image)
        _, head = pkg.fused_ssim.l1_ssim_loss(run.rast, comp_t, tgt)
        s = sky.rast.image
        dot = (head[..., 0] * s[..., 0] + head[..., 1] * s[..., 1]) + head[..., 2] * s[..., 2]
        assert none_term is None and p2.item() == photo.item()
        assert torch.equal(vp2[..., 4], -dot) and torch.equal(vp2[..., :3], head[..., :3]) and not vp2[..., 3].any().item()
        assert torch.equal(vsky2, (1.0 - img[..., 4])[..., None] * head[..., :3])
    finally:
        sky.close()


def test_terms_compose_in_either_order_to_one_add(SD, pkg, orc):
    """The sky pullback, the depth term and the depth-normal term all ADD onto channels 3 / 4 of one cotangent: in either
    order the result is the sum of their separate contributions, to the rounding of one fp32 add per element."""
    G, DS = pkg.geometry_regularization, pkg.depth_supervision
    sc, cam0 = scenes.sky_test_scene()
    cam = _turned(orc, cam0)
    run = HipRun(pkg, sc["means"], sc["shs"], sc["opac"], sc["scales"], sc["rots"], cam, 0, (0.0, 0.0, 0.0), "rgbdn")
    W, H = cam.width, cam.height
    sky = SD.SkyDome(run.camera, 2048, "hemisphere", radius=50.0, color=(0.3, 0.5, 0.8))
    try:
        img = run.forward()
        tgt, mask = dev(pkg.synthetic.make_target(W, H, 21)), dev(_mask(H, W))
        nw = G.NORMAL_CONSISTENCY_WEIGHT
        e = img[..., 3] / torch.clamp(img[..., 4], min=1e-6)
        prior = torch.where(img[..., 4] > 0.3, 1.0 / (1.15 * e + 0.15), torch.full_like(e, 0.004)).contiguous()   # 15 % off the render
        anchor = DS.DepthAnchor.from_support(1.0, 0.0, 0.15, 1.0, 0.25, 0.4)
        depth = dict(prior=prior, anchor=anchor, qstep=1.0 / 255.0, step=1000)
        wd = DS.depth_weight(1000)
        terms = {}
        _, sky_term, both, _ = SD.l1_ssim_sky_loss(run.rast, img, tgt, sky, run.camera, mask, LW, depth=depth, normal=nw, terms=terms)
        both = both.clone()
        sky_rgb = sky.rast.image.clone()
        comp, _ = SD.composite_sky(img, sky_rgb, None, mask, LW)
        _, head = pkg.fused_ssim.l1_ssim_loss(run.rast, comp, tgt)
        head = head.clone()
        assert not head[..., 3:].any().item()
        only_s, only_d, only_n = head.clone(), torch.zeros_like(img), torch.zeros_like(img)
        SD.sky_composite_backward_(img, sky_rgb, only_s, mask, LW)
        d_term = DS.depth_loss(img, prior, anchor, 1.0 / 255.0, wd)
        DS.depth_loss_backward_(img, prior, anchor, 1.0 / 255.0, only_d, wd)
        n_term = G.depth_normal_loss(img, run.camera, nw)
        G.depth_normal_loss_backward_(img, run.camera, only_n, nw)
        assert terms["depth"].item() == d_term.item() and terms["normal"].item() == n_term.item() and sky_term.item() > 0
        assert only_s[..., 4].any().item() and only_d[..., 3:5].any().item() and only_n[..., 3:].any().item()
        expect = (only_s + only_d) + only_n          # the head's zero + sky, then + depth, then + normal
        expect[..., :3] = head[..., :3]              # the colour channels are not touched at all
        assert torch.equal(both, expect)
        # the commuted order: normal, then depth, then the sky pullback last
        other = head.clone()
        G.depth_normal_loss_backward_(img, run.camera, other, nw)
        DS.depth_loss_backward_(img, prior, anchor, 1.0 / 255.0, other, wd)
        SD.composite_sky(img, sky_rgb, None, mask, LW)      # the scratch of this mask
        SD.sky_composite_backward_(img, sky_rgb, other, mask, LW)
        sky_c = torch.zeros_like(img)
        sky_c[..., 4] = only_s[..., 4]
        expect2 = ((head + only_n) + only_d) + sky_c
        expect2[..., :3] = head[..., :3]
        assert torch.equal(other, expect2)
    finally:
        sky.close()


# ---- trainer steps ----

def _steps(pkg, SD, steps, ckpt_at=None, resume=None, path=None):
    O, Dz, R = pkg.optim, pkg.densification, pkg.rasterizer
    W, H, deg = 128, 80, 1
    gt = pkg.synthetic.make_scene(2000, W, H, deg, 31, sigma_px=4.0)
    rast = R.GaussianRasterizer(W, H, mode="rgbd", device="cuda:0")
    cam = pkg.Camera(W, H, tuple(gt.focal))
    t = [dev(gt.means), dev(gt.shs), dev(gt.opacities.reshape(-1, 1)), dev(gt.scales), dev(gt.rotations)]
    truth = rast.forward_raw(*t, cam, deg, (0.0, 0.0, 0.0)).clone()
    # the target: the true scene over a sky-blue background
    bgc = torch.tensor((0.35, 0.55, 0.9), device="cuda")
    target = (truth[..., :3] + (1.0 - truth[..., 4])[..., None] * bgc).permute(2, 0, 1).contiguous()
    mask = torch.clamp(1.0 - torch.arange(H, device="cuda") / 30.0, 0.0, 1.0).reshape(H, 1).repeat(1, W).contiguous()   # the top rows, fading
    init = pkg.synthetic.make_scene(2000, W, H, deg, 32, sigma_px=4.0)
    shs = init.shs.astype(np.float32)
    gs = Dz.GaussianModel(dev(init.means), dev(shs[:, :1]), dev(shs[:, 1:]), dev(init.scales_raw), dev(init.rotations),
                          dev(init.opacities_raw.reshape(-1, 1)))
    lrs = dict(points=1.6e-4, features_dc=2.5e-3, features_rest=1.25e-4, opacities=5e-2, scales=5e-3, rotations=1e-3)
    opts = {k: O.Adam(getattr(gs, k), lrs[k], eps=1e-15) for k in O.GROUPS}
    sky = SD.SkyDome(cam, 2048, "hemisphere", radius=60.0, color=(0.5, 0.5, 0.5), device="cuda:0")
    first = 1
    if resume is not None:
        g, first = pkg.checkpoint.load_state(resume, opts, sky=sky)
        for k in O.GROUPS:
            getattr(gs, k).copy_(dev(getattr(g, k)))
        first += 1
    losses = []
    for step in range(first, steps + 1):
        act = R.prologue_forward(gs.features_dc, gs.features_rest, gs.opacities, gs.scales)
        img = rast.forward_raw(gs.points, *act, gs.rotations, cam, deg, (0.0, 0.0, 0.0))
        gen = int(rast.stats.generation)
        photo, sky_term, vp, vsky = SD.l1_ssim_sky_loss(rast, img, target, sky, cam, mask, 0.5, step=step, sky_loss_from_iter=2)
        vm, vs, vo, vsc, vr = rast.backward_raw(vp, gs.points, *act, gs.rotations, cam, deg, (0.0, 0.0, 0.0),
                                                forward_generation=gen, color_cotangent=False)[:5]
        raw = {k: getattr(gs, k) for k in O.GROUPS}
        O.trainer_tail_step(opts, raw, dict(vmeans=vm, vshs=vs, vopacities=vo, vscales=vsc, vrot=vr), *act)
        sky.optimizer.step(sky.gaussians.features_dc, SD.sky_backward(sky, cam, vsky))
        losses.append((photo.item(), None if sky_term is None else sky_term.item()))
        if step == ckpt_at:
            torch.cuda.synchronize()
            m = pkg.ply.GaussianModel(gs.points, gs.features_dc, gs.features_rest, gs.scales, gs.rotations, gs.opacities, deg, deg)
            pkg.checkpoint.save_state(path, m, opts, step, sky=sky)
    torch.cuda.synchronize()
    state = [getattr(gs, k).clone() for k in O.GROUPS] + [opts[k].mu.clone() for k in O.GROUPS] + \
        [sky.gaussians.features_dc.clone(), sky.optimizer.mu.clone(), sky.optimizer.nu.clone()]
    count = sky.optimizer.current_step
    sky.close()
    rast.close()
    return losses, state, count


def test_five_trainer_steps_are_bit_identical_and_resume_from_a_checkpoint(pkg, SD, tmp_path):
    path = str(tmp_path / "sky.safetensors")
    l1, s1, c1 = _steps(pkg, SD, 5, ckpt_at=3, path=path)
    l2, s2, c2 = _steps(pkg, SD, 5)
    assert l1 == l2 and c1 == c2 == 5 and all(np.isfinite(s[0]) for s in l1)
    assert l1[0][1] is None and all(s[1] is not None and s[1] > 0 for s in l1[1:])   # the mask is ignored before sky_loss_from_iter
    for a, b in zip(s1, s2):
        assert torch.equal(_bits(a), _bits(b))
    l3, s3, c3 = _steps(pkg, SD, 5, resume=path)
    assert l3 == l1[3:] and c3 == 5
    for a, b in zip(s1, s3):                        # steps 4-5 bit for bit, the dome's colours and moments included
        assert torch.equal(_bits(a), _bits(b))
    ck = pkg.checkpoint.load_checkpoint(path)
    assert "sky.gaussians.points" in ck and ck.meta["sky.optimizer.current_step"] == "3"


def test_dome_colours_learn_a_uniform_sky(pkg, SD):
    """An empty scene (nothing in front of the camera) against a uniform target: only the dome can explain it, and twenty
    Adam steps on its colours bring its render closer."""
    W, H = 64, 48
    cam = pkg.Camera(W, H, (100.0, 100.0))
    rast = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgbd")
    n = 8
    means = np.zeros((n, 3), np.float32)
    means[:, 2] = -3.0                                       # behind the camera: alpha = 0 everywhere
    rots = np.zeros((n, 4), np.float32)
    rots[:, 0] = 1
    t = [dev(means), dev(np.zeros((n, 1, 3), np.float32)), dev(np.full((n, 1), 0.5, np.float32)), dev(np.full((n, 3), 0.1, np.float32)), dev(rots)]
    sky = SD.SkyDome(cam, 2048, "hemisphere", radius=50.0, color=(0.5, 0.5, 0.5))
    colour = torch.tensor((0.2, 0.7, 0.4), device="cuda")
    target = colour.reshape(3, 1, 1).repeat(1, H, W).contiguous()
    try:
        l1 = []
        for step in range(20):
            img = rast.forward_raw(*t, cam, 0, (0.0, 0.0, 0.0))
            assert step or not img.any().item()
            _, _, _, vsky = SD.l1_ssim_sky_loss(rast, img, target, sky, cam)
            l1.append((sky.rast.image - colour).abs().mean().item())
            sky.optimizer.step(sky.gaussians.features_dc, SD.sky_backward(sky, cam, vsky))
        l1.append((SD.render_sky(sky, cam, forward_only=True) - colour).abs().mean().item())
        assert all(np.isfinite(l1)) and l1[-1] < l1[0] and l1[10] < l1[0]
        # validate's form: the forward-only dome render added into the frame in place
        frame = rast.forward_raw(*t, cam, 0, (0.0, 0.0, 0.0), forward_only=True)
        assert SD.composite_sky_(frame, sky, cam) is frame and torch.equal(frame[..., :3], sky.rast.image)
    finally:
        sky.close()
        rast.close()


# ---- guarded buffers ----

@pytest.mark.parametrize("W,H,Cn", [(1, 1, 5), (17, 3, 8), (130, 35, 5), (97, 61, 8)])
def test_entry_points_on_guarded_buffers(pkg, W, H, Cn):
    """The three entry points on guarded arenas at both alignments: nothing outside out / channel 4 of vpixels / vsky /
    scratch / loss_out is written, the inputs are unchanged, and poisoned out, vsky and scratch do not reach a result."""
    L, lib = pkg._lib, pkg._lib.load()
    frame, sky, masks, g, per = _case(W, H, Cn)
    nb = int(lib.gsr_sky_scratch_bytes(W, H))
    assert nb == 16 + 16 * ((W * H + 1023) // 1024)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    ref = None
    for P in placements(4 << 20, "cuda"):
        tag = f"{P.skew}/{P.fill}"
        im, sk, mk = P.place("image", frame), P.place("sky_rgb", sky), P.place("sky_weight", masks["fractional"])
        out, loss = P.place("out", (H, W, Cn)), P.place("loss_out", (1,))
        scr = P.place("scratch", (nb,), U8, align=8, role="scratch")
        vp, vsky = P.place("vpixels", g, role="inout"), P.place("vsky", (H, W, 3))
        inplace = P.place("image_in_place", frame, role="inout")
        out2, vp2, vsky2 = P.place("out_no_mask", (H, W, Cn)), P.place("vpixels_no_mask", g, role="inout"), P.place("vsky_no_mask", (H, W, 3))
        for t in (out, scr, vsky, out2, vsky2):
            t.view(-1).view(U8).fill_(0xFF)
        calls = [
            lib.gsr_sky_composite_forward(W, H, Cn, ptr(im), ptr(sk), ptr(mk), LW, ptr(out), ptr(loss), ptr(scr), _stream()),
            lib.gsr_sky_composite_backward(W, H, Cn, ptr(im), ptr(sk), ptr(mk), LW, ptr(vp), ptr(vsky), ptr(scr), _stream()),
            lib.gsr_sky_composite_forward(W, H, Cn, ptr(inplace), ptr(sk), None, LW, ptr(inplace), None, None, _stream()),
            lib.gsr_sky_composite_forward(W, H, Cn, ptr(im), ptr(sk), None, LW, ptr(out2), None, None, _stream()),
            lib.gsr_sky_composite_backward(W, H, Cn, ptr(im), ptr(sk), None, LW, ptr(vp2), ptr(vsky2), None, _stream()),
        ]
        assert calls == [0] * 5, (tag, calls, lib.gsr_last_error_string().decode())
        torch.cuda.synchronize()
        assert P.check() == [], (tag, P.check())
        P.assert_inputs_unchanged()
        got = dict(out=out, loss=loss, inv=scr[:4].view(torch.float32), vp=vp, vsky=vsky, inplace=inplace, out2=out2, vp2=vp2, vsky2=vsky2)
        got = {k: v.clone() for k, v in got.items()}
        if ref is None:
            ref = got
            r, r0 = per["fractional"][0], per[None][0]
            for k, want in (("out", r["out"]), ("vsky", r["vsky"]), ("inplace", r0["out"]), ("out2", r0["out"]), ("vsky2", r0["vsky"])):
                assert _same_bits(got[k].cpu().numpy(), want), (tag, k)
            for k, want in (("vp", r["v4"]), ("vp2", r0["v4"])):
                v = got[k].cpu().numpy()
                keep = [0, 1, 2, 3] + list(range(5, Cn))
                assert _same_bits(v[..., 4], want) and _same_bits(v[..., keep], g[..., keep]), (tag, k)
            assert np.float32(got["loss"].item()).tobytes() == np.float32(r["loss"]).tobytes()
            assert np.float32(got["inv"].item()).tobytes() == np.float32(r["inv"]).tobytes()
            continue
        for k in got:
            assert torch.equal(got[k].contiguous().view(-1).view(U8), ref[k].contiguous().view(-1).view(U8)), (tag, k)
