"""-m gpu: antialiased rendering (GSR_FLAG_ANTIALIASED, `GaussianRasterizer(antialiased=True)`) — the opacity
compensation of add_blur in `preprocess`, and its pullback through both gradient chains of `pergauss_bwd`.

What holds the mode: an antialiased render of opacities o IS the plain render of o · rho (rho: GSR_BUF_COMPENSATIONS).
  1. identity, bit for bit: every forward output and every gradient that does not pass through rho, against a plain handle fed
     o · rho_dev;
  2. rho itself against float64 (tests/antialias_ref.rho_bound);
  3. every gradient row (tests/gradient_rows.check_rows) against the composed oracle and the float64 autograd of the antialiased
     image (tests/antialias_ref.py; their premises on the CPU: tests/test_antialias_cpu.py), at all three grad_precision settings —
     what a missing or mis-signed ∇add_blur fails;
  4. the pose gradient;  5. edge rows (rho = 0, sub-pixel splats that drop out, the lone thread of a second workgroup);
  6. the fused trainer tail;  7. state and plumbing (flags, buffer 10, guards, poisoned scratch, reserve);  8. autograd.
Every test fails on a build without the mode: the constructor is refused (unknown flags 0x4)."""
import ctypes as C

import numpy as np
import pytest
import torch

import antialias_ref as ar
import gradient_rows as gr
from hip_helpers import HipRun, dev, pose_distances, pose_ok
from test_gpu_guarded_handle import debug_guard, guards_ok
from test_gpu_poisoned_buffers import POISON, WORDS, debug_fill

pytestmark = pytest.mark.gpu


class AARun(HipRun):
    """HipRun on an antialiased rasterizer (HipRun builds a plain one: it is closed and replaced)."""

    def __init__(self, pkg, *args, exact_tile_cull=False, bins_budget_bytes=0, grad_precision=None, radius_clip=3, **kw):
        super().__init__(pkg, *args, exact_tile_cull=exact_tile_cull, bins_budget_bytes=bins_budget_bytes,
                         grad_precision=grad_precision, **kw)
        self.rast.close()
        cam = self.cam
        self.rast = pkg.rasterizer.GaussianRasterizer(cam.width, cam.height, mode=self.mode, near_plane=cam.near_plane,
                                                      far_plane=cam.far_plane, exact_tile_cull=exact_tile_cull,
                                                      bins_budget_bytes=bins_budget_bytes, grad_precision=grad_precision,
                                                      radius_clip=radius_clip, antialiased=True)


def rho_of(run):
    """(rho_dev with 1 where radii == 0 — the buffer is stale there —, the device radii), numpy."""
    radii = run.rast.radii.cpu().numpy()
    rho = run.rast.compensations
    assert rho is not None and rho.dtype == torch.float32 and tuple(rho.shape) == (radii.size,)
    rho = rho.cpu().numpy().copy()
    rho[radii <= 0] = 1.0
    return rho, radii


def trained_like(pkg):
    s = pkg.synthetic.make_trained_like(1500, 96, 64, 2, seed=1010, sigma_px=3.0)
    from oracle.oracle import Camera
    vp = np.random.default_rng(5).standard_normal((64, 96, 5)).astype(np.float32)
    return gr.RowScene("trained-like", (s.means, s.shs, s.opacities, s.scales, s.rotations), Camera(96, 64, s.focal), 2, "rgbd",
                       gr.BG, vp)


def scene(pkg, name):
    return trained_like(pkg) if name == "trained-like" else gr.build_scene(pkg, name)


# ---- 1. the identity ----
IDENTITY = ("cell-101", "cell-103", "cell-104", "tile-1025", "edge-2", "trained-like")


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", IDENTITY)
def test_antialiased_render_is_the_plain_render_of_effective_opacities(pkg, name, exact):
    sc = scene(pkg, name)
    means, shs, opac, scales, rots = sc.arrays
    opac = np.asarray(opac, np.float32).reshape(-1)
    aa = AARun(pkg, means, shs, opac, scales, rots, sc.cam, sc.deg, sc.bg, sc.mode, exact_tile_cull=exact)
    img_aa = aa.forward().clone()
    rho, radii = rho_of(aa)
    vis = radii > 0
    assert vis.any() and np.isfinite(rho).all()
    pl = HipRun(pkg, means, shs, (opac * rho).astype(np.float32), scales, rots, sc.cam, sc.deg, sc.bg, sc.mode,
                exact_tile_cull=exact)
    img_pl = pl.forward().clone()
    if name == "tile-1025":
        assert list(aa.rast.stats.tier_tiles)[0] == 1, "the list beyond 1024 entries: the tier path"
    assert aa.rast.stats.n_rendered == pl.rast.stats.n_rendered and aa.rast.stats.n_visible == pl.rast.stats.n_visible
    assert torch.equal(img_aa, img_pl)
    for nm in ("accum_alpha", "n_contrib", "radii", "ranges", "values_sorted"):
        assert torch.equal(getattr(aa.rast, nm), getattr(pl.rast, nm)), nm
    n = radii.size
    L = pkg._lib
    rec_aa = aa.rast._buffer(L.BUF_GEOM, torch.int32, (n, 16))[torch.as_tensor(vis).cuda()]
    rec_pl = pl.rast._buffer(L.BUF_GEOM, torch.int32, (n, 16))[torch.as_tensor(vis).cuda()]
    assert torch.equal(rec_aa, rec_pl), "geometry records of the visible Gaussians"
    vp = np.random.default_rng(77).standard_normal(sc.vp.shape).astype(np.float32)
    out_aa, out_pl = aa.backward(vp), pl.backward(vp)
    for k, o in enumerate(out_aa[:5]):
        assert torch.isfinite(o).all(), gr.NAMES[k]
    assert torch.equal(out_aa[1], out_pl[1]), "vshs"
    assert torch.equal(aa.rast.grad_means_2d, pl.rast.grad_means_2d), "vmeans2d"
    want = (out_pl[2].cpu().numpy().reshape(-1) * rho).astype(np.float32)
    assert np.array_equal(out_aa[2].cpu().numpy().reshape(-1).view(np.int32), want.view(np.int32)), "vopacities = plain · rho"
    # ... and the geometry gradients are NOT the plain ones: the compensation has a pullback of its own
    assert not torch.equal(out_aa[3], out_pl[3]), "vscales"


# ---- 2. rho ----
@pytest.mark.parametrize("name", ["cell-101", "cell-103", "cell-104", "needle-1", "edge-2"])
def test_compensations_against_float64(pkg, name):
    sc = scene(pkg, name)
    aa = AARun(pkg, *sc.arrays, sc.cam, sc.deg, sc.bg, sc.mode)
    aa.forward()
    rho, radii = rho_of(aa)
    idx = np.flatnonzero(radii > 0)
    r = rho[idx].astype(np.float64)
    assert np.isfinite(r).all() and (r >= 0).all() and (r <= 1).all()
    with torch.no_grad():
        sub = tuple(None if k in (1, 2) else np.asarray(sc.arrays[k])[idx] for k in range(5))
        S2 = ar.preblur_cov_f64(sub, sc.cam).numpy()
        rho64 = ar.rho_f64(sc.arrays, sc.cam, rows=radii > 0).numpy()[idx]
    bound, ill = ar.rho_bound(rho64, S2)
    err = np.abs(r - rho64)
    print(f"{name}: {idx.size} visible, {int(ill.sum())} with 2-D axis ratio > 10; worst |rho_dev - rho64| / rho64 on the others "
          f"{(err[~ill] / np.maximum(rho64[~ill], 1e-300)).max():.2e}; worst err / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all(), (idx[err > bound][:8], err[err > bound][:8], bound[err > bound][:8])


# ---- 3. every gradient row ----
_rho = {}


def device_rho(pkg, name):
    """rho_dev of a scene (a forward on a default-precision antialiased handle; the compensation does not depend on
    grad_precision — asserted where it is used), once."""
    if name not in _rho:
        sc = scene(pkg, name)
        run = AARun(pkg, *sc.arrays, sc.cam, sc.deg, sc.bg, sc.mode)
        run.forward()
        _rho[name] = rho_of(run)
        run.rast.close()
    return _rho[name]


def hip_rows(run, vp, n):
    out = run.backward(np.array(vp))
    rows = {nm: o.cpu().numpy().astype(np.float64).reshape(n, -1) for nm, o in zip(gr.NAMES, out[:5])}
    rows["vmeans2d"] = run.rast.grad_means_2d.cpu().numpy().astype(np.float64).reshape(n, -1)
    return rows, out


@pytest.mark.parametrize("precision", [None, "accurate", "fp32_reference"])
@pytest.mark.parametrize("name", ["cell-101", "cell-103", "cell-104", "needle-1"])
def test_rows_antialiased(pkg, orc, name, precision):
    rho, radii = device_rho(pkg, name)
    ref = ar.reference_aa(pkg, orc, name, rho=rho)
    assert np.array_equal(ref.st.radii, radii)
    sc = ref.sc
    run = AARun(pkg, *sc.arrays, sc.cam, sc.deg, sc.bg, sc.mode, grad_precision=precision)
    run.forward()
    rho_p, _ = rho_of(run)
    assert np.array_equal(rho_p.view(np.int32), rho.view(np.int32))
    rows, _ = hip_rows(run, sc.vp, radii.size)
    for nm in gr.ALL_NAMES:
        assert not rows[nm][~ref.vis].any(), nm
    gr.check_scene(ref, rows, label=f" [antialiased, grad_precision={precision}]")
    if name == "cell-101":
        share = ar.compensation_share(ref, "vscales")
        print(f"cell-101: the compensation's share of vscales exceeds 10 T on {share:.1%} of the visible rows")
        assert share >= 0.1, "the scene cannot see ∇add_blur"
        # ... and the device's rows carry it: they are NOT the plain gradient at o · rho
        T, _ = gr.row_tolerance(np.asarray(ref.orc["vscales"]), ref.vis)
        d = np.linalg.norm(rows["vscales"] - ref.aa.plain["vscales"], axis=1)
        assert (d[ref.vis] > 10.0 * T[ref.vis]).mean() >= 0.1


# ---- 4. the pose ----
def test_pose_gradient_antialiased(pkg, orc):
    name = "cell-103"
    rho, radii = device_rho(pkg, name)
    ref = ar.reference_aa(pkg, orc, name, rho=rho, pose=True)
    sc = ref.sc
    run = AARun(pkg, *sc.arrays, sc.cam, sc.deg, sc.bg, sc.mode, pose_dev=True)
    run.forward()
    rows, out = hip_rows(run, sc.vp, radii.size)
    gr.check_scene(ref, rows, label=" [antialiased, pose]")
    vR, vt = out[5].cpu().numpy().reshape(-1), out[6].cpu().numpy().reshape(-1)
    assert np.isfinite(vR).all() and np.isfinite(vt).all()
    for nm, h, o, f in (("vR", vR, ref.aa.vR, ref.f64["vR"]), ("vt", vt, ref.aa.vt, ref.f64["vt"])):
        e = pose_distances(h, o, f)
        print(f"antialiased {nm}: HIP-oracle {e[0]:.2e}, oracle-f64 {e[1]:.2e}, HIP-f64 {e[2]:.2e}")
        assert pose_ok(*e), (nm, e)


# ---- 5. edge rows ----
def edge_scene():
    """32 x 32, N = 257, radius_clip = 2 (a splat the dilation alone carries has radius 3).
      0       two scales of 1e-20 on the optical axis, the long axis along it: the pre-blur covariance is diag(~5e-39), det_orig
              underflows to 0 — rho = 0 exactly; visible (radius 3), emits nothing;
      1..16   sub-pixel isotropic splats (0.02 px), o = 0.9: rho ~ 1.3e-3, o · rho < 1/255 — visible, emit nothing;
      17      two scales of 1e-20 off the axis: a 5-px needle whose det_orig is a denormal-sized positive number — rho ~ 1e-19;
      18..255 ordinary splats, every seventh behind the camera (culled: its compensation is never written);
      256     the lone thread of the second workgroup: a large splat (8 - 10 px), rho > 0.99."""
    from oracle.oracle import Camera
    rng = np.random.default_rng(257)
    n, W, H = 257, 32, 32
    f = np.float32(16.0 / np.tan(np.radians(30.0)))
    cam = Camera(W, H, (f, f), radius_clip=2)
    z = rng.uniform(3.0, 6.0, n)
    u, v = rng.uniform(4, 28, n), rng.uniform(4, 28, n)
    means = np.stack([(u - 16) * z / f, (v - 16) * z / f, z], 1)
    scales = (rng.uniform(1.5, 3.5, n) * z / f)[:, None] * rng.uniform(0.7, 1.4, (n, 3))
    rots = rng.standard_normal((n, 4))
    opac = rng.uniform(0.2, 0.9, n)
    means[0] = (0.0, 0.0, 4.0); scales[0] = (1e-20, 1e-20, 2.0); rots[0] = (1, 0, 0, 0); opac[0] = 0.9
    for i in range(1, 17):
        scales[i] = 0.02 * z[i] / f
        opac[i] = 0.9
    means[17] = (1.0, 0.0, 4.0); scales[17] = (1e-20, 1e-20, 2.9); rots[17] = (1, 0, 0, 0); opac[17] = 0.9
    means[18:256:7, 2] = -1.0
    means[256] = (0.5, -0.4, 4.0); scales[256] = np.array([10.0, 9.0, 8.0]) * 4.0 / f; opac[256] = 0.7
    shs = np.zeros((n, 4, 3)); shs[:, 0] = rng.normal(0.0, 0.5, (n, 3)); shs[:, 1:] = rng.normal(0.0, 0.1, (n, 3, 3))
    arrays = tuple(np.ascontiguousarray(a, np.float32) for a in (means, shs, opac, scales, rots))
    vp = rng.standard_normal((H, W, 3)).astype(np.float32)
    return gr.RowScene("aa-edge", arrays, cam, 1, "rgb", gr.BG, vp)


def test_edge_rows(pkg, orc):
    sc = edge_scene()
    n = 257
    aa = AARun(pkg, *sc.arrays, sc.cam, sc.deg, sc.bg, sc.mode, exact_tile_cull=True, radius_clip=2)
    img = aa.forward()
    rho, radii = rho_of(aa)
    assert torch.isfinite(img).all() and np.isfinite(rho).all()
    assert radii[0] > 0 and rho[0] == 0.0, (radii[0], rho[0])
    assert (radii[1:17] > 0).all() and (sc.arrays[2][1:17] * rho[1:17] < 1.0 / 255.0).all() and (rho[1:17] > 0).all()
    assert radii[17] > 0 and 0.0 <= rho[17] < 1e-9
    assert radii[256] > 0 and rho[256] > 0.99
    assert (radii[18:256:7] == 0).all()
    listed = set(aa.rast.values_sorted.cpu().numpy().tolist())
    assert not listed & set(range(18)), "Gaussians 0 .. 17 emit no instance"
    assert 256 in listed
    plain = pkg.rasterizer.GaussianRasterizer(32, 32, mode="rgb", exact_tile_cull=True, radius_clip=2)
    plain.forward_raw(*aa.t, aa.camera, sc.deg, aa.bg)
    torch.cuda.synchronize()
    assert aa.rast.stats.n_rendered < plain.stats.n_rendered
    assert set(range(1, 17)) <= set(plain.values_sorted.cpu().numpy().tolist()), "the plain render does blend the sub-pixel splats"
    rows, out = hip_rows(aa, sc.vp, n)
    for nm in gr.ALL_NAMES:
        assert np.isfinite(rows[nm]).all(), nm
        assert not rows[nm][:18].any(), (nm, "rows of Gaussians that emit nothing")
        assert not rows[nm][radii <= 0].any(), nm
    # Gaussian 256 by rule (a): within T_i of the composed oracle on the device's compensations
    o = ar.oracle_gradients_aa(orc, sc.arrays, sc.cam, sc.deg, sc.mode, sc.bg, sc.vp, rho=rho)
    assert np.array_equal(o.st.radii, radii)
    vis = radii > 0
    for nm in gr.ALL_NAMES:
        T, _ = gr.row_tolerance(o.rows[nm], vis)
        d = np.linalg.norm(rows[nm][256] - o.rows[nm][256])
        print(f"aa-edge {nm}: Gaussian 256 |hip - orc| / T = {d / T[256]:.3f}")
        assert np.linalg.norm(o.rows[nm][256]) > 0 and d <= T[256], nm


# ---- 6. the fused trainer tail ----
@pytest.mark.parametrize("n,deg,iso,mode,precision", [(600, 1, False, "rgb", None), (513, 2, True, "rgbdn", None),
                                                     (300, 3, False, "rgbd", "fp32_reference")])
def test_antialiased_backward_with_the_tail_equals_backward_then_tail(pkg, n, deg, iso, mode, precision):
    """gsr_backward_trainer_tail == gsr_backward + gsr_trainer_tail_step on antialiased handles, bit for bit (θ, μ, ν of every
    group, the activated copies, ∇means_2d), over 2 steps (the pattern of tests/test_gpu_trainer.py)."""
    W, H = 112, 80
    s = pkg.synthetic.make_scene(n, W, H, deg, 77, sigma_px=2.0)
    cam = pkg.Camera(W, H, tuple(s.focal))
    R, O = pkg.rasterizer, pkg.optim
    Cn = pkg._lib.MODES[mode]
    target = dev(np.random.default_rng(3).uniform(0, 1, (H, W, Cn)).astype(np.float32))
    s.means[::7, 2] = -1.0
    host = dict(points=s.means, features_dc=s.shs[:, :1].copy(), features_rest=s.shs[:, 1:].copy(),
                opacities=s.opacities_raw.reshape(-1, 1), scales=s.scales_raw[:, :1].copy() if iso else s.scales_raw,
                rotations=s.rotations)
    lrs = dict(points=1.6e-3, features_dc=2.5e-2, features_rest=2.5e-3, opacities=5e-2, scales=5e-3, rotations=1e-2)
    bg = (0.1, 0.2, 0.3)

    def make():
        raw = {k: dev(np.ascontiguousarray(v)) for k, v in host.items()}
        opts = {k: O.Adam(raw[k], lrs[k], eps=1e-15) for k in O.GROUPS}
        rest = raw["features_rest"] if raw["features_rest"].numel() else None
        act = list(R.prologue_forward(raw["features_dc"], rest, raw["opacities"], raw["scales"]))
        return raw, opts, act, R.GaussianRasterizer(W, H, mode=mode, grad_precision=precision, antialiased=True)

    raw_a, opt_a, act_a, rast_a = make()
    raw_b, opt_b, act_b, rast_b = make()
    for step in range(1, 3):
        img_a = rast_a.forward_raw(raw_a["points"], *act_a, raw_a["rotations"], cam, deg, bg)
        img_b = rast_b.forward_raw(raw_b["points"], *act_b, raw_b["rotations"], cam, deg, bg)
        assert torch.equal(img_a, img_b), step
        vp = (img_a - target) * (2.0 / img_a.numel())
        vp_b = vp.clone()
        vm, vsh, vo, vsc, vr, _, _ = rast_a.backward_raw(vp, raw_a["points"], *act_a, raw_a["rotations"], cam, deg, bg)
        O.trainer_tail_step(opt_a, raw_a, dict(vmeans=vm, vshs=vsh, vopacities=vo, vscales=vsc, vrot=vr), *act_a)
        O.fused_backward_tail_step(rast_b, vp_b, opt_b, raw_b, *act_b, cam, deg, bg, forward_generation=rast_b.stats.generation)
        torch.cuda.synchronize()
        assert (rast_a.gstate.radii <= 0).any() and (rast_a.gstate.radii > 0).any()
        for k in O.GROUPS:
            if not raw_a[k].numel():
                continue
            assert torch.equal(raw_a[k], raw_b[k]), (k, step)
            assert torch.equal(opt_a[k].mu, opt_b[k].mu) and torch.equal(opt_a[k].nu, opt_b[k].nu), (k, step)
        for x, y in zip(act_a, act_b):
            assert torch.equal(x, y), step
        assert torch.equal(rast_a.gstate.grad_means_2d, rast_b.gstate.grad_means_2d), step
    assert not torch.equal(raw_b["points"], dev(host["points"]))


# ---- 7. state and plumbing ----
def _buffer10(pkg, rast):
    p, sz = C.c_void_p(), C.c_size_t()
    pkg._lib.check(pkg._lib.load().gsr_buffer(rast._h, pkg._lib.BUF_COMPENSATIONS, C.byref(p), C.byref(sz)))
    return p.value, sz.value


def _small(pkg):
    W, H, n, deg = 64, 48, 300, 1
    s = pkg.synthetic.make_scene(n, W, H, deg, 41, sigma_px=2.5)
    s.means[::7, 2] = -1.0   # culled rows: their compensation is never written
    t = [dev(s.means), dev(s.shs), dev(s.opacities.reshape(-1, 1)), dev(s.scales), dev(s.rotations)]
    vp = dev(np.random.default_rng(41).standard_normal((H, W, 3)).astype(np.float32))
    return W, H, n, deg, pkg.Camera(W, H, tuple(s.focal)), t, vp


def test_a_default_handle_has_no_compensations(pkg):
    W, H, n, deg, cam, t, vp = _small(pkg)
    L = pkg._lib
    plain = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgb")
    aa = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgb", antialiased=True)
    assert aa.compensations is None and _buffer10(pkg, aa) == (None, 0), "before any forward"
    m0 = plain.memory_usage()
    plain.forward_raw(*t, cam, deg, (0, 0, 0))
    aa.forward_raw(*t, cam, deg, (0, 0, 0))
    torch.cuda.synchronize()
    assert plain.compensations is None and _buffer10(pkg, plain) == (None, 0)
    p, sz = _buffer10(pkg, aa)
    assert p and sz == 4 * n and tuple(aa.compensations.shape) == (n,)
    assert plain.memory_usage() > m0 and aa.memory_usage() > plain.memory_usage()
    for flags, ok in ((8, False), (4 | 1, False), (4 | 8, False), (4, True), (4 | 2, True)):
        cfg = L.Config(W, H, 3, 0.2, 1000.0, 3, 0.3, flags, 0, 0, 0, 0, 0)
        h = C.c_void_p()
        rc = L.load().gsr_create(C.byref(cfg), C.byref(h))
        assert rc == (L.GSR_OK if ok else L.GSR_E_INVALID_ARG), (flags, rc)
        if ok:
            L.load().gsr_destroy(h)


def _pair(pkg, fill=None):
    """forward + backward of the small scene on a fresh antialiased handle, every caller output pre-filled (`fill`)."""
    W, H, n, deg, cam, t, vp = _small(pkg)
    rast = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgb", antialiased=True)
    K = t[1].shape[1]
    arena = torch.empty((11 + 3 * K) * n, device="cuda")
    for buf in (arena, rast.image):
        if fill is None:
            buf.zero_()
        else:
            buf.view(torch.int32).fill_(WORDS[fill])
    img = rast.forward_raw(*t, cam, deg, (0.1, 0.2, 0.3)).clone()
    rho = rast.compensations.clone()
    radii = rast.radii.clone()
    out = rast.backward_raw(vp, *t, cam, deg, (0.1, 0.2, 0.3), arena=arena)
    torch.cuda.synchronize()
    vis = radii > 0
    res = dict(img=img, rho_vis=rho[vis], radii=radii, vm2=rast.grad_means_2d.clone(), **{nm: o.clone() for nm, o in zip(gr.NAMES, out[:5])})
    return rast, res


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), (what, k)


def test_guarded_antialiased_handle(pkg):
    with debug_guard(False):
        _, clean = _pair(pkg)
    with debug_guard(True):
        rast, guarded = _pair(pkg)
        guards_ok(pkg, rast)
    _same(clean, guarded, "GSR_DEBUG_GUARD=1")


@pytest.mark.parametrize("fill", POISON)
def test_poisoned_antialiased_handle(pkg, fill):
    """No poisoned word reaches an output: the compensation of a culled Gaussian (never written: the fill word) is not used."""
    with debug_fill(None):
        _, clean = _pair(pkg)
    with debug_fill(fill):
        rast, poisoned = _pair(pkg, fill)
        stale = rast.compensations[rast.radii <= 0]
    for k, v in poisoned.items():
        if v.dtype == torch.float32:
            assert torch.isfinite(v).all() and (v.abs() < 1e30).all(), k
    _same(clean, poisoned, f"GSR_DEBUG_FILL={fill}")
    assert stale.numel() and (stale.view(torch.int32) == WORDS[fill]).all(), "the culled rows were never written (stale)"


def test_a_reallocating_reserve_ends_the_compensations(pkg):
    W, H, n, deg, cam, t, vp = _small(pkg)
    rast = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgb", antialiased=True)
    rast.forward_raw(*t, cam, deg, (0, 0, 0))
    torch.cuda.synchronize()
    assert rast.compensations is not None
    m = rast.memory_usage()
    rast.reserve(0, 0)
    assert rast.compensations is not None, "a reserve that reallocates nothing leaves the forward live"
    rast.reserve(4 * n, 4 * int(rast.stats.n_rendered))
    assert rast.memory_usage() > m
    assert rast.compensations is None and _buffer10(pkg, rast) == (None, 0)
    assert not rast._forward_live()
    rast.forward_raw(*t, cam, deg, (0, 0, 0))
    torch.cuda.synchronize()
    assert rast.compensations is not None
    rast.release_scene_buffers()
    assert rast.compensations is None


# ---- 8. autograd ----
def test_autograd_through_the_prologue(pkg):
    W, H, n, deg = 64, 48, 300, 2
    s = pkg.synthetic.make_scene(n, W, H, deg, 58, sigma_px=2.0)
    cam = pkg.Camera(W, H, tuple(s.focal))
    R = pkg.rasterizer
    bg = (0.2, 0.3, 0.1)
    raw = dict(means=s.means, opac=s.opacities_raw.reshape(-1, 1), scales=s.scales_raw, rots=s.rotations, dc=s.shs[:, :1].copy(),
               rest=s.shs[:, 1:].copy())
    leaves = {k: dev(np.ascontiguousarray(v)).requires_grad_(True) for k, v in raw.items()}
    vp = dev(np.random.default_rng(58).standard_normal((H, W, 5)).astype(np.float32))
    rast = R.GaussianRasterizer(W, H, mode="rgbd", antialiased=True)
    img = rast(leaves["means"], leaves["opac"], leaves["scales"], leaves["rots"], leaves["dc"], leaves["rest"], camera=cam,
               sh_degree=deg, background=bg)
    order = ("means", "opac", "scales", "rots", "dc", "rest")
    got = torch.autograd.grad((img * vp).sum(), [leaves[k] for k in order])
    # by hand: prologue -> forward_raw -> backward_raw -> prologue_backward
    rast2 = R.GaussianRasterizer(W, H, mode="rgbd", antialiased=True)
    d = {k: v.detach() for k, v in leaves.items()}
    shs, oa, sa = R.prologue_forward(d["dc"], d["rest"], d["opac"], d["scales"])
    img2 = rast2.forward_raw(d["means"], shs, oa, sa, d["rots"], cam, deg, bg)
    assert torch.equal(img.detach(), img2)
    vm, vsh, vo, vsc, vr, _, _ = rast2.backward_raw(vp, d["means"], shs, oa, sa, d["rots"], cam, deg, bg)
    vdc, vrest, vor, vsr = R.prologue_backward(oa, sa, vsh, vo, vsc, 3)
    want = dict(means=vm, opac=vor, scales=vsr, rots=vr, dc=vdc, rest=vrest)
    for k, g in zip(order, got):
        assert torch.isfinite(g).all() and g.abs().sum() > 0, k
        assert torch.equal(g, want[k].reshape(g.shape)), k
