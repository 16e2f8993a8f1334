"""The point-cloud initialisation on the MI355X: gsr_knn_scales (csrc/knn.hip) through point_cloud.compute_scales against
the brute-force restatement of tests/knn_ref.py — the three squared distances bit for bit, for every family, size and
order of the search —, the scales against the float64 twin, model_from_point_cloud against gaussians.jl:22-56, and the
entry point on guarded arenas (tests/guarded.py), a vector that is no permutation included."""
import ctypes as C

import numpy as np
import pytest
import torch

import knn_ref as kr
from guarded import Arena, placements
from hip_helpers import dev
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu

CASES = [(f, n) for f in kr.FAMILIES for n in kr.SIZES]


def _orders(n, seed):
    g = torch.Generator().manual_seed(seed)
    ident = torch.arange(n, dtype=torch.int32)
    return {"morton": "morton", "identity": None, "random": torch.randperm(n, generator=g).to(torch.int32).cuda(),
            "reversed": ident.flip(0).contiguous().cuda(), "identity_tensor": ident.to(torch.int64).cuda()}


@pytest.mark.parametrize("family,n", CASES)
def test_dist2_is_brute_force_bit_for_bit_in_every_order(pkg, family, n):
    """The search is exact: the multiset of the three nearest squared distances equals the brute-force search's whatever
    permutation groups the points — Morton, none, random, reversed."""
    pts = dev(kr.make_points(family, n))
    want = torch.from_numpy(kr.reference(family, n)[0])
    for name, order in _orders(n, n).items():
        scales, d2 = pkg.point_cloud.compute_scales(pts, order=order, return_dist2=True)
        got = d2.cpu()
        bad = (got.view(torch.int32) != want.view(torch.int32)).any(1).nonzero().reshape(-1)
        print(f"{family} n={n} order={name}: {bad.numel()} rows differ" + (f", first {int(bad[0])}: {got[bad[0]].tolist()} vs {want[bad[0]].tolist()}" if bad.numel() else ""))
        assert torch.equal(got, want), (family, n, name)
        assert scales.shape == (n, 3)


@pytest.mark.parametrize("family,n", CASES)
def test_scales_against_the_float64_twin(pkg, family, n):
    """|Δ| <= 1e-5 · max(1, |s|) (knn_ref.scale_tolerance: 6 fp32 roundings in md, ½·log, 1-2 ulp of logf, 5x margin); the
    three columns are one value; the isotropic column is within 2 ulp of it; point_size enters under the root."""
    pts = dev(kr.make_points(family, n))
    _, s64, s64_iso = kr.reference(family, n)
    s3 = pkg.point_cloud.compute_scales(pts).cpu().numpy()
    s1 = pkg.point_cloud.compute_scales(pts, isotropic=True).cpu().numpy()
    assert s3.shape == (n, 3) and s1.shape == (n, 1) and s3.dtype == np.float32
    err = np.abs(s3.astype(np.float64) - s64)
    print(f"{family} n={n}: max |s - s64| = {err.max():.3e}, max |s| = {np.abs(s64).max():.3f}")
    assert np.all(err <= kr.scale_tolerance(s64))
    assert np.array_equal(s3[:, 0], s3[:, 1]) and np.array_equal(s3[:, 0], s3[:, 2])
    assert np.all(np.abs(s1.astype(np.float64) - s64_iso) <= kr.scale_tolerance(s64_iso))
    assert np.all(np.abs(s1[:, 0].astype(np.float64) - s3[:, 0].astype(np.float64)) <= 2.0 * np.spacing(np.abs(s3[:, 0])))
    s4 = pkg.point_cloud.compute_scales(pts, point_size=4.0).cpu().numpy()
    want4 = kr.scales_from_dist2(kr.dist2_three(kr.make_points(family, n), np.float64), 4.0, False, np.float64)
    assert np.all(np.abs(s4.astype(np.float64) - want4) <= kr.scale_tolerance(want4))


def test_python_checks_on_device_tensors(pkg):
    pc = pkg.point_cloud
    for n in (1, 2, 3):
        with pytest.raises(ValueError, match="at least 4"):
            pc.compute_scales(torch.zeros(n, 3, device="cuda"))
    for bad in (float("nan"), float("inf"), -float("inf")):
        p = dev(kr.make_points("uniform", 65)).clone()
        p[17, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            pc.compute_scales(p)
        with pytest.raises(ValueError, match="non-finite"):
            pc.compute_scales(p, order=None)
    p = dev(kr.make_points("uniform", 65))
    with pytest.raises(ValueError):
        pc.compute_scales(p.double())
    with pytest.raises(ValueError):
        pc.compute_scales(p[:, :2])
    with pytest.raises(ValueError):
        pc.compute_scales(p.t().contiguous().t())
    with pytest.raises(ValueError, match="order"):
        pc.compute_scales(p, order="hilbert")
    with pytest.raises(ValueError, match="order"):
        pc.compute_scales(p, order=torch.arange(64, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="point_size"):
        pc.compute_scales(p, point_size=0.0)
    e = pc.compute_scales(torch.zeros(0, 3, device="cuda"), return_dist2=True)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3)


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("isotropic", [False, True])
def test_model_from_point_cloud(pkg, deg, isotropic):
    """gaussians.jl:22-56, field by field."""
    pc, n = pkg.point_cloud, 257
    f32 = np.float32
    pts_h = kr.make_points("uniform", n)
    col_h = np.random.default_rng(5).random((n, 3)).astype(f32)
    pts, col = dev(pts_h), dev(col_h)
    gs = pc.model_from_point_cloud(pts, col, max_sh_degree=deg, isotropic=isotropic, use_ids=True)
    assert isinstance(gs, pkg.densification.GaussianModel) and len(gs) == n
    k = (deg + 1) ** 2
    assert gs.points.shape == (n, 3) and gs.features_dc.shape == (n, 1, 3) and gs.features_rest.shape == (n, k - 1, 3)
    assert gs.scales.shape == (n, 1 if isotropic else 3) and gs.rotations.shape == (n, 4) and gs.opacities.shape == (n, 1)
    sh0 = f32(0.28209479177387814)
    want_dc = ((col_h - f32(0.5)) * (f32(1) / sh0)).astype(f32)   # rgb_2_sh (gaussians.jl:133)
    assert want_dc.dtype == f32
    assert np.array_equal(gs.features_dc.cpu().numpy().reshape(n, 3).view(np.uint32), want_dc.view(np.uint32))
    assert not gs.features_rest.any()
    rot = gs.rotations.cpu().numpy()
    assert np.array_equal(rot, np.tile(np.array([[1, 0, 0, 0]], f32), (n, 1)))
    op = np.log(f32(0.1) / (f32(1) - f32(0.1)))
    assert op.dtype == f32
    assert np.array_equal(gs.opacities.cpu().numpy(), np.full((n, 1), op, f32))
    assert gs.ids.dtype == torch.int32 and gs.ids.shape == (n,) and not gs.ids.any()
    assert pc.model_from_point_cloud(pts, col, max_sh_degree=deg).ids is None
    assert torch.equal(gs.scales, pc.compute_scales(pts, isotropic=isotropic))
    # the model owns its arrays: writing them leaves the arguments alone
    assert torch.equal(gs.points, pts) and gs.points.data_ptr() != pts.data_ptr()
    given = pc.compute_scales(pts)
    keep = given.clone()
    gs2 = pc.model_from_point_cloud(pts, col, given, max_sh_degree=deg, isotropic=isotropic)
    if isotropic:   # mean(scales; dims=1)
        g = given.cpu().numpy()
        assert np.array_equal(gs2.scales.cpu().numpy(), (((g[:, 0] + g[:, 1]) + g[:, 2]) / f32(3))[:, None])
    else:
        assert torch.equal(gs2.scales, given) and gs2.scales.data_ptr() != given.data_ptr()
    gs2.scales.fill_(7.0); gs2.points.fill_(7.0)
    assert torch.equal(given, keep) and torch.equal(pts.cpu(), torch.from_numpy(pts_h))
    # the empty model (gaussians.jl:58-61)
    z = torch.zeros(0, 3, device="cuda")
    e = pc.model_from_point_cloud(z, z, max_sh_degree=deg, isotropic=isotropic, use_ids=True)
    assert len(e) == 0 and e.features_rest.shape == (0, k - 1, 3) and e.scales.shape == (0, 1 if isotropic else 3) and e.ids.shape == (0,)


def test_model_renders_and_takes_a_densification_round(pkg):
    """What a trainer does first: model from the cloud, forward + loss + backward + Adam, one DefaultStrategy round."""
    R, O, Dz = pkg.rasterizer, pkg.optim, pkg.densification
    W, H, deg, n = 96, 64, 3, 1031
    s = pkg.synthetic.make_scene(n, W, H, deg, 321, sigma_px=4.0)
    cam = pkg.Camera(W, H, tuple(s.focal))
    colors = dev(np.random.default_rng(3).random((n, 3)).astype(np.float32))
    gs = pkg.point_cloud.model_from_point_cloud(dev(s.means), colors, max_sh_degree=deg, use_ids=True)
    assert len(gs) == n and bool(torch.isfinite(gs.scales).all())
    lrs = dict(points=1.6e-4, features_dc=2.5e-3, features_rest=2.5e-3 / 20, opacities=2.5e-2, scales=5e-3, rotations=1e-3)
    opt = {k: O.Adam(getattr(gs, k), lrs[k], eps=1e-15) for k in Dz.PARAMS}
    st = Dz.DefaultStrategy(gs, densify_from_iter=1, densify_until_iter=100, densification_interval=1, opacity_reset_interval=3,
                            densify_grad_threshold=1e-6, dense_percent=0.01)
    rast = R.GaussianRasterizer(W, H, mode="rgb")
    tgt = dev(pkg.synthetic.make_target(W, H, 5))
    shs, oa, sa = R.prologue_forward(gs.features_dc, gs.features_rest, gs.opacities, gs.scales)
    img = rast.forward_raw(gs.points, shs, oa, sa, gs.rotations, cam, deg, (0, 0, 0))
    loss, vp = pkg.fused_ssim.l1_ssim_loss(rast, img, tgt)
    vm, vsh, vo, vsc, vr, _, _ = rast.backward_raw(vp, gs.points, shs, oa, sa, gs.rotations, cam, deg, (0, 0, 0))
    raw = {k: getattr(gs, k) for k in Dz.PARAMS}
    O.trainer_tail_step(opt, raw, dict(vmeans=vm, vshs=vsh, vopacities=vo, vscales=vsc, vrot=vr), shs, oa, sa)
    densified, _ = Dz.post_train_step(st, gs, opt, rast, 1, 5.0, seed=1)
    torch.cuda.synchronize()
    assert densified and rast.stats.n_rendered > 0
    assert bool(torch.isfinite(img).all()) and float(img.abs().sum()) > 0.0 and np.isfinite(float(loss))
    assert len(gs) > 0 and gs.ids.shape == (len(gs),)
    for k in Dz.PARAMS:
        t = getattr(gs, k)
        assert t.shape[0] == len(gs) and bool(torch.isfinite(t).all()), k


def _knn_calls(lib, P, n, pts_h, order_h, tag):
    """gsr_knn_scales on the placement P: (3 columns, dist2 given) and (1 column, dist2 NULL), both through `order_h`, and
    (3 columns, dist2 given) with order NULL; scratch exactly gsr_knn_scratch_bytes(n) long."""
    U8 = torch.uint8
    nb = int(lib.gsr_knn_scratch_bytes(n))
    assert nb == 16 * n + 24 * ((n + 63) // 64)
    pts = P.place("points", pts_h)
    order = P.place("order", order_h, guard=(0, n - 1))
    s3, d3, scr3 = P.place("scales3", (n, 3)), P.place("dist2", (n, 3)), P.place("scratch3", (nb,), U8, align=16, role="scratch")
    s1, scr1 = P.place("scales1", (n, 1)), P.place("scratch1", (nb,), U8, align=16, role="scratch")
    s3n, d3n, scr3n = P.place("scales3_null_order", (n, 3)), P.place("dist2_null_order", (n, 3)), P.place("scratch3n", (nb,), U8, align=16, role="scratch")
    if P.skew == "worst":
        assert pts.data_ptr() % 16 == 4 and order.data_ptr() % 16 == 4 and scr3.data_ptr() % 32 == 16
    for t in (s3, d3, scr3, s1, scr1, s3n, d3n, scr3n):
        t.view(-1).view(U8).fill_(0xFF)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    calls = [lib.gsr_knn_scales(n, ptr(pts), ptr(order), 1.0, 3, ptr(s3), ptr(d3), ptr(scr3), nb, _stream()),
             lib.gsr_knn_scales(n, ptr(pts), ptr(order), 1.0, 1, ptr(s1), None, ptr(scr1), nb, _stream()),
             lib.gsr_knn_scales(n, ptr(pts), None, 1.0, 3, ptr(s3n), ptr(d3n), ptr(scr3n), nb, _stream())]
    assert calls == [0] * 3, (tag, calls, lib.gsr_last_error_string().decode())
    torch.cuda.synchronize()
    assert P.check() == [], (tag, P.check())
    P.assert_inputs_unchanged()
    return {k: v.clone() for k, v in dict(s3=s3, d3=d3, s1=s1, s3n=s3n, d3n=d3n).items()}


@pytest.mark.parametrize("n", [4, 65, 257, 1031])
@pytest.mark.parametrize("family", ["uniform", "duplicated"])
def test_entry_point_on_guarded_buffers(pkg, family, n):
    """The five placements: no guard word changes, the inputs are unchanged, poisoned outputs and scratch do not reach a
    result, and the results are the same bits everywhere.  Under skew "worst" points and order start at 4 mod 16 and the
    scratch at 16 mod 32: the entry point may not ask for more."""
    lib = pkg._lib.load()
    pts_h = kr.make_points(family, n)
    order_h = np.random.default_rng(n).permutation(n).astype(np.int32)
    want = torch.from_numpy(kr.reference(family, n)[0])
    ref = None
    for P in placements(1 << 20, "cuda"):
        tag = f"{P.skew}/{P.fill}"
        got = _knn_calls(lib, P, n, pts_h, order_h, tag)
        assert torch.equal(got["d3"].cpu(), want) and torch.equal(got["d3n"].cpu(), want), tag
        assert torch.equal(got["s3"], got["s3n"]), tag
        if ref is None:
            ref = got
            continue
        for k in got:
            assert torch.equal(got[k].contiguous().view(-1).view(torch.uint8), ref[k].contiguous().view(-1).view(torch.uint8)), (tag, k)


def test_non_finite_points_are_nobodys_neighbour(pkg):
    """The C ABI takes what the Python layer refuses: rows with a NaN or an Inf coordinate.  The call returns, no guard word
    changes, and every FINITE row gets exactly the brute-force answer over the finite rows alone (min / max drop the NaN, an
    infinite distance never beats a finite one).  The rows of the non-finite points themselves are unspecified."""
    lib = pkg._lib.load()
    n, U8 = 257, torch.uint8
    pts_h = kr.make_points("uniform", n).copy()
    bad = np.array([0, 3, 63, 64, 65, 128, 200, 255, 256])
    pts_h[bad[0::3], 0] = np.nan
    pts_h[bad[1::3], 1] = np.inf
    pts_h[bad[2::3], 2] = -np.inf
    pts_h[200] = np.nan
    good = np.setdiff1d(np.arange(n), bad)
    want = torch.from_numpy(kr.dist2_three(pts_h[good]))
    nb = int(lib.gsr_knn_scratch_bytes(n))
    order_h = np.random.default_rng(4).permutation(n).astype(np.int32)
    for P in placements(1 << 20, "cuda"):
        tag = f"{P.skew}/{P.fill}"
        pts, order = P.place("points", pts_h), P.place("order", order_h, guard=(0, n - 1))
        for k, o in (("given order", order), ("no order", None)):
            s3, d3 = P.place(f"scales {k}", (n, 3)), P.place(f"dist2 {k}", (n, 3))
            scr = P.place(f"scratch {k}", (nb,), U8, align=16, role="scratch")
            rc = lib.gsr_knn_scales(n, C.c_void_p(pts.data_ptr()), None if o is None else C.c_void_p(o.data_ptr()), 1.0, 3,
                                    C.c_void_p(s3.data_ptr()), C.c_void_p(d3.data_ptr()), C.c_void_p(scr.data_ptr()), nb, _stream())
            assert rc == 0, (tag, k, lib.gsr_last_error_string().decode())
            torch.cuda.synchronize()
            assert torch.equal(d3.cpu()[good], want), (tag, k)
            assert bool(torch.isfinite(s3.cpu()[good]).all()), (tag, k)
        assert P.check() == [], (tag, P.check())
        P.assert_inputs_unchanged()


def test_out_of_range_order_stays_inside_the_arrays(pkg):
    """A vector that is no permutation — negative, n, far past n, INT32 extremes, repeats — is clamped by the gather: the call
    returns, no guard word changes and the inputs are unchanged.  No value is asserted (the numbers are wrong by design).
    Guarded arenas only: an access outside an array must land in a guard, not in somebody else's allocation."""
    lib = pkg._lib.load()
    n, U8 = 257, torch.uint8
    pts_h = kr.make_points("uniform", n)
    order_h = np.random.default_rng(9).integers(-3 * n, 4 * n, n).astype(np.int32)
    order_h[:6] = [-1, n, n + 1, 2 ** 31 - 1, -2 ** 31, 0]
    nb = int(lib.gsr_knn_scratch_bytes(n))
    for skew in ("aligned", "worst"):
        for fill in (0, 1):
            P = Arena(1 << 20, "cuda", skew, fill)
            pts = P.place("points", pts_h)
            order = P.place("order", order_h, guard=(0, n - 1))
            s3, d3 = P.place("scales", (n, 3)), P.place("dist2", (n, 3))
            scr = P.place("scratch", (nb,), U8, align=16, role="scratch")
            rc = lib.gsr_knn_scales(n, C.c_void_p(pts.data_ptr()), C.c_void_p(order.data_ptr()), 1.0, 3, C.c_void_p(s3.data_ptr()),
                                    C.c_void_p(d3.data_ptr()), C.c_void_p(scr.data_ptr()), nb, _stream())
            assert rc == 0, lib.gsr_last_error_string().decode()
            torch.cuda.synchronize()
            assert P.check() == [], (skew, fill, P.check())
            P.assert_inputs_unchanged()
