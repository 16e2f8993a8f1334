"""-m gpu: the row-independent job of the :rgb zero-background backward (csrc/bwd_row_job.h).

With background (0, 0, 0), the default grad_precision and ∇shs asked for in full, composite_bwd_kernel_rgb_bg0 is launched
with extra workgroups behind the tiles': they store, per VISIBLE Gaussian, the nine floats d rgb / d dir of the SH colour into
the handle's sh_jac buffer and, per CULLED Gaussian, the zero rows of every gradient array; pergauss_bwd_kernel<..., JAC> then
reads the nine floats instead of the SH bands and leaves the rows of culled Gaussians alone.  The job's slices are
gsr_policy_bwd_row_job's (tests/test_bwd_row_job_policy.py): 256 Gaussians per workgroup for every scene here.

Every case runs on handle scratch poisoned with GSR_DEBUG_FILL=nan and guarded with GSR_DEBUG_GUARD=1, and the gradients go
into an arena filled with NaN before EACH backward: a row nobody wrote, or a Jacobian nobody stored, shows as a NaN.  All six
gradient tensors are held row by row to the oracle and the float64 model (tests/gradient_rows.py: T_i = 1e-4 |ref_i| + 1e-5
rms(ref), its rules z / a / f / b unchanged), culled Gaussians must have exact zero rows, and a second backward of the same
forward must be torch.equal to the first.

Cases (cameras 40 x 24 = 6 tiles and 80 x 64 = 20 tiles):
  * Gaussian counts 1, 63, 65, 255, 256, 257 (one slice - 1, one slice, one slice + 1) and 513 (two slices + 1), SH degree 3,
    every second Gaussian behind the camera; 63 and 65 also put ∇shs at an address that is not 16-byte aligned;
  * 2000 Gaussians behind 6 tiles (8 job workgroups: more than tiles) and 513 behind 20 tiles (3: fewer);
  * all visible; none visible (an empty view: the parent's path); visible Gaussians of whose rect the exact footprint cull emits no tile (no instance);
  * SH degrees 0, 1, 2, 3, degree 1 in 16-coefficient storage: colours clamped in one or two channels (asserted on the oracle),
    a moved camera, and a Gaussian exactly AT the camera centre, where the view direction is 0 / 0 — it is behind the near
    plane and culled; the oracle's and the float64 model's ∇means / ∇shs rows for it are NaN (0 x inf: the reference defines
    nothing there), the library's row is an exact zero as before: neither kernel of the pair may evaluate its direction;
  * an antialiased handle (the same two kernels, with the compensation's chain);
  * stale data: 600 Gaussians all visible, then on the same handle every third one only — a Jacobian left by the first view
    must not reach the second;
  * the paths that keep the parent's kernels, on the same scene and zero background: :rgbd, grad_precision accurate and
    fp32_reference, the factored SH gradient (vcolors), a view whose only listed tile is composite_bwd_long_kernel's;
  * call orders: a gsr_reserve that reallocates between forward and backward ends the forward (GSR_E_STATE, as before), and
    the forward + backward after it give the gradients of an undisturbed handle.
The fused trainer tail never takes the job; tests/test_gpu_trainer.py holds it to the unfused chain."""
import numpy as np
import pytest
import torch

import gradient_rows as gr
import list_scenes as ls

pytestmark = pytest.mark.gpu

BG0 = (0.0, 0.0, 0.0)
CAMS = {"40x24": (40, 24), "80x64": (80, 64)}
CH = {"rgb": 3, "rgbd": 5, "rgbdn": 8}
_refs = {}


def build(pkg, orc, n, wh, deg, seed, pattern, K=None, view=None, centre=False):
    """make_scene behind one of the two cameras; `pattern`: which Gaussians are moved behind the camera / off the image.
    Every fourth Gaussian's first colour channel and every sixth one's second are pushed below zero (clamped)."""
    W, H = CAMS[wh]
    s = pkg.synthetic.make_scene(n, W, H, deg, seed, sigma_px=4.0, K=K)
    means, shs, opac = s.means.copy(), s.shs.copy(), s.opacities.copy()
    if pattern == "all":
        means[:, :2] *= 0.5
    elif pattern == "none":
        means[:, 2] = -3.0
    elif pattern == "alternating":
        means[1::2, 2] = -3.0
    elif pattern == "third":
        means[np.arange(n) % 3 != 0, 2] = -3.0
    elif pattern == "offscreen":
        # every second one: centre 8 px left of the image and opacity 0.0045 — within 3 sigma of the image (visible, listed by
        # the reference), but alpha >= 1/255 only within sqrt(2 ln(255 x 0.0045)) = 0.52 sigma of the centre
        means[1::2, 0] = (-8.0 - 0.5 * W) * means[1::2, 2] / float(s.focal[0])
        opac[1::2] = 0.0045
    else:
        raise ValueError(pattern)
    shs[::4, 0, 0] = -4.0
    shs[::6, 0, 1] = -4.0
    kw = {}
    if view is not None:
        R, t = pkg.synthetic.view_pose(view)
        kw = dict(R=R, t=t)
    cam = orc.Camera(W, H, s.focal, **kw)
    if centre:
        means[n // 2] = cam.camera_center
    return (means, shs, opac, s.scales, s.rotations), cam


def reference(orc, name, arrays, cam, deg, mode="rgb", order=None):
    """Oracle state, oracle and float64 gradients of one case on the zero background: computed once, read-only."""
    if name not in _refs:
        from hip_helpers import blend_boundary_pixels
        means, shs, opac, scales, rots = arrays
        n = means.shape[0]
        vp = np.random.default_rng(53).standard_normal((cam.height, cam.width, CH[mode])).astype(np.float32)
        rs = gr.RowScene(name, arrays, cam, deg, mode, BG0, vp, order)
        st = orc.forward(*arrays, cam, deg, background=BG0, mode=mode)
        g = gr.oracle_gradients(orc, rs, st)
        f64 = gr.f64_gradients(arrays, cam, deg, mode, BG0, st, vp)
        bmask, _, ids = blend_boundary_pixels(st, opac, cam.width, cam.height, with_ids=True)
        touched = np.zeros(n, bool)
        touched[list(ids)] = True
        s = np.abs(np.asarray(scales, np.float64))
        ill = s.max(1) / np.maximum(s.min(1), 1e-30) > gr.ILL_RATIO
        graw = orc.backward(st, vp, *arrays, cam, deg, background=BG0)
        for a in list(g.values()) + list(f64.values()) + [vp]:
            a.setflags(write=False)
        _refs[name] = (graw, gr.Reference(rs, st, g, f64, st.radii > 0, touched, ill, None, bmask))
    return _refs[name]


def nan_arena(n, K, factored=False):
    return torch.full(((14 if factored else 11 + 3 * K) * n,), float("nan"), device="cuda", dtype=torch.float32)


def backward(run, vp, n, K, **kw):
    """One backward into a fresh NaN arena -> the five gradients and ∇means_2d, cloned."""
    from hip_helpers import dev
    out = run.rast.backward_raw(dev(vp), *run.t, run.camera, run.deg, run.bg, arena=nan_arena(n, K, kw.get("factored_sh", False)), **kw)
    torch.cuda.synchronize()
    return [o.clone() for o in out[:5]] + [run.rast.grad_means_2d.clone()]


def check_guards(pkg, run):
    pkg._lib.check(pkg._lib.load().gsr_debug_check_guards(run.rast._h))


def run_and_check(pkg, orc, name, arrays, cam, deg, mode="rgb", order=None, names=gr.ALL_NAMES, **form):
    """Forward + two backwards of the case on a fresh poisoned, guarded handle; every check of the module docstring."""
    from hip_helpers import HipRun
    from test_gpu_bwd_instance_trims import env
    graw, ref = reference(orc, name, arrays, cam, deg, mode, order)
    n, K = arrays[0].shape[0], arrays[1].shape[1]
    with env("GSR_DEBUG_FILL", "nan"), env("GSR_DEBUG_GUARD", "1"):
        run = HipRun(pkg, *arrays, cam, deg, BG0, mode, **form)
        run.forward()
        if form.get("exact_tile_cull"):
            assert 0 < run.rast.stats.n_rendered <= ref.st.n_rendered
        else:
            assert run.rast.stats.n_rendered == ref.st.n_rendered
        first = backward(run, ref.sc.vp, n, K)
        second = backward(run, ref.sc.vp, n, K)
        check_guards(pkg, run)
    for nm, a, b in zip(gr.ALL_NAMES, first, second):
        assert torch.equal(a, b), f"{nm}: two backwards of one forward differ"
    hold(ref, graw, first, n, names)
    return run, ref, first


def hold(ref, graw, tensors, n, names=gr.ALL_NAMES):
    rows = {nm: o.cpu().numpy().astype(np.float64).reshape(n, -1) for nm, o in zip(gr.ALL_NAMES, tensors)}
    for nm in names:
        assert np.isfinite(rows[nm]).all(), (nm, "rows nobody wrote", np.flatnonzero(~np.isfinite(rows[nm]).all(1))[:8])
        assert not rows[nm][~ref.vis].any(), nm
    if ref.vis.any():
        gr.check_scene(ref, rows, names=names)
    return rows


# ---- Gaussian counts around the trip of 64 and the slice of 256 ----
@pytest.mark.parametrize("n", [1, 63, 65, 255, 256, 257, 513])
def test_counts_around_a_trip_and_a_slice(pkg, orc, n):
    arrays, cam = build(pkg, orc, n, "40x24", 3, 300 + n, "alternating" if n > 1 else "all")
    _, ref, _ = run_and_check(pkg, orc, f"count-{n}", arrays, cam, 3)
    if n > 1:
        assert ref.vis[0::2].any() and not ref.vis[1::2].any()
    else:
        assert ref.vis.all()


# ---- more job workgroups than tiles, and fewer ----
@pytest.mark.parametrize("n,wh,job_wgs,tiles", [(2000, "40x24", 8, 6), (513, "80x64", 3, 20)])
def test_more_and_fewer_job_workgroups_than_tiles(pkg, orc, n, wh, job_wgs, tiles):
    import ctypes as C
    L = pkg._lib
    cfg, out = L.PolicyConfig(), L.BwdRowJob()
    W, H = CAMS[wh]
    L.load().gsr_policy_config_init(C.byref(cfg), W, H, 0, -1)
    L.load().gsr_policy_bwd_row_job(C.byref(cfg), n, C.byref(out))
    assert int(out.n_wg) == job_wgs and ((W + 15) // 16) * ((H + 15) // 16) == tiles
    arrays, cam = build(pkg, orc, n, wh, 2, 400 + n, "alternating")
    run_and_check(pkg, orc, f"wgs-{n}-{wh}", arrays, cam, 2)


# ---- visibility ----
def test_every_gaussian_visible(pkg, orc):
    arrays, cam = build(pkg, orc, 300, "80x64", 1, 501, "all")
    _, ref, _ = run_and_check(pkg, orc, "vis-all", arrays, cam, 1)
    assert ref.vis.all()


def test_no_gaussian_visible_is_the_empty_view(pkg, orc):
    from hip_helpers import HipRun
    from test_gpu_bwd_instance_trims import env
    arrays, cam = build(pkg, orc, 300, "80x64", 1, 502, "none")
    st = orc.forward(*arrays, cam, 1, background=BG0)
    assert not (st.radii > 0).any() and st.n_rendered == 0
    vp = np.ones((cam.height, cam.width, 3), np.float32)
    with env("GSR_DEBUG_FILL", "nan"), env("GSR_DEBUG_GUARD", "1"):
        run = HipRun(pkg, *arrays, cam, 1, BG0, "rgb")
        run.forward()
        assert run.rast.stats.n_rendered == 0
        first = backward(run, vp, 300, 4)
        second = backward(run, vp, 300, 4)
        check_guards(pkg, run)
    for nm, a, b in zip(gr.ALL_NAMES, first, second):
        assert torch.equal(a, b) and not a.any(), f"{nm}: every row of an empty view is an exact zero"


def test_visible_gaussians_without_an_instance(pkg, orc):
    """Visible (radii > 0), but the exact footprint cull emits none of the tiles of their rect: the job stores their Jacobian,
    the per-Gaussian kernel sums no row for them."""
    arrays, cam = build(pkg, orc, 300, "80x64", 2, 503, "offscreen")
    run, ref, first = run_and_check(pkg, orc, "vis-offscreen", arrays, cam, 2, exact_tile_cull=True)
    listed = np.zeros(300, bool)
    listed[run.rast.values_sorted.cpu().numpy().astype(np.int64)] = True
    bare = ref.vis & ~listed
    assert bare[1::2].sum() >= 20 and not bare[0::2].all()
    for nm, t in zip(gr.ALL_NAMES, first):
        assert not t.cpu().numpy().reshape(300, -1)[bare].any(), nm


# ---- SH degrees, clamped colours, the camera centre ----
@pytest.mark.parametrize("deg,K", [(0, None), (1, None), (1, 16), (2, None), (3, None)])
def test_degrees_with_clamped_colours_and_a_gaussian_at_the_camera_centre(pkg, orc, deg, K):
    n = 300
    arrays, cam = build(pkg, orc, n, "80x64", deg, 600 + deg, "alternating", K=K, view=2, centre=True)
    assert np.abs(cam.camera_center).max() > 0.1 and np.array_equal(arrays[0][n // 2], cam.camera_center)
    _, ref, first = run_and_check(pkg, orc, f"deg-{deg}-K{K}", arrays, cam, deg)
    assert not ref.vis[n // 2], "at the camera centre: behind the near plane"
    assert not np.isfinite(ref.orc["vmeans"][n // 2]).all(), "the oracle's own row there is not a number"
    clamped = ref.st.clamped[ref.vis]
    assert clamped[:, 0].any() and clamped[:, 1].any() and not clamped.all(1).all() and (~clamped.any(1)).any()
    if K is not None:
        assert not first[1].cpu().numpy()[:, (deg + 1) ** 2:, :].any(), "bands above the active degree: zero gradient"


def test_antialiased_handle(pkg, orc):
    """The job's pair of kernels against the parent's pair on one antialiased scene: the run with a background of 1e-30 takes the
    general compositing kernel and the per-Gaussian kernel that reads the SH bands.  The background enters the gradients through
    -T_final / (1 - alpha) (bg . v) alone, 1e-30 times a transmittance: the two runs must agree to the row tolerance."""
    from hip_helpers import HipRun
    from test_gpu_bwd_instance_trims import env
    n, deg = 513, 3
    arrays, cam = build(pkg, orc, n, "80x64", deg, 701, "alternating")
    vp = np.random.default_rng(53).standard_normal((cam.height, cam.width, 3)).astype(np.float32)
    got = {}
    with env("GSR_DEBUG_FILL", "nan"), env("GSR_DEBUG_GUARD", "1"):
        for key, bg in (("job", BG0), ("general", (1e-30, 0.0, 0.0))):
            run = HipRun(pkg, *arrays, cam, deg, bg, "rgb")
            run.rast.close()
            run.rast = pkg.rasterizer.GaussianRasterizer(cam.width, cam.height, mode="rgb", near_plane=cam.near_plane,
                                                         far_plane=cam.far_plane, antialiased=True)
            run.forward()
            got[key] = backward(run, vp, n, 16)
            check_guards(pkg, run)
    vis = run.rast.radii.cpu().numpy() > 0
    for nm, a, b in zip(gr.ALL_NAMES, got["job"], got["general"]):
        a, b = (x.cpu().numpy().astype(np.float64).reshape(n, -1) for x in (a, b))
        assert np.isfinite(a).all() and not a[~vis].any(), nm
        T, _ = gr.row_tolerance(b, vis)
        assert (np.linalg.norm(a - b, axis=1) <= T).all(), nm


# ---- a Jacobian left by an earlier view ----
def test_second_view_with_fewer_visible_gaussians_on_the_same_handle(pkg, orc):
    from hip_helpers import dev
    n, deg = 600, 3
    many, cam = build(pkg, orc, n, "80x64", deg, 801, "all")
    run, ref_many, _ = run_and_check(pkg, orc, "stale-many", many, cam, deg)
    few, _ = build(pkg, orc, n, "80x64", deg, 802, "third")
    graw, ref = reference(orc, "stale-few", few, cam, deg)
    assert ref_many.vis.all() and ref.vis.sum() <= n // 3 and ref.vis.sum() >= 100
    run.t = [dev(few[0]), dev(few[1]), dev(np.asarray(few[2]).reshape(-1, 1)), dev(few[3]), dev(few[4])]
    run.forward()
    first = backward(run, ref.sc.vp, n, 16)
    hold(ref, graw, first, n)
    check_guards(pkg, run)


# ---- the paths that keep the parent's kernels ----
@pytest.mark.parametrize("path", ["rgbd", "accurate", "fp32_reference"])
def test_modes_and_precisions_that_do_not_take_the_job(pkg, orc, path):
    n, deg = 513, 3
    arrays, cam = build(pkg, orc, n, "80x64", deg, 901, "alternating")
    if path == "rgbd":
        run_and_check(pkg, orc, "fallback-rgbd", arrays, cam, deg, mode="rgbd")
    else:
        run_and_check(pkg, orc, "fallback-rgb", arrays, cam, deg, grad_precision=path)


def test_factored_sh_gradient_does_not_take_the_job(pkg, orc):
    from hip_helpers import HipRun
    from test_gpu_bwd_instance_trims import env
    n, deg = 513, 3
    arrays, cam = build(pkg, orc, n, "80x64", deg, 901, "alternating")
    graw, ref = reference(orc, "fallback-rgb", arrays, cam, deg)
    with env("GSR_DEBUG_FILL", "nan"), env("GSR_DEBUG_GUARD", "1"):
        run = HipRun(pkg, *arrays, cam, deg, BG0, "rgb")
        run.forward()
        full = backward(run, ref.sc.vp, n, 16)
        fact = backward(run, ref.sc.vp, n, 16, factored_sh=True)
        check_guards(pkg, run)
    for k, nm in ((0, "vmeans"), (2, "vopacities"), (3, "vscales"), (4, "vrots"), (5, "vmeans2d")):
        assert torch.equal(full[k], fact[k]), f"{nm}: the job's pair of kernels and the parent's pair differ"
    vc = fact[1].cpu().numpy()
    assert np.isfinite(vc).all() and not vc[~ref.vis].any()
    # ∇shs band 0 = SH0 x vc (one rounding)
    np.testing.assert_allclose(full[1].cpu().numpy()[:, 0, :], np.float32(0.28209479177387814) * vc, rtol=3e-7, atol=0)
    hold(ref, graw, full, n)


@pytest.mark.parametrize("L", [1025, 2049])
def test_view_whose_listed_tile_is_the_long_kernels(pkg, orc, L):
    sc = ls.single_tile_scene(L, 7)
    run, ref, _ = run_and_check(pkg, orc, f"long-{L}", sc.args, sc.cam, sc.deg, order=sc.order)
    assert list(run.rast.stats.tier_tiles) == [1, 0, 0], "the one tile with a list is composite_bwd_long_kernel's"


# ---- call orders ----
def test_reserve_that_reallocates_between_forward_and_backward(pkg, orc):
    from hip_helpers import HipRun
    from test_gpu_bwd_instance_trims import env
    n, deg = 513, 3
    arrays, cam = build(pkg, orc, n, "80x64", deg, 901, "alternating")
    graw, ref = reference(orc, "fallback-rgb", arrays, cam, deg)
    L = pkg._lib
    with env("GSR_DEBUG_FILL", "nan"), env("GSR_DEBUG_GUARD", "1"):
        run = HipRun(pkg, *arrays, cam, deg, BG0, "rgb")
        run.forward()
        undisturbed = backward(run, ref.sc.vp, n, 16)
        run.forward()
        run.rast.reserve(8 * n, 0)   # reallocates the per-Gaussian buffers of the forward: it is no longer live
        with pytest.raises(L.GsrError) as e:
            backward(run, ref.sc.vp, n, 16)
        assert e.value.code == L.GSR_E_STATE
        run.forward()
        again = backward(run, ref.sc.vp, n, 16)
        run.rast.reserve(8 * n, 0)   # within capacity: reallocates nothing, the forward stays live
        third = backward(run, ref.sc.vp, n, 16)
        check_guards(pkg, run)
    for nm, a, b, c in zip(gr.ALL_NAMES, undisturbed, again, third):
        assert torch.equal(a, b) and torch.equal(a, c), nm
    hold(ref, graw, again, n)
