"""-m gpu: the camera-pose gradient ∇R / ∇t — the one output of the backward that is a reduction over every Gaussian of the
view (pergauss.hip: lane -> wave -> workgroup of 256 Gaussians -> per-workgroup partials -> pose_final_kernel).

Every case runs the HIP path with device-resident poses (HipRun(..., pose_dev=True)) against orc.backward(..., pose_grad=True),
whose pose accumulators are doubles over the reference's own fp32 per-Gaussian terms; pose = synthetic.view_pose(1), cotangent =
default_rng(3).standard_normal unless a case says otherwise; the per-Gaussian tensors go through compare_backward.  The pose
criterion is hip_helpers.pose_ok, on vR (9, column-major) and vt (3) separately: rel-L2(HIP, oracle) <= 1e-4, or — only in the
cases that name the float64 leg — against the float64 autograd model rel-L2(HIP, f64) <= 1e-4 or <= 4 x rel-L2(oracle, f64) +
1e-4.  For scale: the oracle sits 3e-7 .. 2e-6 from float64 on these scenes, and an in-order fp32 sum of the 79 per-workgroup
partials of the largest scene 1e-7 from their double sum, so a correct kernel has three orders of magnitude of room; the
conditioning Σ|partial| / |Σ partial| over the workgroups is printed (it is no reason to loosen anything).

a. every (degree, mode, grad_precision) instantiation family of pergauss_bwd_kernel<DEG, false, F32CHAIN>; the :rgbdn cells with
   the float64 leg, whose model detaches the normals from the pose (projection.jl:227-229).
b. reduction edges: 1, 63 / 64 / 65 (wave), 255 / 256 / 257 (workgroup), 513, 2 000 (8 workgroups) Gaussians, all of them
   visible up to 513, and 20 000 on 128 x 96 (79 workgroups).
c. ONE visible Gaussian at a chosen thread of a 600-Gaussian scene: the pose gradient equals, value for value, that of the
   scene holding the Gaussian alone — adding zeros is exact in any fixed-order reduction.
d. the per-Gaussian 1e-7 threshold of projection.jl:243-256 at a cotangent scale where it is active.
e. bit reproducibility: the same handle twice, a fresh handle, poisoned vR / vt buffers.
f. layout through the autograd functor.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from hip_helpers import HipRun, compare_backward, dev, pose_distances, pose_grad_f64, pose_ok, rel_l2

pytestmark = pytest.mark.gpu
CH = {"rgb": 3, "rgbd": 5, "rgbdn": 8}


def _cotangent(W, H, mode, scale=None):
    vp = np.random.default_rng(3).standard_normal((H, W, CH[mode])).astype(np.float32)
    return vp if scale is None else (np.float32(scale) * vp).astype(np.float32)


def _case(orc, arrays, focal, W, H, deg, mode, vp, f64=False):
    """The oracle side of one scene: forward, backward with pose gradients and (f64) the float64 model's pose gradient."""
    means, shs, opac, scales, rots = arrays
    R, t = _pose()
    cam = orc.Camera(W, H, focal, R=R, t=t)
    st = orc.forward(means, shs, opac, scales, rots, cam, deg, mode=mode)
    g = orc.backward(st, vp, means, shs, opac, scales, rots, cam, deg, pose_grad=True)
    f = pose_grad_f64(means, shs, opac, scales, rots, cam, deg, (0, 0, 0), mode, st, vp) if f64 else (None, None)
    return types.SimpleNamespace(arrays=arrays, cam=cam, deg=deg, mode=mode, vp=vp, st=st, g=g, fR=f[0], ft=f[1], W=W, H=H)


_PKG = None


def _pose():
    return _PKG.synthetic.view_pose(1)


def _arrays(s, keep=None):
    a = (s.means, s.shs, s.opacities, s.scales, s.rotations)
    return a if keep is None else tuple(np.ascontiguousarray(x[keep]) for x in a)


@functools.lru_cache(maxsize=None)
def _scene(orc, n, W, H, deg, mode, seed, sigma_px, all_visible=False, scale=None, f64=False):
    """synthetic.make_scene under view_pose(1) with its oracle results, computed once per test session and left unchanged.
    all_visible: the first n Gaussians of a larger cloud that survive the cull (visibility is a per-Gaussian property)."""
    if all_visible:
        s = _PKG.synthetic.make_scene(2 * n + 64, W, H, deg, seed, sigma_px=sigma_px)
        R, t = _pose()
        radii = orc.project(s.means, s.scales, s.rotations, orc.Camera(W, H, s.focal, R=R, t=t))[1]
        keep = np.flatnonzero(radii > 0)[:n]
        assert keep.size == n
        arrays = _arrays(s, keep)
    else:
        s = _PKG.synthetic.make_scene(n, W, H, deg, seed, sigma_px=sigma_px)
        arrays = _arrays(s)
    return _case(orc, arrays, s.focal, W, H, deg, mode, _cotangent(W, H, mode, scale), f64)


def _run(pkg, sc, grad_precision=None):
    return HipRun(pkg, *sc.arrays, sc.cam, sc.deg, mode=sc.mode, pose_dev=True, grad_precision=grad_precision)


def _conditioning(orc, sc):
    """max over the 12 components of Σ|partial| / |Σ partial|, the partials being the oracle's pose gradient of each block of
    256 Gaussians (what a workgroup of pergauss_bwd_kernel sums)."""
    st, g = sc.st, sc.g
    means, _, _, scales, rots = sc.arrays
    n = means.shape[0]
    parts = []
    for a in range(0, n, 256):
        b = slice(a, min(a + 256, n))
        vf = g.vfeatures[b]
        _, _, _, vR, vt = orc.project_bwd(np.ascontiguousarray(g.vmeans2d[b]), np.ascontiguousarray(g.vconics[b]),
                                          np.ascontiguousarray(vf[:, 3]) if vf.shape[1] > 3 else None,
                                          np.ascontiguousarray(vf[:, 5:8]) if vf.shape[1] > 5 else None,
                                          np.ascontiguousarray(st.conics[b]), np.ascontiguousarray(st.radii[b]),
                                          means[b], scales[b], rots[b], sc.cam, pose_grad=True)
        parts.append(np.concatenate([vR, vt]).astype(np.float64))
    p = np.stack(parts)
    return float((np.abs(p).sum(0) / np.maximum(np.abs(p.sum(0)), 1e-300)).max()), len(parts)


def _check_pose(tag, out, sc):
    """Prints the three distances of vR and vt and applies the criterion; returns the HIP (vR (9,), vt (3,)) as numpy."""
    vR, vt = compare_backward(sc.g, out, sc.st.radii > 0)
    vR, vt = vR.reshape(-1), vt.reshape(-1)
    assert np.isfinite(vR).all() and np.isfinite(vt).all()
    fmt = lambda e: "n/a" if e is None else f"{e:.2e}"  # noqa: E731
    verdicts = []
    for nm, h, o, f in (("vR", vR, sc.g.vR, sc.fR), ("vt", vt, sc.g.vt, sc.ft)):
        e = pose_distances(h, o, f)
        print(f"{tag} {nm}: HIP-oracle {fmt(e[0])}, oracle-f64 {fmt(e[1])}, HIP-f64 {fmt(e[2])}")
        verdicts.append((nm, e, pose_ok(*e)))
    for nm, e, ok in verdicts:
        assert ok, (tag, nm, e)
    return vR, vt


@pytest.fixture(autouse=True)
def _bind_pkg(pkg):
    global _PKG
    _PKG = pkg


# ---- a. every instantiation ----
CELLS = [(0, "rgb", None), (1, "rgbd", None), (2, "rgbdn", None), (3, "rgb", None), (3, "rgbdn", "accurate"),
         (0, "rgbd", "fp32_reference"), (1, "rgb", "fp32_reference"), (2, "rgbd", "fp32_reference"),
         (3, "rgbdn", "fp32_reference")]


@pytest.mark.parametrize("deg,mode,prec", CELLS)
def test_every_instantiation(pkg, orc, deg, mode, prec):
    sc = _scene(orc, 700, 64, 48, deg, mode, 4100 + deg, 4.0, f64=mode == "rgbdn")
    assert (sc.st.radii > 0).sum() > 512 and np.linalg.norm(sc.g.vR) > 0 and np.linalg.norm(sc.g.vt) > 0
    run = _run(pkg, sc, prec)
    run.forward()
    _check_pose(f"a deg {deg} :{mode} {prec}", run.backward(sc.vp), sc)


# ---- b. reduction edges ----
def _edge_scene(orc, n):
    if n == 20000:
        return _scene(orc, 20000, 128, 96, 1, "rgbd", 4242, 2.0)
    return _scene(orc, n, 64, 48, 1, "rgbd", 4300, 3.0 if n > 513 else 4.0, all_visible=n <= 513)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 2000, 20000])
def test_reduction_edges(pkg, orc, n):
    sc = _edge_scene(orc, n)
    vis = int((sc.st.radii > 0).sum())
    assert vis == n if n <= 513 else vis > 0.8 * n   # every lane (beyond 513: every workgroup) is a visible share of the sum
    assert sc.st.n_rendered > 0 and np.linalg.norm(sc.g.vt) > 0
    tag = f"b n {n}"
    if n >= 2000:
        cond, wgs = _conditioning(orc, sc)
        print(f"{tag}: {vis} visible, {sc.st.n_rendered} instances, {wgs} workgroups, max Σ|partial| / |Σ partial| = {cond:.1f}")
    run = _run(pkg, sc)
    run.forward()
    _check_pose(tag, run.backward(sc.vp), sc)


# ---- c. one visible Gaussian at a chosen thread ----
def _lone_scene(orc, j, n=600):
    """n Gaussians of which only id j survives the cull (the others: behind the camera, far off screen, or below the radius
    clip, in turn); j = None: the surviving Gaussian alone."""
    W, H, deg = 64, 48, 1
    s = _PKG.synthetic.make_scene(n, W, H, deg, 4400, sigma_px=4.0)
    R, t = _pose()
    cam = orc.Camera(W, H, s.focal, R=R, t=t)
    m2 = orc.project(s.means, s.scales, s.rotations, cam)
    radii, means2d = m2[1], m2[2]
    # the survivor: a visible Gaussian whose centre is well inside the image
    inside = (radii > 0) & (np.abs(means2d[:, 0] - W / 2) < W / 4) & (np.abs(means2d[:, 1] - H / 2) < H / 4)
    k = int(np.flatnonzero(inside)[0])
    means, shs, opac, scales, rots = (np.array(a, copy=True) for a in _arrays(s))
    one = tuple(a[k:k + 1].copy() for a in (means, shs, opac, scales, rots))
    if j is None:
        arrays = one
    else:
        i = np.arange(n)
        means[i % 3 == 0, 2] = -3.0            # behind the camera
        means[i % 3 == 1, 0] = 1.0e3           # far off screen
        scales[i % 3 == 2] = 1.0e-5            # projected radius below the clip
        for a, o in zip((means, shs, opac, scales, rots), one):
            a[j] = o[0]
        arrays = (means, shs, opac, scales, rots)
    return _case(orc, arrays, s.focal, W, H, deg, "rgbd", _cotangent(W, H, "rgbd"))


@functools.lru_cache(maxsize=None)
def _lone_reference(orc):
    sc = _lone_scene(orc, None)
    run = _run(_PKG, sc)
    run.forward()
    return _check_pose("c alone", run.backward(sc.vp), sc)


@pytest.mark.parametrize("j", [0, 63, 64, 255, 256, 511, 599])
def test_one_visible_gaussian_at_a_chosen_thread(pkg, orc, j):
    sc = _lone_scene(orc, j)
    assert (sc.st.radii > 0).sum() == 1 and sc.st.radii[j] > 0 and sc.st.n_contrib.max() == 1 and np.all(sc.g.vt != 0)
    run = _run(pkg, sc)
    run.forward()
    vR, vt = _check_pose(f"c j {j}", run.backward(sc.vp), sc)
    ref_R, ref_t = _lone_reference(orc)
    assert np.array_equal(vR, ref_R) and np.array_equal(vt, ref_t), (j, vR - ref_R, vt - ref_t)


# ---- d. the threshold is the reference's ----
def test_threshold_is_applied_per_gaussian_before_the_sum(pkg, orc):
    c = 1e-5
    full = _scene(orc, 2000, 64, 48, 3, "rgbdn", 6242, 3.0)
    sc = _scene(orc, 2000, 64, 48, 3, "rgbdn", 6242, 3.0, scale=c)
    # premise, on the oracle alone: at this cotangent scale the 1e-7 threshold removes a visible part of the sum
    eR, et = rel_l2(sc.g.vR, c * full.g.vR.astype(np.float64)), rel_l2(sc.g.vt, c * full.g.vt.astype(np.float64))
    print(f"d premise: oracle vR(c vp) against c vR(vp) {eR:.2e}, vt {et:.2e}")
    assert eR >= 5e-4 and et >= 5e-4
    run = _run(pkg, sc)
    run.forward()
    _check_pose("d c = 1e-5", run.backward(sc.vp), sc)


# ---- e. bit reproducibility ----
def _backward_into_poisoned(run, vp):
    """gsr_backward into caller buffers whose every word is 0xFFFFFFFF (backward_raw allocates vR / vt itself)."""
    L, rast = run.pkg._lib, run.rast
    inp = rast._inputs(*run.t, run.deg, run.bg)
    cs = rast._camera(run.camera, run.Rd, run.td)
    n, K = inp.n, inp.n_coeffs
    bufs = [torch.full(shape, -1, dtype=torch.int32, device="cuda").view(torch.float32)
            for shape in ((n, 3), (n, K, 3), (n, 1), (n, 3), (n, 4), (3, 3), (3,))]
    vm, vs, vo, vsc, vr, vR, vt = bufs
    g = L.Grads(vm.data_ptr(), vs.data_ptr(), vo.data_ptr(), vsc.data_ptr(), vr.data_ptr(), vR.data_ptr(), vt.data_ptr(), None,
                rast.gstate._grad_means_2d.data_ptr(), int(rast.stats.generation), 0, 0)
    vpd = dev(vp)
    L.check(rast._lib.gsr_backward(rast._h, C.byref(inp), C.byref(cs), vpd.data_ptr(), C.byref(g),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("n", [2000, 20000])
def test_bit_reproducible(pkg, orc, n):
    sc = _edge_scene(orc, n)
    results = []
    run = _run(pkg, sc)
    for _ in range(2):
        run.forward()
        results.append([o.clone() for o in run.backward(sc.vp)])
    fresh = _run(pkg, sc)
    fresh.forward()
    results.append([o.clone() for o in fresh.backward(sc.vp)])
    fresh.forward()
    results.append(_backward_into_poisoned(fresh, sc.vp))
    names = ("vmeans", "vshs", "vopacities", "vscales", "vrots", "vR", "vt")
    for k, other in enumerate(results[1:], 1):
        for nm, a, b in zip(names, results[0], other):
            assert torch.equal(a, b), (n, k, nm, (a != b).sum().item())
    _check_pose(f"e n {n}", results[3], sc)


# ---- f. layout through the autograd functor ----
def test_functor_pose_gradient_layout(pkg, orc):
    sc = _scene(orc, 300, 64, 48, 2, "rgbd", 33, 4.0)
    run = _run(pkg, sc)
    run.forward()
    raw = run.backward(sc.vp)
    vR, vt = _check_pose("f raw", raw, sc)
    assert not np.allclose(vR.reshape(3, 3), vR.reshape(3, 3).T, rtol=1e-2)  # a transposed ∇R would show
    rast = pkg.rasterizer.GaussianRasterizer(sc.W, sc.H, mode=sc.mode, near_plane=sc.cam.near_plane, far_plane=sc.cam.far_plane)
    p = [t.clone().requires_grad_(True) for t in run.t]
    Rd, td = run.Rd.clone().requires_grad_(True), run.td.clone().requires_grad_(True)
    img = pkg.rasterizer.rasterize(*p, Rd, td, rast=rast, camera=run.camera, sh_degree=sc.deg)
    (img * dev(sc.vp)).sum().backward()
    torch.cuda.synchronize()
    assert Rd.grad.shape == (3, 3) and td.grad.shape == (3,)
    assert torch.equal(Rd.grad, raw[5]) and torch.equal(td.grad, raw[6])
    for k in range(5):
        assert torch.equal(p[k].grad, raw[k])
