"""The host side of the sky dome (gaussiansplatting.jl_amd/sky_dome.py; src/sky_dome.jl) without a GPU: the lattice, the
restatement's known answers, `merge_sky`, the `sky.*` checkpoint group, and the calls the C ABI refuses before it touches
a device."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import scenes
import sky_torch as st

f32 = np.float32


@pytest.fixture(scope="module")
def SD(pkg):
    return pkg.sky_dome


# "Sky dome shape" — runtests.jl:855-882
def test_sky_dome_shape(SD):
    up = (0.0, 0.0, 1.0)
    sphere, sphere_spacing = SD.sky_dome_directions(4096, "sphere", up)
    assert sphere.shape == (4096, 3) and sphere.dtype == f32
    assert (sphere[:, 2] < 0).any()                     # covers below the horizon
    hemi, hemi_spacing = SD.sky_dome_directions(4096, "hemisphere", up)
    assert abs(hemi.shape[0] - 4096) <= 0.05 * 4096     # the cut keeps the requested count, not half of it
    assert np.isclose(hemi_spacing, math.sqrt(4 * math.pi / 8192), rtol=1e-6)
    assert hemi_spacing < sphere_spacing
    assert (hemi[:, 2] >= 0).all()                      # nothing below the horizon
    assert hemi[:, 2].min() < 0.05 and hemi[:, 2].max() > 0.95
    tilted = np.array([1, 0, 1], f32) / f32(math.sqrt(2))
    dirs, _ = SD.sky_dome_directions(2048, "hemisphere", (1.0, 0.0, 1.0))   # `up` is normalised inside
    assert ((dirs * tilted).sum(1) >= -1e-5).all()
    with pytest.raises(ValueError, match="Invalid sky dome shape"):
        SD.sky_dome_directions(64, "dome", up)
    assert np.allclose(np.linalg.norm(sphere.astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_fibonacci_sphere_is_the_test_scenes_lattice(SD):
    for n in (1, 7, 4096, 8192):
        a, sa = SD.fibonacci_sphere(n)
        b, sb = scenes.fibonacci_sphere(n)
        assert a.dtype == b.dtype == f32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert f32(sa).tobytes() == f32(sb).tobytes()


def test_radius_and_constants(SD):
    assert SD.SKY_DOME_OVERLAP == 1.0
    assert SD.sky_dome_radius(1000.0, 100.0, 3.0) == 300.0
    assert SD.sky_dome_radius(1000.0, 100.0, 20.0) == 780.0     # clamped: 0.8 · far_plane - extent
    assert np.array_equal(SD.rgb_2_sh((0.2, 0.4, 0.9)), scenes.rgb_2_sh((0.2, 0.4, 0.9)))
    assert abs(1.0 / (1.0 + math.exp(-float(SD.inverse_sigmoid(0.99)))) - 0.99) < 1e-6
    assert np.array_equal(SD.sky_hard(np.array([0.2, 0.5, 0.51], f32)), [False, False, True])


# "sky_opacity_loss" — runtests.jl:884-902, on the restatement (float64, float32 and the kernels' order)
def test_sky_opacity_loss_known_answers():
    frame = np.zeros((2, 2, 5), f32)
    frame[..., 4] = np.array([[0.9, 0.1], [0.5, 1.0]], f32)
    mask = np.array([[1, 0], [0, 1]], f32)
    sky, g = np.zeros((2, 2, 3), f32), np.zeros((2, 2, 5), f32)
    want = (f32(0.9) ** 2 + f32(1) ** 2) / f32(2)
    for dtype in (torch.float64, torch.float32):
        e = st.evaluate(frame, sky, mask, 1.0, g, dtype)
        assert np.isclose(e["loss"], want, rtol=1e-6)
        assert e["valpha"][0, 1] == 0 and e["valpha"][1, 0] == 0            # unmasked pixels are untouched
        assert e["valpha"][0, 0] > 0 and np.isclose(e["valpha"][1, 1], 2 * 1 / 2)   # the saturated pixel keeps its gradient
    r = st.restate(frame, sky, mask, 1.0, g)
    assert np.isclose(r["loss"], want, rtol=1e-6) and r["inv"] == f32(0.5)
    assert r["v4"][0, 1] == 0 and r["v4"][1, 0] == 0 and r["v4"][1, 1] == 1.0 and r["v4"][0, 0] == f32(f32(1.8) * f32(0.5))
    empty = st.restate(frame, sky, np.zeros((2, 2), f32), 1.0, g)
    assert empty["loss"] == 0.0 and empty["inv"] == 1.0 and not empty["v4"].any()   # no division by zero
    assert st.evaluate(frame, sky, np.zeros((2, 2), f32), 1.0, g)["loss"] == 0.0


@pytest.mark.parametrize("W,H,C", [(17, 3, 5), (130, 35, 8)])
def test_restatement_agrees_with_autograd(W, H, C):
    frame, sky, masks, g = st.make_case(W, H, C, seed=W)
    alpha = frame[..., 4]
    assert (alpha == 0).any() and (alpha == 1).any() and ((alpha > 0) & (alpha < 1)).any()
    assert masks["small"].sum() < 1 and not masks["zero"].any() and masks["fractional"].sum() > 1
    for kind in st.MASKS + (None,):
        mask = None if kind is None else masks[kind]
        zero4 = g.copy()
        zero4[..., 4] = 0
        r, e = st.restate(frame, sky, mask, 0.7, zero4), st.evaluate(frame, sky, mask, 0.7, g)
        assert np.allclose(r["out"][..., :3], e["comp"], atol=1e-6) and np.array_equal(r["out"][..., 3:], frame[..., 3:])
        assert np.allclose(r["vsky"], e["vsky"], atol=1e-9) and np.allclose(r["v4"], e["valpha"], rtol=1e-5, atol=1e-8)
        if mask is not None:
            assert np.isclose(r["loss"], e["loss"], rtol=1e-6, atol=0) and np.isclose(r["inv"], e["inv"], rtol=1e-6)


# merge_sky — runtests.jl:843-852
def _host_dome(SD, pkg, n=64, radius=50.0):
    dirs, spacing = SD.fibonacci_sphere(n)
    rot = np.zeros((n, 4), f32)
    rot[:, 0] = 1
    return pkg.ply.GaussianModel(dirs * f32(radius), np.tile(SD.rgb_2_sh((0.2, 0.4, 0.9)).reshape(1, 1, 3), (n, 1, 1)),
                                 np.zeros((n, 0, 3), f32), np.full((n, 3), np.log(f32(radius) * spacing), f32), rot,
                                 np.full((n, 1), SD.inverse_sigmoid(0.99), f32), 0, 0)


def test_merge_sky(SD, pkg, tmp_path):
    sc, _ = scenes.sky_test_scene()
    n = sc["means"].shape[0]
    r = np.random.default_rng(0)
    scene = pkg.ply.GaussianModel(sc["means"], sc["shs"], r.standard_normal((n, 15, 3)).astype(f32), np.log(sc["scales"]),
                                  sc["rots"], np.zeros((n, 1), f32), 2, 3)
    dome = _host_dome(SD, pkg)
    merged = SD.merge_sky(scene, SimpleNamespace(gaussians=dome))     # a SkyDome, or its model
    assert merged.n == n + dome.n and (merged.sh_degree, merged.max_sh_degree) == (2, 3)
    assert merged.features_rest.shape == (n + dome.n, 15, 3)
    assert not merged.features_rest[n:].any() and np.array_equal(merged.features_rest[:n], scene.features_rest)
    assert np.array_equal(merged.points[n:], dome.points) and np.array_equal(merged.points[:n], scene.points)   # dome last
    assert np.array_equal(merged.features_dc[n:], dome.features_dc) and np.array_equal(merged.opacities[n:], dome.opacities)
    path = str(tmp_path / "merged.ply")
    pkg.ply.export_ply(merged, path)
    back = pkg.ply.import_ply(path)
    assert back.n == merged.n and np.array_equal(back.points, merged.points) and np.array_equal(back.features_rest, merged.features_rest)
    # an isotropic scene: the dome's scales are averaged to one column
    iso = pkg.ply.GaussianModel(scene.points, scene.features_dc, scene.features_rest, scene.scales[:, :1].copy(), scene.rotations,
                                scene.opacities, 3, 3)
    m2 = SD.merge_sky(iso, dome)
    assert m2.scales.shape == (n + dome.n, 1) and np.allclose(m2.scales[n:, 0], dome.scales.mean(1), rtol=1e-6)


# the `sky.*` checkpoint group — sky_dome.jl:322-333, training.jl:435-436,463-465
class _Opt:
    def __init__(self, n, seed):
        r = np.random.default_rng(seed)
        self.mu = torch.from_numpy(r.normal(size=n).astype(f32))
        self.nu = torch.from_numpy(r.uniform(size=n).astype(f32))
        self.current_step = 7 + seed


def _trainer(pkg, n=11, kr=15):
    r = np.random.default_rng(1)
    f = lambda *s: r.normal(size=s).astype(f32)  # noqa: E731
    g = pkg.ply.GaussianModel(f(n, 3), f(n, 1, 3), f(n, kr, 3), f(n, 3), f(n, 4), f(n, 1), 2, 3)
    sizes = dict(points=3 * n, features_dc=3 * n, features_rest=n * kr * 3, opacities=n, scales=3 * n, rotations=4 * n)
    return g, {k: _Opt(v, i) for i, (k, v) in enumerate(sizes.items())}


def _dome(SD, pkg, seed, n=64):
    g = _host_dome(SD, pkg, n)
    g.features_dc = np.random.default_rng(seed).normal(size=(n, 1, 3)).astype(f32)
    return SimpleNamespace(gaussians=g, optimizer=_Opt(3 * n, seed), radius=50.0)


def test_checkpoint_sky_group(SD, pkg, tmp_path):
    ck = pkg.checkpoint
    g, opts = _trainer(pkg)
    sky = _dome(SD, pkg, 20)
    with_sky, without = str(tmp_path / "with.safetensors"), str(tmp_path / "without.safetensors")
    ck.save_state(with_sky, g, opts, step=40, sky=sky)
    ck.save_state(without, g, opts, step=40)
    c = ck.load_checkpoint(with_sky)
    n = sky.gaussians.n
    shapes = {"sky.gaussians.points": (3, n), "sky.gaussians.features_dc": (3, 1, n), "sky.gaussians.features_rest": (3, 0, n),
              "sky.gaussians.scales": (3, n), "sky.gaussians.rotations": (4, n), "sky.gaussians.opacities": (1, n),
              "sky.optimizer.mu.1": (3, 1, n), "sky.optimizer.nu.1": (3, 1, n)}
    for k, shape in shapes.items():        # the reference's keys, with their Julia shapes
        assert k in c and c.raw_tensor(k).shape == shape, k
    assert c.meta["sky.optimizer.n_moments"] == "1" and c.meta["sky.optimizer.current_step"] == "27"
    assert float(c.meta["sky.radius"]) == 50.0
    assert c.meta["sky.gaussians.sh_degree"] == "0" and c.meta["sky.gaussians.max_sh_degree"] == "0"
    assert not any(k.startswith("sky.") for k in ck.load_checkpoint(without)._keys)
    # both sides have a dome: restored in place, colours and moments included
    other = _dome(SD, pkg, 21)
    assert not np.array_equal(other.gaussians.features_dc, sky.gaussians.features_dc)
    g2, step = ck.load_state(with_sky, _trainer(pkg)[1], sky=other)
    assert step == 40 and np.array_equal(g2.points, g.points)
    assert np.array_equal(other.gaussians.features_dc, sky.gaussians.features_dc)
    assert torch.equal(other.optimizer.mu, sky.optimizer.mu) and torch.equal(other.optimizer.nu, sky.optimizer.nu)
    assert other.optimizer.current_step == 27
    # a file without the group leaves a dome as built
    fresh = _dome(SD, pkg, 22)
    dc0, mu0 = fresh.gaussians.features_dc.copy(), fresh.optimizer.mu.clone()
    ck.load_state(without, _trainer(pkg)[1], sky=fresh)
    assert np.array_equal(fresh.gaussians.features_dc, dc0) and torch.equal(fresh.optimizer.mu, mu0) and fresh.optimizer.current_step == 29
    # a trainer without a dome ignores the group
    g3, step = ck.load_state(with_sky, _trainer(pkg)[1])
    assert step == 40 and np.array_equal(g3.features_rest, g.features_rest)
    # a dome of another size is refused, not reinterpreted
    with pytest.raises(ValueError, match="Gaussians in the file"):
        ck.load_state(with_sky, _trainer(pkg)[1], sky=_dome(SD, pkg, 23, n=32))


def test_refused_calls_need_no_device(SD, pkg):
    L, lib = pkg._lib, pkg._lib.load()
    one = C.c_void_p(64)      # never dereferenced: every call below is refused on its arguments

    def fwd(W=8, H=8, Cn=5, image=one, sky=one, mask=None, out=one, loss=None, scratch=None):
        return lib.gsr_sky_composite_forward(W, H, Cn, image, sky, mask, 1.0, out, loss, scratch, None)

    def bwd(W=8, H=8, Cn=5, image=one, sky=one, mask=None, vp=C.c_void_p(128), vsky=one, scratch=None):
        return lib.gsr_sky_composite_backward(W, H, Cn, image, sky, mask, 1.0, vp, vsky, scratch, None)

    err = lambda: lib.gsr_last_error_string()  # noqa: E731
    for call in (fwd, bwd):
        assert call(Cn=3) == L.GSR_E_INVALID_ARG and b":rgbd (5) or :rgbdn (8)" in err()    # :rgb has no alpha row
        assert call(W=0) == L.GSR_E_INVALID_ARG and b"image size" in err()
        assert call(H=-1) == L.GSR_E_INVALID_ARG and b"image size" in err()
        assert call(image=None) == L.GSR_E_INVALID_ARG and b"null" in err()
        assert call(sky=None) == L.GSR_E_INVALID_ARG and b"null" in err()
    assert fwd(out=None) == L.GSR_E_INVALID_ARG and b"null" in err()
    assert fwd(mask=one, loss=None, scratch=one) == L.GSR_E_INVALID_ARG and b"needs loss_out" in err()   # a mask without loss_out
    assert fwd(mask=one, loss=one, scratch=None) == L.GSR_E_INVALID_ARG and b"needs loss_out and scratch" in err()
    assert fwd(mask=one, loss=one, scratch=C.c_void_p(68)) == L.GSR_E_INVALID_ARG and b"8-byte aligned" in err()
    assert bwd(vp=None) == L.GSR_E_INVALID_ARG and bwd(vsky=None) == L.GSR_E_INVALID_ARG
    assert bwd(vp=one) == L.GSR_E_INVALID_ARG and b"must not be the image" in err()
    assert bwd(mask=one, scratch=None) == L.GSR_E_INVALID_ARG and b"scratch" in err()
    assert lib.gsr_sky_scratch_bytes(0, 5) == 0
    assert lib.gsr_sky_scratch_bytes(32, 32) == 16 + 16 and lib.gsr_sky_scratch_bytes(33, 32) == 16 + 2 * 16
    assert SD.sky_scratch_bytes(514, 512) == 16 + 257 * 16
