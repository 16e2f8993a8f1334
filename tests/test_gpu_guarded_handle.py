"""-m gpu: GSR_DEBUG_GUARD=1 (gsr.h) — every buffer the HANDLE owns is followed by 4 KiB of guard words, checked by
gsr_debug_check_guards and whenever such a buffer is freed.  The handle's 32 buffers get their capacities from policies, scans
and estimates; GSR_DEBUG_FILL shows a read of a float that was never written, this shows a store past a capacity.

Every cell runs twice, without and with the switch, on scenes the suite already has (test_gpu_poisoned_buffers.py,
test_gpu_list_boundaries.py / list_scenes.py).  With the switch, gsr_debug_check_guards must return GSR_OK before the handle
is closed — after regrowths and releases too, whose findings the handle remembers —, and the outputs and gsr_memory_usage must
be the unguarded run's, bit for bit: the guard lies behind `cap`, nothing the library derives from a capacity moves."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import list_scenes as ls
from hip_helpers import HipRun, dev
from test_gpu_poisoned_buffers import (AUXC, CH, FWDONLY, MATRIX, TAIL, _hot_scene, _stream, assert_same, empty, make, run_view)

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def debug_guard(on):
    """GSR_DEBUG_GUARD for the handles created (and grown) inside the block; read by the library at every allocation."""
    old = os.environ.pop("GSR_DEBUG_GUARD", None)
    if on:
        os.environ["GSR_DEBUG_GUARD"] = "1"
    try:
        yield
    finally:
        os.environ.pop("GSR_DEBUG_GUARD", None)
        if old is not None:
            os.environ["GSR_DEBUG_GUARD"] = old


def guards_ok(pkg, rast):
    """gsr_debug_check_guards == GSR_OK (it names the buffer, the offset and the word otherwise); returns gsr_memory_usage."""
    lib = pkg._lib.load()
    torch.cuda.synchronize()
    rc = lib.gsr_debug_check_guards(rast._h)
    assert rc == 0, lib.gsr_last_error_string().decode()
    return int(lib.gsr_memory_usage(rast._h))


def hook(pkg):
    def check(rast, out):
        out["memory_usage"] = guards_ok(pkg, rast)
    return check


def both(run):
    """run() without and with the switch: the same outputs (memory usage among them), bit for bit."""
    with debug_guard(False):
        plain = run()
    with debug_guard(True):
        guarded = run()
    assert "memory_usage" in plain
    assert_same(plain, guarded, "GSR_DEBUG_GUARD=1")
    return plain


def view_pair(pkg, sc, **kw):
    return both(lambda: run_view(pkg, sc, None, check=hook(pkg), **kw))


class _Raw:
    """A device address as torch sees a foreign array."""
    def __init__(self, address, nbytes):
        self.__cuda_array_interface__ = dict(shape=(nbytes,), typestr="|u1", data=(address, False), version=2)


def test_a_store_behind_a_capacity_is_named(pkg):
    """The check is not vacuous: one word stored (by torch, inside the handle's own allocation) 8 bytes behind final_T's
    capacity is reported with the buffer's name, the offset and the word; a handle created without the switch has no guards."""
    L, lib = pkg._lib, pkg._lib.load()
    W, H = 17, 9
    cap = (W * H * 4 + 255) & ~255
    with debug_guard(True):
        rast = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgb")
    try:
        assert lib.gsr_debug_check_guards(rast._h) == 0
        p, nb = C.c_void_p(), C.c_size_t()
        L.check(lib.gsr_buffer(rast._h, L.BUF_FINAL_T, C.byref(p), C.byref(nb)))
        assert nb.value == W * H * 4
        mem = torch.as_tensor(_Raw(p.value, cap + 16), device="cuda")
        assert mem[cap:cap + 16].view(torch.int32).tolist() == [0x7F7F7F7F] * 4    # a float-only buffer's guard word
        mem[cap + 8:cap + 12] = 0
        torch.cuda.synchronize()
        assert lib.gsr_debug_check_guards(rast._h) == L.GSR_E_STATE
        msg = lib.gsr_last_error_string().decode()
        assert "final_T" in msg and "offset 8 " in msg and "0x00000000" in msg, msg
    finally:
        rast.close()
    rast = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgb")
    try:
        assert lib.gsr_debug_check_guards(rast._h) == 0
    finally:
        rast.close()


# ---- the cells of test_gpu_poisoned_buffers.py --------------------------------------------------------------------
@pytest.mark.parametrize("mode,bg0,prec,cot", MATRIX)
def test_path_matrix(pkg, orc, mode, bg0, prec, cot):
    sc = make(pkg, orc, mode, 2500, 101, 70, 2, 301, (0, 0, 0) if bg0 else (0.3, 0.1, 0.6))
    vp = np.random.default_rng(7).standard_normal((sc.H, sc.W, CH[mode])).astype(np.float32)
    out = view_pair(pkg, sc, prec=prec, warm=60000, vp=vp, loss=cot == "loss", views=2)
    assert out["route"] == (True, False)


@pytest.mark.parametrize("prec", [None, "accurate"])
@pytest.mark.parametrize("mode", ["rgb", "rgbd", "rgbdn"])
def test_hot_tiles_in_all_three_tiers(pkg, orc, mode, prec):
    sc = _hot_scene(pkg, orc, mode, mode != "rgbd")
    vp = np.random.default_rng(58).standard_normal((sc.H, sc.W, CH[mode])).astype(np.float32)
    out = view_pair(pkg, sc, prec=prec, vp=vp)
    assert all(x > 0 for x in out["stats"][2]), out["stats"]


def test_compact_binning_1(pkg, orc):
    sc = make(pkg, orc, "rgb", 2500, 101, 70, 2, 303, (0.3, 0.1, 0.6))
    vp = np.random.default_rng(5).standard_normal((sc.H, sc.W, 3)).astype(np.float32)
    out = view_pair(pkg, sc, budget=1, vp=vp, warm=60000)
    assert out["stats"][1] == 1


def test_compact_binning_2(pkg, orc):
    W, H, n, deg = 640, 416, 30000, 1
    s = pkg.synthetic.make_scene(n, W, H, deg, 67)
    for i, k in enumerate(("dense:0.01:70", "dense:0.005:190", "hot:9000")):
        s = pkg.synthetic.add_skew(s, k, seed=68 + i)
    from test_gpu_poisoned_buffers import Scene
    sc = Scene(means=s.means, shs=s.shs, opac=s.opacities, scales=s.scales, rots=s.rotations, cam=orc.Camera(W, H, s.focal),
               deg=deg, bg=(0.0, 0.0, 0.0), mode="rgb", W=W, H=H, seed=69)
    vp = np.random.default_rng(5).standard_normal((H, W, 3)).astype(np.float32)
    out = view_pair(pkg, sc, budget=(40 * 26 + 1) * 8 * 1536, vp=vp, views=2)
    assert out["stats"][1] == 2 and sum(out["stats"][2]) > 0, out["stats"]


@pytest.mark.parametrize("mode,warm", AUXC)
def test_covisibilities_and_uncertainties(pkg, orc, mode, warm):
    sc = make(pkg, orc, mode, 2000, 101, 70, 0, 305, (0.2, 0.2, 0.2))
    vp = np.random.default_rng(6).standard_normal((sc.H, sc.W, CH[mode])).astype(np.float32)
    out = view_pair(pkg, sc, vp=vp, warm=50000 if warm else 0, views=2 if warm else 1, aux_prior=np.zeros(2000, np.uint8))
    assert out["route"] == (warm, not warm)


@pytest.mark.parametrize("mode,aux", FWDONLY)
def test_forward_only(pkg, orc, mode, aux):
    sc = make(pkg, orc, mode, 2000, 101, 70, 1, 307, (0.0, 0.0, 0.0))
    out = view_pair(pkg, sc, forward_only=True, aux_prior=np.zeros(2000, np.uint8) if aux else None, views=2)
    assert out["route"] == (True, False)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_pose_gradient(pkg, orc, n):
    """pose_part: 12 partial sums per 256-row workgroup of pergauss_bwd — one workgroup, exactly one, one row into the next."""
    sc = make(pkg, orc, "rgbd", n, 101, 70, 2, 309, (0.0, 0.0, 0.0), view=1)
    vp = np.random.default_rng(3).standard_normal((sc.H, sc.W, 5)).astype(np.float32)
    out = view_pair(pkg, sc, vp=vp, pose=True)
    assert torch.isfinite(out["vR"]).all() and out["vR"].abs().sum() > 0


@pytest.mark.parametrize("mode,color", TAIL)
def test_backward_trainer_tail(pkg, mode, color):
    W, H, n, deg = 101, 70, 1500, 2
    s = pkg.synthetic.make_scene(n, W, H, deg, 77, sigma_px=5.0)
    s.means[::7, 2] = -1.0
    cam = pkg.Camera(W, H, tuple(s.focal))
    R, O = pkg.rasterizer, pkg.optim
    target = dev(np.random.default_rng(3).uniform(0, 1, (3, H, W)).astype(np.float32))

    def run():
        raw = dict(points=dev(s.means), features_dc=dev(s.shs[:, :1].copy()), features_rest=dev(s.shs[:, 1:].copy()),
                   opacities=dev(s.opacities_raw.reshape(-1, 1)), scales=dev(s.scales_raw), rotations=dev(s.rotations))
        opts = {k: O.Adam(raw[k], 1e-3, eps=1e-15) for k in O.GROUPS}
        act = list(R.prologue_forward(raw["features_dc"], raw["features_rest"], raw["opacities"], raw["scales"]))
        rast = R.GaussianRasterizer(W, H, mode=mode, form_tuner=False)
        try:
            for _ in range(2):
                img = rast.forward_raw(raw["points"], *act, raw["rotations"], cam, deg, (0.0, 0.0, 0.0))
                lo, vp = empty(1, fill=None), empty(H, W, CH[mode], fill=None)
                pkg._lib.check(pkg._lib.load().gsr_loss_l1_ssim(rast._h, img.data_ptr(), target.data_ptr(), 0.2, lo.data_ptr(),
                                                                vp.data_ptr(), _stream()))
                O.fused_backward_tail_step(rast, vp, opts, raw, *act, cam, deg, (0.0, 0.0, 0.0),
                                           forward_generation=rast.stats.generation, color_cotangent=color)
            return dict(raw=[raw[k].clone() for k in O.GROUPS], mu=[opts[k].mu.clone() for k in O.GROUPS], act=[a.clone() for a in act],
                        vmeans2d=rast.gstate.grad_means_2d.clone(), loss=lo.clone(), memory_usage=guards_ok(pkg, rast))
        finally:
            rast.close()

    both(run)


# ---- tile lists of a chosen length (list_scenes.py) ---------------------------------------------------------------------
def _views(pkg, scenes, mode="rgb", reserve=None, release_before_last=False, **kw):
    """The scenes in turn on ONE handle (forward + backward each); the outputs of the last view and the handle's history."""
    first = scenes[0]
    run = HipRun(pkg, *first.args, first.cam, first.deg, (0.3, 0.1, 0.6), mode, **kw)
    try:
        if reserve:
            run.rast.reserve(*reserve)
        for k, sc in enumerate(scenes):
            if release_before_last and k == len(scenes) - 1:
                run.rast.release_scene_buffers()
            run.t = [dev(sc.means), dev(sc.shs), dev(np.asarray(sc.opac).reshape(-1, 1)), dev(sc.scales), dev(sc.rots)]
            img = run.forward().clone()
            vp = np.random.default_rng(len(sc.means)).standard_normal(tuple(img.shape)).astype(np.float32)
            g = run.backward(vp)
        s = run.rast.stats
        return dict(image=img, final_T=run.rast.accum_alpha, n_contrib=run.rast.n_contrib, grads=[x.clone() for x in g[:5]],
                    vmeans2d=run.rast.grad_means_2d.clone(), n_rendered=int(s.n_rendered), bin_capacity=int(s.bin_capacity),
                    compact=int(s.compact_binning), regrowths=int(s.scratch_regrowths), tiers=tuple(int(x) for x in s.tier_tiles),
                    memory_usage=guards_ok(pkg, run.rast))
    finally:
        run.rast.close()


@pytest.mark.parametrize("L", [1024, 1025, 4096, 4097, 8192, 8193])
def test_list_length_on_each_side_of_a_tier(pkg, L):
    """One 16 x 16 tile whose list has L entries, twice (the second view is the fused kernel's or, past 1024, the tier
    launches'): the per-instance buffers are exactly as long as the first view sized them."""
    sc = ls.single_tile_scene(L, 7)
    out = both(lambda: _views(pkg, [sc, sc]))
    assert out["n_rendered"] == L and out["tiers"] == (int(1024 < L <= 4096), int(4096 < L <= 8192), int(L > 8192))


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("L1", sorted(ls.BIN_FIRST_VIEWS))
def test_bin_capacity_edges(pkg, L1, delta):
    """Two views of L1 entries settle the bins' capacity; the third fills the bin to one short of, exactly, and one past its
    last slot (test_gpu_list_boundaries.py)."""
    cap = ls.BIN_FIRST_VIEWS[L1]
    assert pkg._lib.load().gsr_bins_capacity_after(L1, L1, 16, 16, 0, cap) == cap      # the second view leaves it alone
    a, b = ls.single_tile_scene(L1, 7), ls.single_tile_scene(cap + delta, 7)
    out = both(lambda: _views(pkg, [a, a, b]))
    assert out["bin_capacity"] == cap and out["n_rendered"] == cap + delta
    assert out["compact"] == (0 if delta <= 0 else 2 if cap >= 1024 else 1)


def test_regrowth_small_then_large_n(pkg, orc):
    """ONE handle: the per-Gaussian buffers of 300 Gaussians are freed (their guards checked at the free) and regrown for
    6000; then released and grown again."""
    a = make(pkg, orc, "rgbdn", 300, 101, 70, 2, 325, (0.1, 0.2, 0.3))
    b = make(pkg, orc, "rgbdn", 6000, 101, 70, 2, 323, (0.1, 0.2, 0.3), sigma_px=5.0)

    def run(release):
        def go():
            scenes = [_as_list_scene(a), _as_list_scene(b)] + ([_as_list_scene(b)] if release else [])
            return _views(pkg, scenes, mode="rgbdn", exact_tile_cull=True, release_before_last=release)
        return go

    out = both(run(False))
    assert out["regrowths"] > 0
    both(run(True))


def test_regrowth_short_then_long_lists(pkg):
    """ONE handle: the per-instance buffers sized by a 100-entry list regrow for 5000 entries (a tier list)."""
    a, b = ls.single_tile_scene(100, 7), ls.single_tile_scene(5000, 7)
    out = both(lambda: _views(pkg, [a, a, b, b]))
    assert out["regrowths"] > 0 and out["n_rendered"] == 5000


def _as_list_scene(sc):
    import types
    return types.SimpleNamespace(means=sc.means, shs=sc.shs, opac=np.asarray(sc.opac), scales=sc.scales, rots=sc.rots, cam=sc.cam,
                                 deg=sc.deg, args=(sc.means, sc.shs, np.asarray(sc.opac), sc.scales, sc.rots))


def test_reserve_at_exactly_the_instance_count(pkg, orc):
    """gsr_reserve(n, D) with D the view's own instance count: the sorted ids, the stream planes and the gradient rows hold
    the view with no slack at all."""
    sc = _as_list_scene(make(pkg, orc, "rgbd", 2000, 101, 70, 1, 329, (0.5, 0.5, 0.5)))
    D = _views(pkg, [sc], mode="rgbd", exact_tile_cull=True)["n_rendered"]
    assert D > 0
    out = both(lambda: _views(pkg, [sc, sc], mode="rgbd", exact_tile_cull=True, reserve=(2000, D)))
    assert out["n_rendered"] == D


@pytest.mark.parametrize("prec", ["fast", "exact"])
@pytest.mark.parametrize("W,H", [(17, 9), (130, 70)])
def test_loss_head(pkg, W, H, prec):
    """d0, d1, d2 and the per-wave partials: fewer tiles than the grid's lanes, and more than two SSIM strips each way."""
    L = pkg._lib
    r = np.random.default_rng(W)
    img, tgt = dev(r.uniform(0, 1, (H, W, 5)).astype(np.float32)), dev(r.uniform(0, 1, (3, H, W)).astype(np.float32))

    def run():
        rast = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgbd", ssim_precision=prec)
        try:
            lo, vpx = empty(1, fill=None), empty(H, W, 5, fill=None)
            L.check(L.load().gsr_loss_l1_ssim(rast._h, img.data_ptr(), tgt.data_ptr(), 0.2, lo.data_ptr(), vpx.data_ptr(), _stream()))
            return dict(loss=lo.clone(), vpix=vpx.clone(), memory_usage=guards_ok(pkg, rast))
        finally:
            rast.close()

    out = both(run)
    assert torch.isfinite(out["loss"]).all() and not out["vpix"][:, :, 3:].view(torch.int32).any()
