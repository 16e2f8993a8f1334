"""-m gpu: the C ABI with every caller-provided pointer inside a guarded arena (tests/guarded.py).

torch's caching allocator rounds every request up to 512 bytes inside a segment of megabytes, so a kernel that loads or stores
a few elements past an array neither faults nor, as a rule, changes a compared value.  The callers of include/gsr.h pack their
arrays differently.  Here every case runs FIVE times on identical inputs — plain (each buffer its own torch allocation, as the
rest of the suite), and the two placements ("aligned": 16-byte aligned data pointers, the vector paths; "worst": the weakest
alignment the interface allows, the scalar paths of sh_rows.h / trainer.hip) times the two guard fills — and asserts
  1. every call returns GSR_OK;
  2. no guard word changed (a store outside an array);
  3. every output, in-place buffer and returned scalar is bit-identical in all five runs (a load outside an array follows the
     guard fill; the library has no float atomics, so there is no exception);
  4. every const input still holds what it was given.
Scratch is exactly gsr_*_scratch_bytes(...) long.  Integer buffers whose elements become rows, counts or bounds are guarded by
two in-range values (guarded.py), never by a poison word.

entry point                                   test
--------------------------------------------  ---------------------------------------------------------------
gsr_forward, gsr_backward                     test_forward_backward (three modes; accurate; forward-only; nothing visible)
gsr_loss_l1_ssim                              test_forward_backward (fast and exact SSIM on the guarded image)
gsr_update_stats, gsr_copy_buffer             test_forward_backward
gsr_ssim_forward, gsr_ssim_backward           test_ssim_planar
gsr_prologue_forward, gsr_prologue_backward   test_prologue
gsr_adam_step                                 test_adam_six_odd_groups
gsr_trainer_tail_step                         test_trainer_tail_step
gsr_backward_trainer_tail                     test_backward_trainer_tail
gsr_sh_grad_from_views, ..._tail              test_sh_grad_from_views_and_tail
gsr_mask_findall, gsr_gather_rows             test_mask_findall_and_gather
gsr_compose_rows                              test_compose_rows
gsr_densify_grad_mean, gsr_densify_mask       test_densify_grad_mean_and_masks
gsr_split_transform, gsr_reset_opacity,
gsr_morton_codes, gsr_count_nonfinite         test_split_reset_morton_nonfinite
gsr_ply_pack_rows, gsr_ply_unpack_rows        test_ply_rows
gsr_bilateral_slice_forward / _backward,
gsr_bilateral_tv, gsr_bilateral_adam_tail     test_bilateral
gsr_normal_loss_forward / _backward           test_normal_loss
gsr_flatten_loss                              test_flatten_loss
gsr_depth_target, gsr_depth_loss_forward /
_backward                                     test_depth_loss
gsr_mcmc_weights, gsr_mcmc_sample,
gsr_mcmc_split_sampled, gsr_mcmc_relocate_rows test_mcmc_relocation_round
gsr_mcmc_sample (all weights zero)            test_mcmc_sample_without_weight_writes_nothing
gsr_mcmc_relocation_params                    test_mcmc_relocation_params
gsr_mcmc_inject_noise                         test_mcmc_inject_noise
gsr_mcmc_regularization                       test_mcmc_regularization
gsr_stream_triad                              test_stream_triad
(gsr_allreduce_grads needs a communicator: not here.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_torch as gt
from guarded import placements
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu

I32, I64, U8, F32 = torch.int32, torch.int64, torch.uint8, torch.float32
ROWS = (1, 63, 65, 257, 1031)


def ptr(t):
    return None if t is None else t.data_ptr()


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.uint8) if t.numel() else t


def _five_runs(pkg, case, nbytes=4 << 20):
    lib = pkg._lib.load()
    ref, ref_tag = None, None
    for P in placements(nbytes, "cuda"):
        tag = f"{P.skew}/{P.fill}"

        def ok(rc, what=""):
            assert rc == 0, (tag, what, rc, lib.gsr_last_error_string().decode())

        out = case(P, ok)
        torch.cuda.synchronize()
        found = P.check()
        assert found == [], (tag, found)
        P.assert_inputs_unchanged()
        flat = {}
        for k, v in out.items():
            if isinstance(v, (list, tuple)):
                for i, x in enumerate(v):
                    flat[f"{k}[{i}]"] = x
            else:
                flat[k] = v
        flat = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in flat.items()}
        if ref is None:
            ref, ref_tag = flat, tag
            continue
        assert flat.keys() == ref.keys()
        for k, v in flat.items():
            if isinstance(v, torch.Tensor):
                a, b = bits(v), bits(ref[k])
                assert a.shape == b.shape, (tag, k)
                if not torch.equal(a, b):
                    d = (a.reshape(-1) != b.reshape(-1)).nonzero()
                    raise AssertionError(f"{k} [{tag}]: {d.numel()} bytes differ from the {ref_tag} run, first at byte {int(d[0])}")
            else:
                assert v == ref[k], (tag, k, v, ref[k])
    return ref


def scratch(P, name, nbytes, dtype=F32, align=None):
    """Caller-owned scratch of EXACTLY nbytes bytes."""
    item = torch.empty(0, dtype=dtype).element_size()
    assert nbytes % item == 0, (name, nbytes)
    return P.place(name, (nbytes // item,), dtype, align=align, role="scratch")


def f32(r, *shape, lo=-1.0, hi=1.0):
    return r.uniform(lo, hi, shape).astype(np.float32)


def model_arrays(r, n, k_rest, sd):
    """Raw trainer arrays in GROUPS order: points, features_dc, features_rest, opacities, scales, rotations."""
    return [f32(r, n, 3) + np.float32([0, 0, 6]), f32(r, n, 1, 3), f32(r, n, k_rest, 3), f32(r, n, 1), f32(r, n, sd) - 3.0,
            f32(r, n, 4)]


# ---------------------------------------------------------------------------------------------------------------------
# gsr_forward / gsr_loss_l1_ssim / gsr_copy_buffer / gsr_backward / gsr_update_stats
FB = [
    # mode, n, (W, H), K, deg, prec, ssim, variant
    ("rgb", 1, (55, 33), 1, 0, None, "fast", ""),
    ("rgb", 257, (55, 33), 4, 1, "accurate", "exact", ""),
    ("rgb", 1031, (130, 70), 16, 3, None, "exact", "factored"),
    ("rgbd", 1031, (130, 70), 16, 2, None, "fast", "pose"),            # active degree below the stored one
    ("rgbd", 257, (130, 70), 4, 1, "accurate", "exact", "factored"),
    ("rgbd", 257, (55, 33), 4, 1, None, "fast", "nothing_visible"),
    ("rgbdn", 1031, (55, 33), 4, 1, None, "exact", "loss_cotangent"),
    ("rgbdn", 257, (130, 70), 1, 0, "accurate", "fast", "pose"),
    ("rgbdn", 1031, (130, 70), 16, 3, None, "fast", "forward_only"),
    ("rgbdn", 1, (130, 70), 4, 1, None, "exact", ""),
]
CH = {"rgb": 3, "rgbd": 5, "rgbdn": 8}


@pytest.mark.parametrize("mode,n,wh,K,deg,prec,ssim,variant", FB)
def test_forward_backward(pkg, mode, n, wh, K, deg, prec, ssim, variant):
    L, lib = pkg._lib, pkg._lib.load()
    (W, H), Cn = wh, CH[mode]
    s = pkg.synthetic.make_scene(n, W, H, deg, 400 + n + W, sigma_px=4.0, K=K)
    means = s.means.copy()
    if variant == "nothing_visible":
        means[:, 2] = -3.0
    Rm, tv = pkg.synthetic.view_pose(3)
    camera = pkg.Camera(W, H, tuple(s.focal), (0.5, 0.5), np.asarray(Rm), np.asarray(tv))
    r = np.random.default_rng(n + W)
    vp_host = r.standard_normal((H, W, Cn)).astype(np.float32)
    target = pkg.synthetic.make_target(W, H, n)
    pose, factored, fwd_only = variant == "pose", variant == "factored", variant == "forward_only"

    def case(P, ok):
        rast = pkg.rasterizer.GaussianRasterizer(W, H, mode=mode, grad_precision=prec, ssim_precision=ssim, form_tuner=False)
        try:
            t = dict(means=P.place("means", means), shs=P.place("shs", s.shs), opac=P.place("opacities", s.opacities.reshape(n, 1)),
                     scales=P.place("scales", s.scales), rots=P.place("rotations", s.rotations, align=16))
            Rd = td = None
            if pose:
                Rd = P.place("R_dev", np.asarray(Rm, np.float32).T.copy())
                td = P.place("t_dev", np.asarray(tv, np.float32))
            inp = L.Inputs(n, K, deg, ptr(t["means"]), ptr(t["shs"]), ptr(t["opac"]), ptr(t["scales"]), ptr(t["rots"]),
                           (C.c_float * 3)(0.1, 0.2, 0.3))
            cs = rast._camera(camera, Rd, td)
            img = P.place("image_out", (H, W, Cn))
            covis = P.place("covisibilities", np.zeros(n, np.uint8), role="inout", guard=(0, 1))
            unc = P.place("uncertainties", (H, W))
            radii = P.place("radii", (n,), I32, guard=(0, 1))
            aux = L.Aux(ptr(covis), ptr(unc), ptr(radii), L.FORWARD_ONLY if fwd_only else 0, 0)
            stats = L.Stats()
            ok(lib.gsr_forward(rast._h, C.byref(inp), C.byref(cs), ptr(img), C.byref(aux), _stream(), C.byref(stats)), "forward")
            out = dict(image=img, covis=covis, unc=unc, radii=radii, n_rendered=int(stats.n_rendered), n_visible=int(stats.n_visible))
            if variant == "nothing_visible":
                assert stats.n_rendered == 0
            elif n > 1:
                assert stats.n_rendered > 0
            # the loss head on the guarded image
            tgt = P.place("target", target)
            loss, vpx = P.place("loss_out", (1,)), P.place("vpixels_loss", (H, W, Cn))
            ok(lib.gsr_loss_l1_ssim(rast._h, ptr(img), ptr(tgt), 0.2, ptr(loss), ptr(vpx), _stream()), "loss")
            out.update(loss=loss, vpix=vpx)
            # two handle buffers of different element size into caller memory
            for which, name in ((L.BUF_FINAL_T, "final_T"), (L.BUF_TILE_RANGES, "tile_ranges")):
                p, nb = C.c_void_p(), C.c_size_t()
                ok(lib.gsr_buffer(rast._h, which, C.byref(p), C.byref(nb)), name)
                item, dt = (4, F32) if which == L.BUF_FINAL_T else (8, I64)
                assert nb.value and nb.value % item == 0
                dst = P.place("copy_" + name, (nb.value // item,), dt, guard=(0, 1))
                ok(lib.gsr_copy_buffer(rast._h, which, ptr(dst), nb.value, _stream()), "copy " + name)
                out[name] = dst
            if fwd_only:
                return out
            color = variant == "loss_cotangent"
            vp = vpx if color else P.place("vpixels", vp_host)
            g = dict(vmeans=P.place("vmeans", (n, 3)), vopac=P.place("vopacities", (n, 1)), vscales=P.place("vscales", (n, 3)),
                     vrot=P.place("vrotations", (n, 4), align=16), vmeans2d=P.place("vmeans2d", (n, 2)))
            g["vsh"] = P.place("vcolors", (n, 3)) if factored else P.place("vshs", (n, K, 3))
            vR = P.place("vR", (3, 3)) if pose else None
            vt = P.place("vt", (3,)) if pose else None
            gs = L.Grads(ptr(g["vmeans"]), None if factored else ptr(g["vsh"]), ptr(g["vopac"]), ptr(g["vscales"]), ptr(g["vrot"]),
                         ptr(vR), ptr(vt), ptr(g["vsh"]) if factored else None, ptr(g["vmeans2d"]), int(stats.generation),
                         L.GRADS_COLOR_COTANGENT if color else 0, 0)
            ok(lib.gsr_backward(rast._h, C.byref(inp), C.byref(cs), ptr(vp), C.byref(gs), _stream()), "backward")
            out.update(g)
            if pose:
                out.update(vR=vR, vt=vt)
            mr = P.place("max_radii", np.arange(n, dtype=np.int32) % 7, role="inout", guard=(0, 1))
            acc = P.place("accum", f32(np.random.default_rng(5), n, lo=0.0), role="inout")
            den = P.place("denom", np.ones(n, np.float32), role="inout")
            ok(lib.gsr_update_stats(rast._h, ptr(mr), ptr(acc), ptr(den), _stream()), "update_stats")
            out.update(max_radii=mr, accum=acc, denom=den)
            torch.cuda.synchronize()
            return out
        finally:
            torch.cuda.synchronize()
            rast.close()

    ref = _five_runs(pkg, case)
    if variant == "nothing_visible":
        assert not ref["image"].view(I32).any() and not ref["vmeans"].view(I32).any()
    if not fwd_only and mode != "rgb":
        assert not ref["vpix"][:, :, 3:].view(I32).any()


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("B,CHn,W,H", [(2, 3, 17, 9), (1, 1, 1, 1), (1, 1, 130, 70), (2, 3, 55, 33)])
def test_ssim_planar(pkg, B, CHn, W, H, exact):
    lib = pkg._lib.load()
    r = np.random.default_rng(W * H + B)
    shape = (B, CHn, H, W)
    img, refi, dmap = (f32(r, *shape, lo=0.0) for _ in range(3))

    def case(P, ok):
        i, rf, dm = P.place("img", img), P.place("ref", refi), P.place("dL_dmap", dmap)
        m, d0, d1, d2, gi = (P.place(k, shape) for k in ("ssim_map", "dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12", "dL_dimg"))
        ok(lib.gsr_ssim_forward(W, H, CHn, B, ptr(i), ptr(rf), 0.01 ** 2, 0.03 ** 2, 1, ptr(m), ptr(d0), ptr(d1), ptr(d2), _stream()))
        ok(lib.gsr_ssim_backward(W, H, CHn, B, ptr(i), ptr(rf), ptr(dm), ptr(d0), ptr(d1), ptr(d2), ptr(gi), _stream()))
        return dict(m=m, d0=d0, d1=d1, d2=d2, grad=gi)

    with pkg.fused_ssim.exact_arithmetic(exact):
        ref = _five_runs(pkg, case)
    assert torch.isfinite(ref["m"]).all() and torch.isfinite(ref["grad"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# the trainer tail
TAILS = [(63, 0, 1), (257, 3, 3), (1031, 15, 3), (65, 3, 1), (1, 15, 3)]


@pytest.mark.parametrize("n,k_rest,sd", TAILS)
def test_prologue(pkg, n, k_rest, sd):
    lib = pkg._lib.load()
    r = np.random.default_rng(n + k_rest)
    _, dc, rest, op, sc, _ = model_arrays(r, n, k_rest, sd)
    vshs, vo, vs = f32(r, n, k_rest + 1, 3), f32(r, n, 1), f32(r, n, 3)

    def case(P, ok):
        d, o, s_ = P.place("sh_color", dc), P.place("opacities", op), P.place("scales", sc)
        rs = P.place("sh_remainder", rest) if k_rest else None
        shs, oa, sa = P.place("shs", (n, k_rest + 1, 3)), P.place("opacities_act", (n, 1)), P.place("scales_act", (n, 3))
        ok(lib.gsr_prologue_forward(n, k_rest, sd, ptr(d), ptr(rs), ptr(o), ptr(s_), ptr(shs), ptr(oa), ptr(sa), _stream()), "fwd")
        v1, v2, v3 = P.place("vshs", vshs), P.place("vopacities_act", vo), P.place("vscales_act", vs)
        vdc, vop, vsc = P.place("v_sh_color", (n, 1, 3)), P.place("v_opacities", (n, 1)), P.place("v_scales", (n, sd))
        vrest = P.place("v_sh_remainder", (n, k_rest, 3)) if k_rest else None
        ok(lib.gsr_prologue_backward(n, k_rest, sd, ptr(oa), ptr(sa), ptr(v1), ptr(v2), ptr(v3), ptr(vdc), ptr(vrest), ptr(vop),
                                     ptr(vsc), _stream()), "bwd")
        out = dict(shs=shs, oa=oa, sa=sa, vdc=vdc, vop=vop, vsc=vsc)
        if k_rest:
            out["vrest"] = vrest
        return out

    ref = _five_runs(pkg, case)
    assert torch.equal(ref["shs"][:, :1].cpu(), torch.from_numpy(dc))


def test_adam_six_odd_groups(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    counts = (1, 63, 65, 257, 1031, 771)
    r = np.random.default_rng(6)
    host = [[f32(r, c) for _ in range(2)] + [f32(r, c, lo=0.0, hi=0.1)] + [f32(r, c)] for c in counts]   # theta, mu, nu, grad

    def case(P, ok):
        groups, keep = [], []
        for k, (c, (th, mu, nu, gr)) in enumerate(zip(counts, host)):
            a = [P.place(f"theta{k}", th, role="inout"), P.place(f"grad{k}", gr), P.place(f"mu{k}", mu, role="inout"),
                 P.place(f"nu{k}", nu, role="inout")]
            keep.append(a)
            groups.append(L.AdamGroup(ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), c, 1e-2 * (k + 1), 3 + k))
        arr = (L.AdamGroup * 6)(*groups)
        ok(lib.gsr_adam_step(arr, 6, 0.9, 0.999, 1e-15, _stream()))
        return dict(theta=[a[0] for a in keep], mu=[a[2] for a in keep], nu=[a[3] for a in keep])

    ref = _five_runs(pkg, case)
    assert not torch.equal(ref["theta[4]"].cpu(), torch.from_numpy(host[4][0]))


def _place_trainer(P, lib, ok, L, arrays, n, k_rest, sd, r_seed):
    """θ, μ, ν of the six groups + the activated copies (made by gsr_prologue_forward from θ) + a filled gsr_tail_state."""
    r = np.random.default_rng(r_seed)
    names = ("points", "features_dc", "features_rest", "opacities", "scales", "rotations")
    theta, mu, nu = [], [], []
    for k, (nm, a) in enumerate(zip(names, arrays)):
        if a.size == 0:
            theta.append(None); mu.append(None); nu.append(None)
            r.random(2)
            continue
        al = 16 if nm == "rotations" else None
        theta.append(P.place(nm, a, role="inout", align=al))
        mu.append(P.place("mu_" + nm, f32(r, *a.shape, lo=-0.1, hi=0.1), role="inout"))
        nu.append(P.place("nu_" + nm, f32(r, *a.shape, lo=0.0, hi=0.01), role="inout"))
    shs, oa, sa = (P.place("shs", (n, k_rest + 1, 3), role="inout"), P.place("opacities_act", (n, 1), role="inout"),
                   P.place("scales_act", (n, 3), role="inout"))
    ok(lib.gsr_prologue_forward(n, k_rest, sd, ptr(theta[1]), ptr(theta[2]), ptr(theta[3]), ptr(theta[4]), ptr(shs), ptr(oa), ptr(sa),
                                _stream()), "prologue")
    st = L.TailState()
    for g in range(6):
        st.theta[g], st.mu[g], st.nu[g] = ptr(theta[g]), ptr(mu[g]), ptr(nu[g])
        st.lr[g], st.current_step[g] = 1e-3 * (g + 1), 2 + g
    st.beta1, st.beta2, st.eps, st.scale_dims = 0.9, 0.999, 1e-15, sd
    st.shs, st.opacities_act, st.scales_act = ptr(shs), ptr(oa), ptr(sa)
    live = [g for g in range(6) if theta[g] is not None]
    outs = dict(theta=[theta[g] for g in live], mu=[mu[g] for g in live], nu=[nu[g] for g in live], shs=shs, oa=oa, sa=sa)
    return st, theta, mu, nu, outs


@pytest.mark.parametrize("n,k_rest,sd", TAILS)
def test_trainer_tail_step(pkg, n, k_rest, sd):
    L, lib = pkg._lib, pkg._lib.load()
    r = np.random.default_rng(n * 3 + k_rest)
    arrays = model_arrays(r, n, k_rest, sd)
    K = k_rest + 1
    gh = dict(vmeans=f32(r, n, 3), vshs=f32(r, n, K, 3), vopacities=f32(r, n, 1), vscales=f32(r, n, 3), vrotations=f32(r, n, 4))

    def case(P, ok):
        st, theta, mu, nu, outs = _place_trainer(P, lib, ok, L, arrays, n, k_rest, sd, 11)
        g = {k: P.place(k, v) for k, v in gh.items()}
        tg = L.TailGrads(ptr(g["vmeans"]), ptr(g["vshs"]), ptr(g["vopacities"]), ptr(g["vscales"]), ptr(g["vrotations"]))
        vp6 = C.c_void_p * 6
        ok(lib.gsr_trainer_tail_step(n, k_rest, sd, C.byref(tg), vp6(*[ptr(x) for x in theta]), vp6(*[ptr(x) for x in mu]),
                                     vp6(*[ptr(x) for x in nu]), st.lr, st.current_step, 0.9, 0.999, 1e-15, st.shs, st.opacities_act,
                                     st.scales_act, _stream()), "tail")
        return outs

    ref = _five_runs(pkg, case)
    assert not torch.equal(ref["theta[0]"].cpu(), torch.from_numpy(arrays[0]))


@pytest.mark.parametrize("mode,n,wh,k_rest,deg", [("rgb", 257, (55, 33), 3, 1), ("rgbd", 1031, (130, 70), 15, 2), ("rgbdn", 65, (55, 33), 0, 0)])
def test_backward_trainer_tail(pkg, mode, n, wh, k_rest, deg):
    """The fused step with θ, μ, ν of the six groups and the activated copies at 4 mod 16 (rotations at 16 mod 32, as the
    interface demands): the scalar branches of tail_sh_group and store_sh_rows (sh_rows.h)."""
    L, lib = pkg._lib, pkg._lib.load()
    (W, H), Cn, K = wh, CH[mode], k_rest + 1
    s = pkg.synthetic.make_scene(n, W, H, deg, 500 + n, sigma_px=5.0, K=K)
    s.means[::7, 2] = -1.0
    arrays = [s.means, s.shs[:, :1].copy(), s.shs[:, 1:].copy(), s.opacities_raw.reshape(n, 1), s.scales_raw, s.rotations]
    camera = pkg.Camera(W, H, tuple(s.focal))
    vp_host = np.random.default_rng(n).standard_normal((H, W, Cn)).astype(np.float32)

    def case(P, ok):
        rast = pkg.rasterizer.GaussianRasterizer(W, H, mode=mode, form_tuner=False)
        try:
            st, theta, mu, nu, outs = _place_trainer(P, lib, ok, L, arrays, n, k_rest, 3, 12)
            inp = L.Inputs(n, K, deg, ptr(theta[0]), st.shs, st.opacities_act, st.scales_act, ptr(theta[5]), (C.c_float * 3)(0, 0, 0))
            cs = rast._camera(camera, None, None)
            img, radii = P.place("image_out", (H, W, Cn)), P.place("radii", (n,), I32, guard=(0, 1))
            aux, stats = L.Aux(None, None, ptr(radii), 0, 0), L.Stats()
            ok(lib.gsr_forward(rast._h, C.byref(inp), C.byref(cs), ptr(img), C.byref(aux), _stream(), C.byref(stats)), "forward")
            assert stats.n_rendered > 0
            vp, vm2 = P.place("vpixels", vp_host), P.place("vmeans2d", (n, 2))
            st.vmeans2d, st.forward_generation, st.flags = ptr(vm2), int(stats.generation), 0
            ok(lib.gsr_backward_trainer_tail(rast._h, C.byref(inp), C.byref(cs), ptr(vp), C.byref(st), _stream()), "fused tail")
            torch.cuda.synchronize()
            return dict(outs, image=img, radii=radii, vmeans2d=vm2)
        finally:
            torch.cuda.synchronize()
            rast.close()

    ref = _five_runs(pkg, case)
    assert not torch.equal(ref["theta[1]"].cpu(), torch.from_numpy(arrays[1]))


@pytest.mark.parametrize("n,K,deg,V", [(257, 4, 1, 1), (1031, 16, 3, 3), (63, 16, 2, 3), (1, 1, 0, 1)])
def test_sh_grad_from_views_and_tail(pkg, n, K, deg, V):
    L, lib = pkg._lib, pkg._lib.load()
    r = np.random.default_rng(n + V)
    arrays = model_arrays(r, n, K - 1, 3)
    centers, vc = f32(r, V, 3), f32(r, V, n, 3)
    vc[r.random((V, n)) < 0.2] = 0.0
    small = dict(vmeans=f32(r, n, 3), vopacities=f32(r, n, 1), vscales=f32(r, n, 3), vrotations=f32(r, n, 4))

    def case(P, ok):
        cc, vcd = P.place("camera_centers", centers), P.place("vcolors_all", vc)
        means = P.place("means", arrays[0])
        vshs = P.place("vshs", (n, K, 3))
        ok(lib.gsr_sh_grad_from_views(n, K, deg, V, ptr(cc), ptr(means), ptr(vcd), ptr(vshs), _stream()), "views")
        st, theta, mu, nu, outs = _place_trainer(P, lib, ok, L, arrays, n, K - 1, 3, 13)
        g = {k: P.place(k, v) for k, v in small.items()}
        tg = L.TailGrads(ptr(g["vmeans"]), None, ptr(g["vopacities"]), ptr(g["vscales"]), ptr(g["vrotations"]))
        ok(lib.gsr_sh_grad_from_views_tail(n, K, deg, V, ptr(cc), ptr(vcd), C.byref(tg), C.byref(st), _stream()), "views tail")
        return dict(outs, vshs=vshs)

    ref = _five_runs(pkg, case)
    assert not ref["vshs"][:, (deg + 1) ** 2:].view(I32).any()


# ---------------------------------------------------------------------------------------------------------------------
# density control
@pytest.mark.parametrize("kind", ["zeros", "ones", "random"])
@pytest.mark.parametrize("n", [1, 257, 1031])
def test_mask_findall_and_gather(pkg, n, kind):
    L, lib = pkg._lib, pkg._lib.load()
    r = np.random.default_rng(n)
    mask = {"zeros": np.zeros(n, np.uint8), "ones": np.ones(n, np.uint8), "random": (r.random(n) < 0.4).astype(np.uint8)}[kind]
    if kind == "random":
        mask[-1] = 1
    cnt = int(mask.sum())
    words = (3, 1, 45, 4)
    src = [f32(r, n, w) for w in words]
    nb = int(lib.gsr_mask_findall_scratch_bytes(n))

    def case(P, ok):
        m = P.place("mask", mask, guard=(0, 1))
        idx, count = P.place("indices", (n,), I32, guard=(0, n - 1)), P.place("count_out", (1,), I32)
        sc = scratch(P, "scratch", nb, I32)
        ok(lib.gsr_mask_findall(ptr(m), n, ptr(idx), ptr(count), ptr(sc), _stream()), "findall")
        out = dict(count=count, indices=idx[:cnt])
        # gather with an index vector of EXACTLY count entries
        exact = P.place("indices_exact", np.flatnonzero(mask).astype(np.int32), guard=(0, n - 1))
        if cnt:
            s_ = [P.place(f"src{k}", a) for k, a in enumerate(src)]
            d_ = [P.place(f"dst{k}", (cnt, w)) for k, w in enumerate(words)]
            gg = (L.GatherGroup * len(words))(*[L.GatherGroup(ptr(a), ptr(b), w) for a, b, w in zip(s_, d_, words)])
            ok(lib.gsr_gather_rows(gg, len(words), ptr(exact), cnt, _stream()), "gather")
            out["gather"] = d_
        return out

    ref = _five_runs(pkg, case)
    assert int(ref["count"]) == cnt
    assert np.array_equal(ref["indices"].cpu().numpy(), np.flatnonzero(mask))
    if cnt:
        for k, a in enumerate(src):
            assert np.array_equal(ref[f"gather[{k}]"].cpu().numpy(), a[np.flatnonzero(mask)])


@pytest.mark.parametrize("form", ["clone", "split", "prune"])
@pytest.mark.parametrize("n", [65, 1031])
def test_compose_rows(pkg, n, form):
    """A moment group with new_zero, a row wider than one word and a row of 45 words."""
    L, lib = pkg._lib, pkg._lib.load()
    r = np.random.default_rng(n)
    words, zero = (3, 3, 1, 45, 4, 1), (0, 1, 0, 0, 1, 0)
    src = [f32(r, n, w) for w in words]
    sel_mask = r.random(n) < 0.3
    sel_mask[-1] = True
    if form == "clone":
        keep, sel, reps = None, np.flatnonzero(sel_mask), 1
    elif form == "split":
        keep, sel, reps = np.flatnonzero(~sel_mask), np.flatnonzero(sel_mask), 2
    else:
        keep, sel, reps = np.flatnonzero(sel_mask), None, 0
    n_keep = n if keep is None else len(keep)
    n_sel = 0 if sel is None else len(sel)
    rows = n_keep + reps * n_sel

    def case(P, ok):
        kd = None if keep is None else P.place("keep_idx", keep.astype(np.int32), guard=(0, n - 1))
        sd_ = None if sel is None else P.place("sel_idx", sel.astype(np.int32), guard=(0, n - 1))
        s_ = [P.place(f"src{k}", a) for k, a in enumerate(src)]
        d_ = [P.place(f"dst{k}", (rows, w)) for k, w in enumerate(words)]
        cg = (L.ComposeGroup * len(words))(*[L.ComposeGroup(ptr(a), ptr(b), w, z) for a, b, w, z in zip(s_, d_, words, zero)])
        ok(lib.gsr_compose_rows(cg, len(words), ptr(kd), n_keep, ptr(sd_), n_sel, reps, _stream()))
        return dict(dst=d_)

    ref = _five_runs(pkg, case)
    for k, a in enumerate(src):
        got = ref[f"dst[{k}]"].cpu().numpy()
        assert np.array_equal(got[:n_keep], a if keep is None else a[keep])
        if n_sel and reps:
            want = np.zeros((reps * n_sel, words[k]), np.float32) if zero[k] else np.tile(a[sel], (reps, 1))
            assert np.array_equal(got[n_keep:], want)


@pytest.mark.parametrize("n,sd", [(1, 3), (63, 1), (257, 3), (1031, 1)])
def test_densify_grad_mean_and_masks(pkg, n, sd):
    L, lib = pkg._lib, pkg._lib.load()
    r = np.random.default_rng(n)
    accum, denom = f32(r, n, lo=0.0), r.integers(0, 3, n).astype(np.float32)
    n_grad = max(n - 5, 0) if n > 1 else 1
    grad, scales, opac = f32(r, n_grad, lo=0.0), f32(r, n, sd) - 1.0, f32(r, n, 1, lo=-3, hi=3)
    radii = r.integers(0, 40, n).astype(np.int32)

    def case(P, ok):
        a, d = P.place("accum", accum), P.place("denom", denom)
        go = P.place("grad_out", (n,))
        ok(lib.gsr_densify_grad_mean(n, ptr(a), ptr(d), ptr(go), _stream()), "grad_mean")
        g, s_, o = P.place("grad", grad), P.place("scales", scales), P.place("opacities", opac)
        mr = P.place("max_radii", radii, guard=(0, 39))
        out = dict(grad_out=go)
        for kind, name in ((L.DENSIFY_CLONE, "clone"), (L.DENSIFY_SPLIT, "split"), (L.DENSIFY_PRUNE, "prune")):
            m = P.place("mask_" + name, (n,), U8, guard=(0, 1))
            ok(lib.gsr_densify_mask(kind, n, n_grad, ptr(g), ptr(s_), sd, ptr(o), ptr(mr), 0.4, float(np.exp(-1.0)), 0.3, 20, ptr(m),
                                    _stream()), name)
            out[name] = m
        return out

    ref = _five_runs(pkg, case)
    assert not ref["split"][n_grad:].any()      # rows beyond n_grad count as 0 (padded_grad)
    assert not torch.isnan(ref["grad_out"]).any()


@pytest.mark.parametrize("n,sd", [(1, 3), (65, 1), (1031, 3)])
def test_split_reset_morton_nonfinite(pkg, n, sd):
    lib = pkg._lib.load()
    r = np.random.default_rng(n)
    pts, rot, sc, op = f32(r, n, 3), f32(r, n, 4), f32(r, n, sd) - 2.0, f32(r, n, 1, lo=-4, hi=4)
    words = (3, 48, 1)
    grads = [f32(r, n, w) for w in words]
    grads[1][n // 2, 5] = np.nan
    grads[2][n - 1, 0] = np.inf

    def case(P, ok):
        p, q, s_ = P.place("points", pts, role="inout"), P.place("rotations", rot, align=16), P.place("scales", sc, role="inout")
        ok(lib.gsr_split_transform(n, sd, ptr(p), ptr(q), ptr(s_), 77, _stream()), "split_transform")
        o = P.place("opacities", op, role="inout")
        ok(lib.gsr_reset_opacity(n, ptr(o), _stream()), "reset_opacity")
        src = P.place("morton_points", pts)
        codes = P.place("codes", (n,), I64)
        lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
        ok(lib.gsr_morton_codes(n, ptr(src), lo, hi, ptr(codes), _stream()), "morton")
        g = [P.place(f"grad{k}", a) for k, a in enumerate(grads)]
        counts, first = P.place("counts", (3,), I32), P.place("first_bad", (3,), I32)
        arr, rw = (C.c_void_p * 3)(*[ptr(x) for x in g]), (C.c_int32 * 3)(*words)
        ok(lib.gsr_count_nonfinite(arr, rw, 3, n, ptr(counts), ptr(first), _stream()), "nonfinite")
        torch.cuda.synchronize()
        return dict(points=p, scales=s_, opacities=o, codes=codes, counts=counts, first=first)

    ref = _five_runs(pkg, case)
    assert ref["counts"].tolist() == [0, 1, 1] and ref["first"].tolist() == [-1, n // 2, n - 1]


@pytest.mark.parametrize("n,k_rest", [(1, 0), (63, 3), (257, 15), (1031, 3)])
def test_ply_rows(pkg, n, k_rest):
    lib = pkg._lib.load()
    r = np.random.default_rng(n + k_rest)
    arrays = model_arrays(r, n, k_rest, 3)
    names = ("points", "features_dc", "features_rest", "opacities", "scales", "rotations")

    def case(P, ok):
        src = [P.place(nm, a) if a.size else None for nm, a in zip(names, arrays)]
        rows = P.place("rows", (n, 17 + 3 * k_rest))
        ok(lib.gsr_ply_pack_rows(n, k_rest, *[ptr(t) for t in src], ptr(rows), _stream()), "pack")
        back = [P.place("back_" + nm, a.shape) if a.size else None for nm, a in zip(names, arrays)]
        ok(lib.gsr_ply_unpack_rows(n, k_rest, ptr(rows), *[ptr(t) for t in back], _stream()), "unpack")
        return dict(rows=rows, back=[b for b in back if b is not None])

    ref = _five_runs(pkg, case)
    live = [a for a in arrays if a.size]
    for k, a in enumerate(live):
        assert np.array_equal(ref[f"back[{k}]"].cpu().numpy(), a)


# ---------------------------------------------------------------------------------------------------------------------
# bilateral grid
@pytest.mark.parametrize("grid,nimg,wh,Cn", [((5, 4, 3), 1, (17, 9), 3), ((16, 16, 8), 3, (130, 70), 5), ((5, 4, 3), 3, (55, 33), 8),
                                            ((16, 16, 8), 1, (1, 1), 3)])
def test_bilateral(pkg, grid, nimg, wh, Cn):
    lib = pkg._lib.load()
    (gx, gy, gz), (W, H) = grid, wh
    r = np.random.default_rng(gx + W)
    image, vout = f32(r, H, W, Cn, lo=0.0), f32(r, H, W, Cn)
    grids0 = np.zeros((nimg, 12, gz, gy, gx), np.float32)
    for d in range(3):
        grids0[:, d * 4 + d] = 1.0
    grids0 += r.normal(scale=0.05, size=grids0.shape).astype(np.float32)
    nb_slice, nb_tv = int(lib.gsr_bilateral_scratch_bytes(W, H, gx, gy, gz)), int(lib.gsr_bilateral_tv_scratch_bytes(nimg))
    view = nimg - 1
    mu0, nu0 = f32(r, *grids0.shape, lo=-0.01, hi=0.01), f32(r, *grids0.shape, lo=0.0, hi=1e-4)

    def case(P, ok):
        im, vo = P.place("image", image), P.place("vout", vout)
        gr = P.place("grids", grids0)
        one = gr[view]
        out = P.place("out", (H, W, Cn))
        ok(lib.gsr_bilateral_slice_forward(W, H, Cn, ptr(im), ptr(one), gx, gy, gz, ptr(out), _stream()), "slice")
        vim, vgrid = P.place("vimage", (H, W, Cn)), P.place("vgrid", (12, gz, gy, gx))
        s1 = scratch(P, "slice_scratch", nb_slice)
        ok(lib.gsr_bilateral_slice_backward(W, H, Cn, ptr(im), ptr(one), gx, gy, gz, ptr(vo), ptr(vim), ptr(vgrid), ptr(s1), nb_slice,
                                            _stream()), "slice backward")
        loss, tvg = P.place("tv_loss", (1,)), P.place("tv_grad", grids0.shape)
        s2 = scratch(P, "tv_scratch", nb_tv)
        ok(lib.gsr_bilateral_tv(nimg, gx, gy, gz, ptr(gr), 10.0, ptr(loss), ptr(tvg), ptr(s2), nb_tv, _stream()), "tv")
        th, mu, nu = P.place("theta", grids0, role="inout"), P.place("mu", mu0, role="inout"), P.place("nu", nu0, role="inout")
        term = P.place("tv_loss_out", (1,))
        s3 = scratch(P, "tail_scratch", nb_tv)
        ok(lib.gsr_bilateral_adam_tail(nimg, gx, gy, gz, ptr(th), ptr(mu), ptr(nu), ptr(vgrid), view, 10.0, 2e-3, 5, 0.9, 0.999, 1e-15,
                                       ptr(term), ptr(s3), nb_tv, _stream()), "adam tail")
        return dict(out=out, vimage=vim, vgrid=vgrid, tv_loss=loss, tv_grad=tvg, theta=th, mu=mu, nu=nu, term=term)

    ref = _five_runs(pkg, case, nbytes=6 << 20)
    assert torch.isfinite(ref["theta"]).all() and torch.isfinite(ref["vgrid"]).all() and torch.isfinite(ref["term"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# geometry and depth losses
def _focal(W):
    return 0.9 * W + 3.0


def _rgbdn_frame(W, H, Cn=8):
    """The noisy slanted plane of the geometry tests (geometry_torch.noisy_frame): valid and invalid centres, alpha holes."""
    return np.ascontiguousarray(gt.noisy_frame(W, H, _focal(W), seed=W + H)[..., :Cn])


def _cam_struct(pkg, W, H):
    cs = pkg._lib.CameraS()
    cs.focal[0], cs.focal[1] = _focal(W), _focal(W)
    cs.principal[0], cs.principal[1] = 0.5, 0.5
    for k in (0, 4, 8):
        cs.R[k] = 1.0
    return cs


@pytest.mark.parametrize("W,H", [(1, 1), (17, 9), (55, 33), (130, 70)])
def test_normal_loss(pkg, W, H):
    lib = pkg._lib.load()
    r = np.random.default_rng(W)
    frame = _rgbdn_frame(W, H)
    vp0 = np.zeros((H, W, 8), np.float32)
    vp0[..., :3] = f32(r, H, W, 3)
    cs = _cam_struct(pkg, W, H)
    nb = int(lib.gsr_normal_loss_scratch_bytes(W, H))

    def case(P, ok):
        im = P.place("image", frame)
        loss, stats, wmap = P.place("loss_out", (1,)), P.place("stats_out", (2,)), P.place("weights_out", (H, W))
        sc = scratch(P, "scratch", nb)
        ok(lib.gsr_normal_loss_forward(W, H, 8, ptr(im), C.byref(cs), 0.05, ptr(loss), ptr(stats), ptr(wmap), ptr(sc), nb, _stream()), "fwd")
        vp = P.place("vpixels", vp0, role="inout")
        ok(lib.gsr_normal_loss_backward(W, H, 8, ptr(im), C.byref(cs), 0.05, ptr(vp), ptr(sc), nb, _stream()), "bwd")
        return dict(loss=loss, stats=stats, weights=wmap, vpixels=vp)

    ref = _five_runs(pkg, case)
    assert torch.equal(ref["vpixels"][..., :3].cpu(), torch.from_numpy(vp0[..., :3]))
    if (W, H) == (130, 70):
        assert float(ref["loss"]) > 0 and ref["vpixels"][..., 3:].abs().sum() > 0


@pytest.mark.parametrize("n,sd", [(1, 3), (63, 1), (257, 3), (1031, 3)])
def test_flatten_loss(pkg, n, sd):
    lib = pkg._lib.load()
    r = np.random.default_rng(n)
    sc_raw, vs0 = f32(r, n, sd) - 2.0, f32(r, n, 3)
    nb = int(lib.gsr_flatten_loss_scratch_bytes(n))

    def case(P, ok):
        s_, vs, loss = P.place("scales_raw", sc_raw), P.place("vscales", vs0, role="inout"), P.place("loss_out", (1,))
        sc = scratch(P, "scratch", nb)
        ok(lib.gsr_flatten_loss(n, sd, ptr(s_), 0.3, ptr(loss), ptr(vs), ptr(sc), nb, _stream()))
        return dict(loss=loss, vscales=vs)

    ref = _five_runs(pkg, case)
    assert float(ref["loss"]) > 0 and not torch.equal(ref["vscales"].cpu(), torch.from_numpy(vs0))


@pytest.mark.parametrize("disparity", [0.0, 1.0])
@pytest.mark.parametrize("W,H,Cn", [(1, 1, 5), (17, 9, 8), (55, 33, 5), (130, 70, 8)])
def test_depth_loss(pkg, W, H, Cn, disparity):
    L, lib = pkg._lib, pkg._lib.load()
    r = np.random.default_rng(W + Cn)
    frame = _rgbdn_frame(W, H, Cn)
    prior = (1.0 / frame[..., 3] + 0.02 * r.standard_normal((H, W))).astype(np.float32) if disparity else \
        (frame[..., 3] * 0.5 + 0.02 * r.standard_normal((H, W))).astype(np.float32)
    prior[r.random((H, W)) < 0.05] = np.nan
    anchor = L.DepthAnchorS(1.0 if disparity else 2.0, 0.01, 0.01, disparity, 0.3)
    vp0 = np.zeros((H, W, Cn), np.float32)
    vp0[..., :3] = f32(r, H, W, 3)
    nb = int(lib.gsr_depth_loss_scratch_bytes(W, H))

    def case(P, ok):
        pr = P.place("prior", prior)
        t0, h0, f0 = P.place("target_only", (H, W)), P.place("half_band_only", (H, W)), P.place("flags_only", (H, W), U8, guard=(0, 3))
        ok(lib.gsr_depth_target(W, H, ptr(pr), C.byref(anchor), 1.0 / 255.0, ptr(t0), ptr(h0), ptr(f0), _stream()), "target")
        im = P.place("image", frame)
        loss, stats = P.place("loss_out", (1,)), P.place("stats_out", (4,))
        t1, h1, f1 = P.place("target_out", (H, W)), P.place("half_band_out", (H, W)), P.place("flags_out", (H, W), U8, guard=(0, 3))
        sc = scratch(P, "scratch", nb, align=16)
        ok(lib.gsr_depth_loss_forward(W, H, Cn, ptr(im), ptr(pr), C.byref(anchor), 1.0 / 255.0, 0.5, 0.1, ptr(loss), ptr(stats), ptr(t1),
                                      ptr(h1), ptr(f1), ptr(sc), nb, _stream()), "fwd")
        vp = P.place("vpixels", vp0, role="inout")
        ok(lib.gsr_depth_loss_backward(W, H, Cn, ptr(im), ptr(pr), C.byref(anchor), 1.0 / 255.0, 0.5, 0.1, ptr(vp), ptr(sc), nb,
                                       _stream()), "bwd")
        return dict(t0=t0, h0=h0, f0=f0, loss=loss, stats=stats, t1=t1, h1=h1, f1=f1, vpixels=vp)

    ref = _five_runs(pkg, case)
    for a, b in (("t0", "t1"), ("h0", "h1"), ("f0", "f1")):
        assert torch.equal(bits(ref[a]), bits(ref[b]))
    assert torch.equal(ref["vpixels"][..., :3].cpu(), torch.from_numpy(vp0[..., :3]))
    if W == 130:
        assert float(ref["loss"]) > 0 and ref["vpixels"][..., 3:5].abs().sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# the MCMC strategy
def _mcmc_model(r, n, sd):
    op = f32(r, n, 1, lo=-8, hi=3)
    sc = f32(r, n, sd) - 3.0
    return op, sc


@pytest.mark.parametrize("n,sd,m", [(1, 3, 1), (65, 1, 1), (257, 3, 300), (1031, 1, 300), (1031, 3, 1)])
def test_mcmc_relocation_round(pkg, n, sd, m):
    """weights (with and without `dead`) -> sample (scratch exact) -> split_sampled -> relocate_rows, as relocate_gaussians
    chains them; the dead rows the relocation writes are the first min(m, dead) dead ones."""
    L, lib = pkg._lib, pkg._lib.load()
    r = np.random.default_rng(n + m)
    op, sc = _mcmc_model(r, n, sd)
    n_max = 51
    binoms = pkg.mcmc.binom_coefficients(n_max)
    nb = int(lib.gsr_mcmc_sample_scratch_bytes(n))
    words = (3, 3, 1, 45)
    rows = [f32(r, n, w) for w in words]
    zero = (0, 1, 0, 1)

    def case(P, ok):
        o, s_ = P.place("opacities_raw", op, role="inout"), P.place("scales_raw", sc, role="inout")
        q_all = P.place("q_all", (n,), I32, guard=(0, 1 << 29))
        ok(lib.gsr_mcmc_weights(n, sd, ptr(o), ptr(s_), 0.0, 0.0, ptr(q_all), None, _stream()), "weights")
        q, dead = P.place("q", (n,), I32, guard=(0, 1 << 29)), P.place("dead", (n,), U8, guard=(0, 1))
        ok(lib.gsr_mcmc_weights(n, sd, ptr(o), ptr(s_), 0.005, 0.5, ptr(q), ptr(dead), _stream()), "weights + dead")
        sampled, counts = P.place("sampled", (m,), I32, guard=(0, n - 1)), P.place("counts", (n,), I32, guard=(0, 1))
        total = P.place("total", (1,), I64, align=8)
        sc8 = scratch(P, "scratch", nb, I64, align=8)
        ok(lib.gsr_mcmc_sample(n, ptr(q), m, 1234, ptr(sampled), ptr(counts), ptr(total), ptr(sc8), nb, _stream()), "sample")
        b = P.place("binoms", binoms)
        ok(lib.gsr_mcmc_split_sampled(n, sd, ptr(counts), ptr(b), n_max, 0.005, ptr(o), ptr(s_), _stream()), "split_sampled")
        out = dict(q_all=q_all.clone(), q=q, dead=dead, sampled=sampled, counts=counts, total=total, opacities=o, scales=s_)
        dead_host = np.flatnonzero(dead.cpu().numpy())[:m].astype(np.int32)    # (a read-back, as relocate_gaussians has)
        md = len(dead_host) if int(total.item()) > 0 else 0
        if md:
            di = P.place("dead_idx", dead_host, guard=(0, n - 1))
            si = P.place("sampled_idx", sampled[:md].clone(), guard=(0, n - 1))
            x = [P.place(f"rows{k}", a, role="inout") for k, a in enumerate(rows)]
            cg = (L.ComposeGroup * len(words))(*[L.ComposeGroup(None, ptr(t), w, z) for t, w, z in zip(x, words, zero)])
            ok(lib.gsr_mcmc_relocate_rows(cg, len(words), n, ptr(di), ptr(si), md, _stream()), "relocate")
            out["rows"] = x
        return out

    ref = _five_runs(pkg, case)
    assert int(ref["counts"].sum()) == (m if int(ref["total"]) > 0 else 0)


@pytest.mark.parametrize("n,m", [(65, 1), (1031, 300)])
def test_mcmc_sample_without_weight_writes_nothing(pkg, n, m):
    """total = 0: `sampled` is not written (it keeps the caller's words), counts are zeros, *total = 0."""
    lib = pkg._lib.load()
    nb = int(lib.gsr_mcmc_sample_scratch_bytes(n))
    marks = np.arange(m, dtype=np.int32) % n

    def case(P, ok):
        q = P.place("q", np.zeros(n, np.int32), guard=(0, 1 << 29))
        sampled = P.place("sampled", marks, role="inout", guard=(0, n - 1))
        counts = P.place("counts", np.full(n, 3, np.int32), role="inout", guard=(0, 1))
        total = P.place("total", np.full(1, 9, np.int64), role="inout", align=8)
        sc8 = scratch(P, "scratch", nb, I64, align=8)
        ok(lib.gsr_mcmc_sample(n, ptr(q), m, 99, ptr(sampled), ptr(counts), ptr(total), ptr(sc8), nb, _stream()))
        return dict(sampled=sampled, counts=counts, total=total)

    ref = _five_runs(pkg, case)
    assert np.array_equal(ref["sampled"].cpu().numpy(), marks) and not ref["counts"].any() and int(ref["total"]) == 0


@pytest.mark.parametrize("m", [1, 63, 257, 1031])
def test_mcmc_relocation_params(pkg, m):
    lib = pkg._lib.load()
    r = np.random.default_rng(m)
    n_max = 51
    o = f32(r, m, lo=0.001, hi=0.999)
    ratio = r.integers(-3, n_max + 8, m).astype(np.int32)      # values outside [1, n_max] are clamped
    binoms = pkg.mcmc.binom_coefficients(n_max)

    def case(P, ok):
        od, rd, b = P.place("o", o), P.place("ratio", ratio, guard=(1, n_max)), P.place("binoms", binoms)
        new_o, coeff = P.place("new_o", (m,)), P.place("coeff", (m,))
        ok(lib.gsr_mcmc_relocation_params(m, ptr(od), ptr(rd), ptr(b), n_max, 0.005, ptr(new_o), ptr(coeff), _stream()))
        return dict(new_o=new_o, coeff=coeff)

    ref = _five_runs(pkg, case)
    assert torch.isfinite(ref["new_o"]).all() and torch.isfinite(ref["coeff"]).all()


@pytest.mark.parametrize("sd", [1, 3])
@pytest.mark.parametrize("n", ROWS)
def test_mcmc_inject_noise(pkg, n, sd):
    """mcmc_noise_kernel streams points and scales as the flat rows of a wave and keeps lanes >= n alive."""
    lib = pkg._lib.load()
    r = np.random.default_rng(n + sd)
    op, sc = _mcmc_model(r, n, sd)
    pts, rot = f32(r, n, 3), f32(r, n, 4)

    def case(P, ok):
        p, o, s_ = P.place("points", pts, role="inout"), P.place("opacities_raw", op), P.place("scales_raw", sc)
        q = P.place("rotations", rot, align=16)
        ok(lib.gsr_mcmc_inject_noise(n, sd, ptr(p), ptr(o), ptr(s_), ptr(q), 5e5 * 1.6e-4, 0.05, 4321, _stream()))
        return dict(points=p)

    ref = _five_runs(pkg, case)
    assert torch.isfinite(ref["points"]).all()
    if n >= 63:     # (a single row may be opaque enough for the gate to leave it where it is)
        assert not torch.equal(ref["points"].cpu(), torch.from_numpy(pts))


@pytest.mark.parametrize("with_grads", [False, True])
@pytest.mark.parametrize("n,sd", [(1, 3), (63, 1), (257, 3), (1031, 1)])
def test_mcmc_regularization(pkg, n, sd, with_grads):
    lib = pkg._lib.load()
    r = np.random.default_rng(n)
    op, sc = _mcmc_model(r, n, sd)
    vo0, vs0 = f32(r, n, 1), f32(r, n, 3)
    nb = int(lib.gsr_mcmc_regularization_scratch_bytes(n))

    def case(P, ok):
        o, s_, loss = P.place("opacities_raw", op), P.place("scales_raw", sc), P.place("loss_out", (1,))
        vo = P.place("vopacities", vo0, role="inout") if with_grads else None
        vs = P.place("vscales", vs0, role="inout") if with_grads else None
        scr = scratch(P, "scratch", nb)
        ok(lib.gsr_mcmc_regularization(n, sd, ptr(o), ptr(s_), 0.01, 0.01, ptr(loss), ptr(vo), ptr(vs), ptr(scr), nb, _stream()))
        out = dict(loss=loss)
        if with_grads:
            out.update(vo=vo, vs=vs)
        return out

    ref = _five_runs(pkg, case)
    assert float(ref["loss"]) > 0


@pytest.mark.parametrize("count", [4, 1028])
def test_stream_triad(pkg, count):
    lib = pkg._lib.load()
    r = np.random.default_rng(count)
    b, c = f32(r, count), f32(r, count)

    def case(P, ok):
        a, bd, cd = P.place("a", (count,), align=16), P.place("b", b, align=16), P.place("c", c, align=16)
        ok(lib.gsr_stream_triad(ptr(a), ptr(bd), ptr(cd), count, 3.0, _stream()))
        return dict(a=a)

    ref = _five_runs(pkg, case)
    assert np.allclose(ref["a"].cpu().numpy(), b + np.float32(3.0) * c, rtol=1e-6, atol=1e-6)   # (a sanity check; the five runs are bit-identical)
