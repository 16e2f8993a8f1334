"""CPU tests of tests/antialias_ref.py — the references the antialiased mode (GSR_FLAG_ANTIALIASED) is held to on
the GPU (tests/test_gpu_antialias.py).  They pin the helper, not the feature: rho_f64 against the oracle's add_blur, its autograd
against the oracle's ∇add_blur, and the composed oracle column against the float64 autograd of the antialiased image under the
row criterion of tests/gradient_rows.py — so that a row the GPU test exempts or fails is the device's doing.

Tolerances.  rho: 1e-4 relative (the project's gradient tolerance) where the float64 2-D axis ratio is at most 10
(gradient_rows.ILL_RATIO); beyond it det_orig = S00 S11 - S01² cancels, and the bound adds 4 x (ILL_FACTOR) the error a numpy fp32
evaluation of the three add_blur lines shows from the same rounded covariance.  ∇add_blur: 1e-5 relative on cases with rho >= 0.05 —
the reference's `+ 1e-6` under vsqrt_comp is a deliberate deviation of relative size 1e-6 / rho."""
import numpy as np
import pytest
import torch

import antialias_ref as ar
import f64_model as fm
import gradient_rows as gr

ROW_SCENES = ("cell-101", "cell-103", "cell-104", "needle-1")   # the scenes of the GPU gradient test


@pytest.mark.parametrize("name", ["cell-101", "cell-103", "needle-1"])
def test_rho_f64_against_orc_add_blur(pkg, orc, name):
    sc = gr.build_scene(pkg, name)
    vis = orc.project(*(np.asarray(sc.arrays[k], np.float32) for k in (0, 3, 4)), sc.cam)[1] > 0
    idx = np.flatnonzero(vis)
    with torch.no_grad():
        sub = tuple(None if k in (1, 2) else np.asarray(sc.arrays[k])[idx] for k in range(5))
        S2 = ar.preblur_cov_f64(sub, sc.cam).numpy()
        rho64 = ar.rho_f64(sc.arrays, sc.cam, rows=vis).numpy()[idx]
    assert np.isfinite(rho64).all() and (rho64 >= 0).all() and (rho64 <= 1).all()
    bound, ill = ar.rho_bound(rho64, S2)
    rho_orc = np.array([ar.orc_add_blur(orc, S.astype(np.float32), sc.cam.blur_eps)[2] for S in S2])
    err = np.abs(rho_orc - rho64)
    print(f"{name}: {idx.size} visible, {int(ill.sum())} with 2-D axis ratio > 10, worst |rho_orc - rho64| / rho64 = "
          f"{(err / np.maximum(rho64, 1e-300)).max():.2e}, worst err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (idx[err > bound][:8], err[err > bound][:8], bound[err > bound][:8])


def test_rho_autograd_against_orc_grad_add_blur(orc):
    import ctypes as C
    rng = np.random.default_rng(20261020)
    eps, worst, used = 0.3, 0.0, 0
    for _ in range(100):
        A = rng.standard_normal((2, 2)).astype(np.float32)
        S = (A @ A.T + np.float32(rng.uniform(0.02, 2.0)) * np.eye(2, dtype=np.float32)).astype(np.float32)
        S[0, 1] = S[1, 0]
        vcomp = float(np.float32(rng.standard_normal()))
        Sb, _, comp = ar.orc_add_blur(orc, S, eps)
        if comp < 0.05:
            continue
        used += 1
        conic = np.zeros(4, np.float32)
        orc.lib().orc_inverse2(np.ascontiguousarray(Sb.T).reshape(-1).ctypes.data_as(C.POINTER(C.c_float)),
                               conic.ctypes.data_as(C.POINTER(C.c_float)))
        G = ar.orc_grad_add_blur(orc, comp, vcomp, (conic[0], conic[1], conic[3]), eps).astype(np.float64)
        p = torch.tensor([float(S[0, 0]), float(S[0, 1]), float(S[1, 1])], dtype=fm.DT, requires_grad=True)
        S64 = torch.stack([torch.stack([p[0], p[1]]), torch.stack([p[1], p[2]])])
        (vcomp * ar.rho_of_cov(S64, eps)).backward()
        got, want = np.array([G[0, 0], G[0, 1] + G[1, 0], G[1, 1]]), p.grad.numpy()
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        worst = max(worst, rel)
        assert rel <= 1e-5, (S, comp, got, want, rel)
    assert used >= 50
    print(f"∇add_blur: {used} cases with rho >= 0.05, worst relative distance {worst:.2e}")


@pytest.mark.parametrize("name", ROW_SCENES)
def test_composed_oracle_rows_against_f64(pkg, orc, name):
    """oracle_gradients_aa alone passes the row criterion against render_dense_aa's autograd (the oracle column stands for both `hip`
    and `orc`): what the 2 % exemption cap of the GPU test rests on."""
    ref = ar.reference_aa(pkg, orc, name)
    assert gr.boundary_pixels_ok(ref.bmask)
    for nm in gr.ALL_NAMES:
        rep = gr.check_rows(f"{name} [antialiased, oracle alone] {nm}", ref.orc[nm], ref.orc[nm], ref.f64[nm], ref.vis, ref.touched,
                            ref.ill, ref.positions)
        print(f"rows {rep.name}: checked {rep.checked}, z {rep.z}, a {rep.a}, f {rep.f}, b {rep.b}, exempt {rep.exempt}")
        # (with the oracle in both roles rule (a) holds trivially; the statement is the one of test_gradient_rows_cpu.py: the oracle
        #  against float64 directly — every row outside the two exemption sets within T_i(f64), and the rows that miss it few)
        T, _ = gr.row_tolerance(np.asarray(ref.f64[nm]), ref.vis)
        miss = ref.vis & (np.linalg.norm(np.asarray(ref.orc[nm]) - np.asarray(ref.f64[nm]), axis=1) > T)
        assert not (miss & ~ref.touched & ~ref.ill).any(), (nm, np.flatnonzero(miss & ~ref.touched & ~ref.ill))
        assert miss.sum() <= gr.EXEMPT_CAP * rep.checked, (nm, int(miss.sum()))
        assert not np.asarray(ref.orc[nm])[~ref.vis].any() and not np.asarray(ref.f64[nm])[~ref.vis].any()


def test_cell_101_sees_the_compensation_pullback(pkg, orc):
    """On cell-101 the compensation's share of ∇scales is not negligible: |aa gradient - plain gradient at o · rho| exceeds 10 x the
    row tolerance on at least a tenth of the visible rows.  Otherwise the scene could not tell a missing ∇add_blur."""
    ref = ar.reference_aa(pkg, orc, "cell-101")
    share = ar.compensation_share(ref, "vscales")
    print(f"cell-101: compensation share of vscales beyond 10 T on {share:.1%} of {int(ref.vis.sum())} visible rows")
    assert share >= 0.1


def test_antialiased_opacity_gradient_is_with_respect_to_the_callers_opacity(pkg, orc):
    """∇opacities of the composed oracle = the plain gradient at o · rho times rho, and float64 agrees row by row."""
    ref = ar.reference_aa(pkg, orc, "cell-101")
    want = (np.asarray(ref.aa.plain["vopacities"], np.float32).reshape(-1) * ref.aa.rho).astype(np.float32)
    assert np.array_equal(np.asarray(ref.orc["vopacities"], np.float32).reshape(-1), want)
    gr.check_rows("cell-101 vopacities", ref.orc["vopacities"], ref.orc["vopacities"], ref.f64["vopacities"], ref.vis, ref.touched,
                  ref.ill)
