"""References of the antialiased rendering mode (GSR_FLAG_ANTIALIASED), built from what the suite already trusts.

The identity everything here rests on: an antialiased render of opacities o is the plain render of o · rho, rho the
per-Gaussian, per-view compensation of add_blur (render.jl:387-396), rho = sqrt(max(0, det S / det(S + eps I))) of the 2-D
covariance S before the dilation.  So
  * the float64 column is tests/f64_model.render_dense called with opac · rho_f64(...): autograd carries the compensation path to
    the means, scales, rotations and (with pose tensors) the pose;
  * the fp32 oracle column is COMPOSED from unchanged oracle pieces, by linearity of the pullback (oracle_gradients_aa): the
    oracle's backward on the effective opacities, plus oracle.project_bwd on the conic cotangent that ∇inverse maps to
    orc_grad_add_blur's matrix.
Pure numpy / torch on top of f64_model and the oracle; no GPU code."""
import collections
import ctypes as C

import numpy as np
import torch

import f64_model as fm
import gradient_rows as gr

Leaves = collections.namedtuple("Leaves", "means shs opac scales rots")


def _t(a, grad=False):
    if torch.is_tensor(a):
        return a
    return torch.tensor(np.asarray(a, np.float64), dtype=fm.DT, requires_grad=grad)


def preblur_cov_f64(arrays, cam, R_w2c=None, t_w2c=None):
    """(N, 2, 2) float64 torch: the 2-D covariance BEFORE `+ blur_eps`, from the leaves `arrays` = (means, shs, opacities, scales,
    rotations) (numpy or float64 torch), through the camera transform, quat_scale_to_cov and perspective_projection exactly as
    f64_model.render_dense applies them."""
    means, _, _, scales, rots = arrays
    means, scales, rots = _t(means), _t(scales), _t(rots)
    R = torch.as_tensor(cam.R, dtype=fm.DT) if R_w2c is None else R_w2c
    t = torch.as_tensor(cam.t, dtype=fm.DT) if t_w2c is None else t_w2c
    pc = means @ R.T + t
    Sc = R @ fm.quat_scale_to_cov(rots, scales) @ R.T
    S2, _ = fm.perspective_projection(pc, Sc, cam.focal, (cam.width, cam.height), cam.principal)
    return S2


def rho_of_cov(S2, eps):
    """add_blur's compensation of pre-blur covariances (..., 2, 2), float64 torch, differentiable."""
    d0 = S2[..., 0, 0] * S2[..., 1, 1] - S2[..., 0, 1] * S2[..., 1, 0]
    d1 = (S2[..., 0, 0] + eps) * (S2[..., 1, 1] + eps) - S2[..., 0, 1] * S2[..., 1, 0]
    return torch.sqrt(torch.clamp(d0 / d1, min=0.0))


def rho_f64(arrays, cam, R_w2c=None, t_w2c=None, rows=None):
    """rho (N,) in float64 torch from the leaves, differentiable.  `rows` (optional boolean (N,), e.g. radii > 0): rho is evaluated
    on those rows only and is the constant 1 elsewhere — a Gaussian behind the camera has no finite projection, and a NaN in a row
    no list holds would still poison autograd (0 · inf)."""
    means, shs, opac, scales, rots = arrays
    means, scales, rots = _t(means), _t(scales), _t(rots)
    if rows is None:
        return rho_of_cov(preblur_cov_f64((means, shs, opac, scales, rots), cam, R_w2c, t_w2c), float(cam.blur_eps))
    idx = torch.as_tensor(np.flatnonzero(np.asarray(rows, bool)))
    sub = (means[idx], None, None, scales[idx], rots[idx])
    r = rho_of_cov(preblur_cov_f64(sub, cam, R_w2c, t_w2c), float(cam.blur_eps))
    return torch.ones(means.shape[0], dtype=fm.DT).index_put((idx,), r)


def render_dense_aa(means, shs, opac, scales, rots, cam, deg, background, mode, values_sorted, ranges, radii, R_w2c=None,
                    t_w2c=None, taps=None):
    """f64_model.render_dense of the effective opacities opac · rho_f64(...): the float64 definition of the antialiased image on
    the discrete structure given (float64 torch leaves in, image (H, W, C) out)."""
    rho = rho_f64((means, shs, opac, scales, rots), cam, R_w2c, t_w2c, rows=np.asarray(radii) > 0)
    return fm.render_dense(means, shs, opac * rho, scales, rots, cam, deg, background, mode, values_sorted, ranges, radii,
                           R_w2c=R_w2c, t_w2c=t_w2c, taps=taps)


def f64_gradients_aa(arrays, cam, deg, mode, bg, st, vp, pose=False):
    """gradient_rows.f64_gradients for the antialiased image: {name: (N, -1) float64} over gradient_rows.ALL_NAMES on the discrete
    structure of the oracle state `st`; pose=True: also "vR" (9, column-major) and "vt" (3), as hip_helpers.pose_grad_f64."""
    means, shs, opac, scales, rots = arrays
    n = np.asarray(means).shape[0]
    leaves = [_t(means, True), _t(shs, True), _t(np.asarray(opac).reshape(-1), True), _t(scales, True), _t(rots, True)]
    Rl = tl = None
    if pose:
        Rl, tl = _t(cam.R, True), _t(cam.t, True)
    taps = {}
    img = render_dense_aa(*leaves, cam, deg, np.asarray(bg, np.float32), mode, st.values_sorted, st.ranges, st.radii, R_w2c=Rl,
                          t_w2c=tl, taps=taps)
    taps["m2"].retain_grad()
    (img * torch.tensor(np.asarray(vp), dtype=fm.DT)).sum().backward()
    out = {nm: leaf.grad.numpy().reshape(n, -1).copy() for nm, leaf in zip(gr.NAMES, leaves)}
    out["vmeans2d"] = taps["m2"].grad.numpy().reshape(n, -1).copy()
    if pose:
        out["vR"], out["vt"] = Rl.grad.numpy().T.reshape(-1).copy(), tl.grad.numpy().reshape(-1).copy()
    return out


def add_blur_fp32(S2):
    """The three add_blur lines (render.jl:388-394) in numpy fp32 on pre-blur covariances (N, 2, 2) already rounded to fp32, eps =
    0.3: what ANY fp32 evaluation of the compensation inherits from the cancellation in det_orig."""
    S2 = np.asarray(S2, np.float32)
    eps = np.float32(0.3)
    d0 = S2[:, 0, 0] * S2[:, 1, 1] - S2[:, 0, 1] * S2[:, 1, 0]
    d1 = (S2[:, 0, 0] + eps) * (S2[:, 1, 1] + eps) - S2[:, 0, 1] * S2[:, 1, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(np.maximum(np.float32(0.0), d0 / d1)).astype(np.float32)


def axis_ratio_2d(S2):
    """sqrt(lambda_max / lambda_min) of (N, 2, 2) float64 covariances (inf where the smaller eigenvalue is <= 0)."""
    w = np.linalg.eigvalsh(np.asarray(S2, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w[:, 0] > 0, np.sqrt(w[:, 1] / np.maximum(w[:, 0], 1e-300)), np.inf)


def rho_bound(rho64, S2_64):
    """(bound on |rho_fp32 - rho64| per Gaussian, the rows beyond the ratio): 1e-4 · rho64 (the project's gradient tolerance) where the
    float64 2-D axis ratio is at most 10 (gradient_rows.ILL_RATIO); beyond it det_orig = S00 S11 - S01² cancels in fp32, and the bound
    adds 4 x (ILL_FACTOR) the error a numpy fp32 evaluation of the three add_blur lines shows against float64, starting from the
    float64 pre-blur covariance `S2_64` rounded to fp32."""
    S32 = np.asarray(S2_64, np.float32)
    err_np = np.abs(add_blur_fp32(S32).astype(np.float64) - rho64)
    ill = axis_ratio_2d(S2_64) > gr.ILL_RATIO
    return gr.REL * rho64 + np.where(ill, gr.ILL_FACTOR * err_np, 0.0), ill


def orc_add_blur(orc, S, eps=0.3):
    """orc_add_blur on one fp32 (2, 2) covariance: (blurred covariance (2, 2), det_blur, compensation)."""
    S = np.asarray(S, np.float32)
    Sb, det, comp = np.zeros(4, np.float32), C.c_float(), C.c_float()
    orc.lib().orc_add_blur(np.ascontiguousarray(S.T).reshape(-1).ctypes.data_as(C.POINTER(C.c_float)), C.c_float(eps),
                           Sb.ctypes.data_as(C.POINTER(C.c_float)), C.byref(det), C.byref(comp))
    return Sb.reshape(2, 2).T.copy(), float(det.value), float(comp.value)


def orc_grad_add_blur(orc, comp, vcomp, conic, eps=0.3):
    """orc_grad_add_blur: the (2, 2) fp32 cotangent of the pre-blur covariance for the conic (a, b, c)."""
    a, b, c = (np.float32(x) for x in conic)
    cm = np.array([a, b, b, c], np.float32)
    out = np.zeros(4, np.float32)
    orc.lib().orc_grad_add_blur(C.c_float(comp), C.c_float(vcomp), cm.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(eps),
                                out.ctypes.data_as(C.POINTER(C.c_float)))
    return out.reshape(2, 2).T.copy()


AAOracle = collections.namedtuple("AAOracle", "st rows plain extra rho o_eff vR vt")


def oracle_gradients_aa(orc, arrays, cam, deg, mode, bg, vp, rho=None, pose_grad=False):
    """The fp32 oracle column of the antialiased gradients, composed from unchanged oracle pieces by linearity.
      1. o_eff = o · rho in fp32 (`rho`: fp32 (N,), e.g. the device's GSR_BUF_COMPENSATIONS; None: rho_f64 rounded to fp32 — the
         oracle has no entry point that returns a scene's pre-blur covariances);
      2. st = oracle.forward(o_eff), g = oracle.backward(st, vp, o_eff): everything downstream of the effective opacity;
      3. v rho = g.vopacities · o;
      4. G = orc_grad_add_blur(rho, v rho, conic, eps) per visible Gaussian: the cotangent of the 2-D covariance;
      5. the conic cotangent that ∇inverse (-C vC C) maps to G: vC = -S_b G S_b, S_b the conic's inverse, formed in float64, rounded;
      6. oracle.project_bwd(vmeans2d = 0, vconics = vC, no depth / normal cotangent): the extra ∇means / ∇scales / ∇rotations (/ pose);
      7. added to g; ∇opacities = g.vopacities · rho.
    Returns AAOracle: the oracle state, rows = {name: (N, k) float64} over gradient_rows.ALL_NAMES, `plain` = the same rows before
    steps 3-7 (the plain render's gradients at o_eff), `extra` = what step 6 added per name, rho (fp32), o_eff, vR / vt (or None)."""
    means, shs, opac, scales, rots = (np.asarray(a, np.float32) for a in arrays)
    opac = opac.reshape(-1)
    n = means.shape[0]
    if rho is None:
        with torch.no_grad():
            rho = rho_f64(arrays, cam, rows=orc.project(means, scales, rots, cam)[1] > 0).numpy()
    rho = np.asarray(rho, np.float32).reshape(-1)
    o_eff = (opac * rho).astype(np.float32)
    st = orc.forward(means, shs, o_eff, scales, rots, cam, deg, background=bg, mode=mode)
    g = orc.backward(st, vp, means, shs, o_eff, scales, rots, cam, deg, background=bg, pose_grad=pose_grad)
    plain = {nm: gr._rows(a, n) for nm, a in zip(gr.ALL_NAMES, (g.vmeans, g.vshs, g.vopacities, g.vscales, g.vrots, g.vmeans2d))}
    vis = st.radii > 0
    vrho = (g.vopacities.astype(np.float32) * opac).astype(np.float32)
    vC = np.zeros((n, 3), np.float32)
    for i in np.flatnonzero(vis):
        a, b, c = (float(x) for x in st.conics[i])
        G = orc_grad_add_blur(orc, float(rho[i]), float(vrho[i]), st.conics[i], cam.blur_eps).astype(np.float64)
        Sb = np.linalg.inv(np.array([[a, b], [b, c]], np.float64))
        v = -Sb @ G @ Sb
        vC[i] = (v[0, 0], 0.5 * (v[0, 1] + v[1, 0]), v[1, 1])
    zeros2 = np.zeros((n, 2), np.float32)
    xm, xs, xr, xR, xt = orc.project_bwd(zeros2, vC, None, None, st.conics, st.radii, means, scales, rots, cam, pose_grad=pose_grad)
    extra = {nm: np.zeros_like(plain[nm]) for nm in gr.ALL_NAMES}
    extra["vmeans"], extra["vscales"], extra["vrots"] = gr._rows(xm, n), gr._rows(xs, n), gr._rows(xr, n)
    rows = {nm: plain[nm] + extra[nm] for nm in gr.ALL_NAMES}
    rows["vopacities"] = gr._rows((g.vopacities.astype(np.float32) * rho).astype(np.float32), n)
    vR = vt = None
    if pose_grad:
        vR = g.vR.astype(np.float64) + xR.astype(np.float64)
        vt = g.vt.astype(np.float64) + xt.astype(np.float64)
    return AAOracle(st, rows, plain, extra, rho, o_eff, vR, vt)


AAReference = collections.namedtuple("AAReference", "sc st orc f64 vis touched ill positions bmask aa")
_references = {}


def reference_aa(pkg, orc, name, rho=None, pose=False):
    """gradient_rows.reference for the antialiased mode: the scene `name` of gradient_rows.build_scene, the composed oracle column and
    the float64 column on the discrete structure of oracle.forward(o · rho), `touched` from the effective opacities.  Computed once
    per (scene, rho, pose), shared, read-only.  `aa` is the AAOracle (plain / extra rows, rho, o_eff, pose)."""
    key = (name, None if rho is None else np.asarray(rho, np.float32).tobytes(), pose)
    if key not in _references:
        from hip_helpers import blend_boundary_pixels
        sc = gr.build_scene(pkg, name)
        aa = oracle_gradients_aa(orc, sc.arrays, sc.cam, sc.deg, sc.mode, sc.bg, sc.vp, rho=rho, pose_grad=pose)
        f64 = f64_gradients_aa(sc.arrays, sc.cam, sc.deg, sc.mode, sc.bg, aa.st, sc.vp, pose=pose)
        n = np.asarray(sc.arrays[0]).shape[0]
        bmask, _, ids = blend_boundary_pixels(aa.st, aa.o_eff, sc.cam.width, sc.cam.height, with_ids=True)
        touched = np.zeros(n, bool)
        touched[list(ids)] = True
        s = np.abs(np.asarray(sc.arrays[3], np.float64))
        ill = s.max(1) / np.maximum(s.min(1), 1e-30) > gr.ILL_RATIO
        positions = None
        if sc.order is not None:
            positions = np.full(n, -1, np.int64)
            positions[sc.order] = np.arange(sc.order.size)
        for a in list(aa.rows.values()) + list(f64.values()) + [sc.vp]:
            a.setflags(write=False)
        _references[key] = AAReference(sc, aa.st, aa.rows, f64, aa.st.radii > 0, touched, ill, positions, bmask, aa)
    return _references[key]


def compensation_share(ref, name="vscales"):
    """Fraction of the visible rows of `name` on which the compensation's own pullback (step 6 of oracle_gradients_aa: the antialiased
    gradient minus the plain gradient at o · rho) exceeds 10 x the row tolerance: whether the scene can see ∇add_blur at all."""
    T, _ = gr.row_tolerance(np.asarray(ref.orc[name]), ref.vis)
    d = np.linalg.norm(ref.aa.extra[name], axis=1)
    return float((d[ref.vis] > 10.0 * T[ref.vis]).mean())
