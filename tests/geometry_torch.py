"""An independent torch formulation of the depth-normal consistency loss (autograd gives its gradients), in a chosen
dtype, and the input family of the geometry regularisation tests.  In float64 it checks the numpy restatement
(geometry_ref.py); in float32, on the CPU, it is the YARDSTICK of the GPU tests: what another valid evaluation of the same
fp32 formulation is off from float64 by."""
import numpy as np
import torch

import geometry_ref as gr


def depth_normal(image, focal, principal=(0.5, 0.5), dtype=torch.float64):
    """image (H, W, 8) numpy -> (loss tensor, leaf tensor with .grad after loss.backward(), valid mask (H-2, W-2) numpy,
    Σw, count).  The whole formulation in `dtype`, mask decisions included; the rays are the float32 values of pixel_rays."""
    H, W = image.shape[:2]
    x = torch.tensor(np.asarray(image), dtype=dtype, requires_grad=True)
    rx, ry = (torch.tensor(r, dtype=dtype) for r in gr.pixel_rays(W, H, focal, principal))
    D, A, N = x[..., 3], x[..., 4], x[..., 5:8]
    tiny = torch.tensor(1e-6, dtype=dtype)
    e = torch.clamp(D, min=0.0) / torch.maximum(A, tiny)
    c = (slice(1, -1), slice(1, -1))
    xp, xm = (slice(1, -1), slice(2, None)), (slice(1, -1), slice(0, -2))
    yp, ym = (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1))
    Rc, Rp, Rm = rx[None, 1:-1], rx[None, 2:], rx[None, :-2]
    Sc, Sp, Sm = ry[1:-1, None], ry[2:, None], ry[:-2, None]
    # central differences of the back-projected points e · (rx, ry, 1)
    tx = torch.stack([e[xp] * Rp - e[xm] * Rm, (e[xp] - e[xm]) * Sc, e[xp] - e[xm]], dim=-1)
    ty = torch.stack([(e[yp] - e[ym]) * Rc, e[yp] * Sp - e[ym] * Sm, e[yp] - e[ym]], dim=-1)
    n = torch.linalg.cross(tx, ty, dim=-1)
    n_sq = (n * n).sum(-1)
    ray = torch.stack([Rc.expand(H - 2, W - 2), Sc.expand(H - 2, W - 2), torch.ones(H - 2, W - 2, dtype=dtype)], dim=-1)
    sign = torch.where((n * ray).sum(-1) > 0, -1.0, 1.0).to(dtype).detach()
    nd = n * (sign / torch.sqrt(torch.clamp(n_sq, min=1e-24)))[..., None]
    nr = N[c]
    nr_sq = (nr * nr).sum(-1)
    cos = (nd * nr).sum(-1) / torch.sqrt(torch.clamp(nr_sq, min=float(np.float32(0.1)) ** 2))
    with torch.no_grad():
        a = torch.clamp(A, 0.0, 1.0)
        opaque = (a[c] >= 0.5) & (a[xp] >= 0.5) & (a[xm] >= 0.5) & (a[yp] >= 0.5) & (a[ym] >= 0.5)
        jump = torch.tensor(float(np.float32(0.05)), dtype=dtype) * e[c]
        cont = (e[c] >= tiny) & ((e[xp] - e[c]).abs() <= jump) & ((e[xm] - e[c]).abs() <= jump) & \
               ((e[yp] - e[c]).abs() <= jump) & ((e[ym] - e[c]).abs() <= jump)
        ok = opaque & cont & torch.isfinite(e[c]) & (n_sq >= 1e-24) & (nr_sq >= float(np.float32(0.1)) ** 2)
        w = torch.where(ok, a[c], torch.zeros((), dtype=dtype))
        count, sum_w = float(ok.sum()), float(w.sum())
    if not (count >= 64 and sum_w >= 16):
        return (x * 0).sum(), x, ok.numpy(), sum_w, count
    loss = (w * (1.0 - cos)).sum() / max(sum_w, 1.0)
    return loss, x, ok.numpy(), sum_w, count


def gradient(image, focal, principal=(0.5, 0.5), dtype=torch.float64):
    """-> (loss float, ∇image (H, W, 8) float64 numpy, valid mask, Σw, count)"""
    loss, x, ok, sum_w, count = depth_normal(image, focal, principal, dtype)
    loss.backward()
    return float(loss.detach()), x.grad.double().numpy(), ok, sum_w, count


PLANE_N = np.array([0.2, -0.3, -1.0]) / np.linalg.norm([0.2, -0.3, -1.0])
PLANE_D = -5.0


def plane_frame(W, H, f, normals=None, alpha=1.0):
    """The reference's test surface (test/runtests.jl:636-660): the slanted plane n·X = d sampled along the pixel rays,
    e = d / (n·ray); D = e·α; the normal channels hold `normals` (default: the plane's)·α."""
    rx, ry = gr.pixel_rays(W, H, (f, f), dtype=np.float64)
    e = PLANE_D / (PLANE_N[0] * rx[None, :] + PLANE_N[1] * ry[:, None] + PLANE_N[2])
    img = np.zeros((H, W, 8), np.float32)
    a = np.broadcast_to(np.asarray(alpha, np.float64), (H, W))
    img[..., 4] = a
    img[..., 3] = e * a
    img[..., 5:8] = (PLANE_N if normals is None else np.asarray(normals, np.float64)) * a[..., None]
    img[..., :3] = 0.5
    return img


def noisy_frame(W, H, f, seed):
    """The family of the GPU tests: the slanted plane with multiplicative depth noise, α uniform in [0.35, 1] with half
    the pixels set to 1, normals α·(n + 0.3·noise) and 5 % of them scaled by 0.05.  The noise on the normals is uniform in
    [-1, 1]³, so |nr|² stays outside [0.0081, 0.0121] by construction: >= (0.35·(1 - 0.3·√3))² = 0.028 unscaled,
    <= (0.05·(1 + 0.3·√3))² = 0.0058 scaled."""
    r = np.random.default_rng(seed)
    rx, ry = gr.pixel_rays(W, H, (f, f), dtype=np.float64)
    e = PLANE_D / (PLANE_N[0] * rx[None, :] + PLANE_N[1] * ry[:, None] + PLANE_N[2])
    e = e * (1.0 + 1e-3 * r.standard_normal((H, W)))
    a = r.uniform(0.35, 1.0, (H, W))
    a[r.random((H, W)) < 0.5] = 1.0
    nr = a[..., None] * (PLANE_N + 0.3 * r.uniform(-1.0, 1.0, (H, W, 3)))
    nr[r.random((H, W)) < 0.05] *= 0.05
    img = np.zeros((H, W, 8), np.float32)
    img[..., :3] = r.uniform(0.0, 1.0, (H, W, 3))
    img[..., 3] = e * a
    img[..., 4] = a
    img[..., 5:8] = nr
    return img


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
