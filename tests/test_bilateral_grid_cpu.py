"""Bilateral grid (src/bilateral_grid.jl) without a GPU: the float64 restatement in bilateral_ref.py against an independent
torch float64 formulation and central differences, the reference's own test (test/runtests.jl:521-552) re-expressed,
the learning-rate schedule, the checkpoint keys, and the argument checks of the gsr_bilateral_* entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

import bilateral_ref as br

# ---- an independent torch float64 formulation: trilinear interpolation written as a gather over the 8 corners ----


def torch_slice(image, grid, zero_z_grad=None):
    """image (H, W, C) f64 tensor (finite), grid (12, gz, gy, gx) f64 tensor -> (H, W, 3).  `zero_z_grad` (H, W) bool:
    pixels whose guidance coordinate gets no gradient."""
    H, W = image.shape[:2]
    gz, gy, gx = grid.shape[1:]
    ax = lambda n, g: (torch.arange(n, dtype=torch.float64) / (n - 1) * (g - 1)) if n > 1 else torch.zeros(n, dtype=torch.float64)  # noqa: E731
    x = ax(W, gx)[None, :].expand(H, W)
    y = ax(H, gy)[:, None].expand(H, W)
    rgb = image[..., :3]
    guide = (0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]).clamp(0.0, 1.0)
    z = guide * (gz - 1)
    if zero_z_grad is not None:
        z = torch.where(zero_z_grad, z.detach(), z)
    x0, y0 = x.floor().long(), y.floor().long()
    z0 = z.detach().floor().long().clamp(0, gz - 1)
    idx = {0: (x0, y0, z0), 1: (torch.clamp(x0 + 1, max=gx - 1), torch.clamp(y0 + 1, max=gy - 1), torch.clamp(z0 + 1, max=gz - 1))}
    fx, fy, fz = x - x0, y - y0, z - z0
    coef = torch.zeros(H, W, 12, dtype=torch.float64)
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                w = (fx if cx else 1 - fx) * (fy if cy else 1 - fy) * (fz if cz else 1 - fz)
                coef = coef + w[..., None] * grid[:, idx[cz][2], idx[cy][1], idx[cx][0]].permute(1, 2, 0)
    A = coef.reshape(H, W, 3, 4)
    hom = torch.cat([rgb, torch.ones(H, W, 1, dtype=torch.float64)], dim=-1)
    return (A * hom[:, :, None, :]).sum(-1)


def torch_tv(grids):
    n, _, gz, gy, gx = grids.shape
    dx, dy, dz = grids.diff(dim=4), grids.diff(dim=3), grids.diff(dim=2)
    return ((dx ** 2).sum() / max(1, (gx - 1) * gy * gz) + (dy ** 2).sum() / max(1, gx * (gy - 1) * gz)
            + (dz ** 2).sum() / max(1, gx * gy * (gz - 1))) / (12 * n)


def _case(W, H, Cc, size, seed, specials=True):
    r = np.random.default_rng(seed)
    gx, gy, gz = size
    img = r.uniform(-0.5, 1.5, (H, W, Cc)).astype(np.float32)
    grid = (br.identity_grids(1, gx, gy, gz)[0] + r.normal(0, 0.3, (12, gz, gy, gx))).astype(np.float32)
    vout = r.normal(size=(H, W, Cc)).astype(np.float32)
    if specials and W * H > 4:
        img[0, -1, 1] = np.nan
        img[-1, 0, 2] = np.inf
        vout[-1, -1, 0] = np.nan
        vout[0, 0, 2] = -np.inf
    return img, grid, vout


SIZES = [(13, 9), (1, 7), (7, 1), (1, 1)]
GRIDS = [(4, 3, 5), (1, 1, 1), (3, 1, 2), (2, 5, 1)]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("size", GRIDS)
def test_reference_matches_torch_autograd(W, H, size):
    img, grid, vout = _case(W, H, 5, size, 1 + W + 7 * H)
    c = br.coords(img, *size)
    out = br.slice_forward(img, grid)
    vimg, vgrid = br.slice_backward(img, grid, vout)
    # the torch formulation works on the sanitized values; its guidance gradient is dropped where the reference's is
    s = np.where(np.isfinite(img), img, 0.5).astype(np.float64)
    ti = torch.tensor(s, requires_grad=True)
    tg = torch.tensor(grid.astype(np.float64), requires_grad=True)
    tout = torch_slice(ti, tg, zero_z_grad=torch.tensor(~c["z_interior"]))
    # (the reference's coordinates are fp32, the torch formulation's float64: they agree to fp32 rounding)
    assert np.abs(tout.detach().numpy() - out[..., :3]).max() <= 2e-6
    assert np.array_equal(out[..., 3:], img[..., 3:].astype(np.float64))
    d = np.where(np.isfinite(vout), vout, 0.0)[..., :3]
    (tout * torch.tensor(d)).sum().backward()
    finite = np.isfinite(img[..., :3])
    assert np.abs(ti.grad.numpy()[..., :3][finite] - vimg[..., :3][finite]).max() <= 1e-5 * max(1.0, np.abs(vimg).max())
    assert np.abs(tg.grad.numpy() - vgrid).max() <= 1e-5 * max(1.0, np.abs(vgrid).max())
    # channels >= 3 of the cotangent pass through unchanged (non-finite values included)
    np.testing.assert_array_equal(vimg[..., 3:], vout[..., 3:].astype(np.float64))


def test_saturated_and_on_cell_guidance_get_no_guidance_gradient():
    gx, gy, gz = 3, 2, 3
    # a grey whose fp32 guidance lands exactly on the middle level: z = 1
    v = np.float32(0.5)
    while br.coords(np.full((1, 1, 3), v, np.float32), gx, gy, gz)["fz"][0, 0] != 0.0:
        v = np.nextafter(v, np.float32(1.0), dtype=np.float32)
    img = np.array([[[v, v, v], [2.0, 2.0, 2.0], [-1.0, -1.0, -1.0], [0.3, 0.6, 0.2]]], np.float32)
    c = br.coords(img, gx, gy, gz)
    assert list(c["z_interior"][0]) == [False, False, False, True]
    r = np.random.default_rng(5)
    grid = r.normal(size=(12, gz, gy, gx)).astype(np.float32)
    vout = r.normal(size=img.shape).astype(np.float32)
    vimg, _ = br.slice_backward(img, grid, vout)
    # without the guidance path the image gradient is A^T Δ of the interpolated transform
    ti = torch.tensor(img.astype(np.float64), requires_grad=True)
    tout = torch_slice(ti, torch.tensor(grid.astype(np.float64)), zero_z_grad=torch.ones(1, 4, dtype=torch.bool))
    (tout * torch.tensor(vout.astype(np.float64))).sum().backward()
    np.testing.assert_allclose(vimg[0, :3], ti.grad.numpy()[0, :3], atol=1e-6)
    assert np.abs(vimg[0, 3] - ti.grad.numpy()[0, 3]).max() > 1e-6   # the interior pixel does have a guidance term


def test_reference_matches_central_differences():
    W, H, size = 6, 5, (3, 3, 4)
    img, grid, vout = _case(W, H, 3, size, 11, specials=False)
    img = np.clip(img, 0.05, 0.95).astype(np.float32)   # away from the clamp
    vimg, vgrid = br.slice_backward(img, grid, vout)
    f = lambda im, g: float((br.slice_forward(im, g)[..., :3] * vout.astype(np.float64)).sum())  # noqa: E731
    r = np.random.default_rng(3)
    u = r.normal(size=grid.shape)
    h = 1e-3
    num = (f(img, (grid + h * u)) - f(img, (grid - h * u))) / (2 * h)   # linear in the grid
    assert abs(num - (vgrid * u).sum()) <= 1e-9 * max(1.0, abs(num))
    for (hi, wi, ch) in [(0, 0, 0), (2, 3, 1), (4, 5, 2), (1, 2, 0)]:
        ip, im = img.astype(np.float64).copy(), img.astype(np.float64).copy()
        e = 1e-3
        ip[hi, wi, ch] += e
        im[hi, wi, ch] -= e
        num = (f(ip.astype(np.float32), grid) - f(im.astype(np.float32), grid)) / (float(np.float32(ip[hi, wi, ch])) - float(np.float32(im[hi, wi, ch])))
        assert abs(num - vimg[hi, wi, ch]) <= 2e-3 * max(1.0, abs(num)), (hi, wi, ch, num, vimg[hi, wi, ch])


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 4, 2, 3), (2, 1, 5, 1), (1, 8, 1, 6)])
def test_tv_matches_autograd_and_central_differences(shape):
    n, gz, gy, gx = shape
    r = np.random.default_rng(sum(shape))
    grids = r.normal(size=(n, 12, gz, gy, gx))
    t = torch.tensor(grids, requires_grad=True)
    loss = torch_tv(t)
    loss.backward()
    assert abs(loss.item() - br.tv_loss(grids)) <= 1e-12 * max(1.0, loss.item())
    np.testing.assert_allclose(br.tv_grad(grids), t.grad.numpy(), atol=1e-12)
    u = r.normal(size=grids.shape)
    h = 1e-4
    num = (br.tv_loss(grids + h * u) - br.tv_loss(grids - h * u)) / (2 * h)
    assert abs(num - (br.tv_grad(grids) * u).sum()) <= 1e-7 * max(1.0, abs(num))


def _brute_force_terms(img, grid, vout):
    """slice_forward_terms / slice_backward_terms as a loop over pixels, corners and coefficients, scalar by scalar, from
    the fp32 coordinates of coords()."""
    gz, gy, gx = grid.shape[1:]
    H, W = img.shape[:2]
    c = br.coords(img, gx, gy, gz)
    G = grid.astype(np.float64)
    acc, facc = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    r = dict(vimage=vout.astype(np.float64).copy(), vgrid=np.zeros(G.shape), vgrid_abs=np.zeros(G.shape),
             vgrid_count=np.zeros(G.shape, np.int64), gs_abs=np.zeros((H, W, 3)), gz_abs=np.zeros((H, W)))
    for h in range(H):
        for w in range(W):
            s4 = [c["s"][h, w, 0], c["s"][h, w, 1], c["s"][h, w, 2], 1.0]
            d = [float(v) if np.isfinite(v) else 0.0 for v in vout[h, w, :3]]
            fx, fy, fz = c["fx"][h, w], c["fy"][h, w], c["fz"][h, w]
            gs, gzs = [0.0, 0.0, 0.0], 0.0
            for xc in (0, 1):
                for yc in (0, 1):
                    for zc in (0, 1):
                        xi, yi, zi = c["x"][xc][h, w], c["y"][yc][h, w], c["z"][zc][h, w]
                        wxy = (fx if xc else 1 - fx) * (fy if yc else 1 - fy)
                        wt = wxy * (fz if zc else 1 - fz)
                        dwdz = wxy * (1.0 if zc else -1.0) * (gz - 1)
                        for di in range(3):
                            for si in range(4):
                                v = G[di * 4 + si, zi, yi, xi]
                                acc[h, w, di] += v * wt * s4[si]
                                facc[h, w, di] += abs(v * wt * s4[si])
                                if si < 3:
                                    gs[si] += v * wt * d[di]
                                    r["gs_abs"][h, w, si] += abs(v * wt * d[di])
                                if c["z_interior"][h, w]:
                                    gzs += dwdz * v * (s4[si] * d[di])
                                    r["gz_abs"][h, w] += abs(dwdz * v * (s4[si] * d[di]))
                                r["vgrid"][di * 4 + si, zi, yi, xi] += wt * (s4[si] * d[di])
                                r["vgrid_abs"][di * 4 + si, zi, yi, xi] += abs(wt * (s4[si] * d[di]))
                                r["vgrid_count"][di * 4 + si, zi, yi, xi] += wt != 0
            for k in range(3):
                r["vimage"][h, w, k] = gs[k] + float(br.C2G[k]) * gzs
    return acc, facc, r


def test_term_helpers_match_a_brute_force_loop_and_the_definitions():
    """One tiny case with a column on a cell boundary (W = 5, gx = 3: x = 0, 0.5, 1, 1.5, 2), saturated and non-finite
    pixels, a non-finite cotangent: the absolute-value sums and term counts of slice_forward_terms / slice_backward_terms
    against the scalar loop, and their plain sums against slice_forward / slice_backward themselves."""
    W, H, size = 5, 4, (3, 2, 3)
    img, grid, vout = _case(W, H, 5, size, 23)
    img[1, 2, :3] = 2.0                                    # saturated, on the boundary column
    img[2, 1, :3] = -1.0
    acc, facc, r = _brute_force_terms(img, grid, vout)
    a, A = br.slice_forward_terms(img, grid)
    np.testing.assert_allclose(a, acc, rtol=0, atol=1e-13)
    np.testing.assert_allclose(A, facc, rtol=1e-13, atol=0)
    assert np.array_equal(np.where(np.isfinite(a), a, 0.5), br.slice_forward(img, grid)[..., :3])
    t = br.slice_backward_terms(img, grid, vout)
    for k in ("vimage", "vgrid"):
        np.testing.assert_allclose(t[k], r[k], rtol=0, atol=1e-13, err_msg=k)
    for k in ("vgrid_abs", "gs_abs", "gz_abs"):
        np.testing.assert_allclose(t[k], r[k], rtol=1e-13, atol=0, err_msg=k)
    assert np.array_equal(t["vgrid_count"], r["vgrid_count"])
    vimg, vgrid = br.slice_backward(img, grid, vout)
    assert np.array_equal(t["vimage"], vimg, equal_nan=True) and np.array_equal(t["vgrid"], vgrid)
    # what the sums must satisfy whatever the case: |sum| <= Σ|terms|; an entry without a term is exactly zero; the
    # boundary column puts its full xy weight on one column, so those pixels count 4 (or 2, on a level) terms, not 8
    assert (np.abs(t["vgrid"]) <= t["vgrid_abs"] * (1 + 1e-12)).all()
    assert not t["vgrid"][t["vgrid_count"] == 0].any() and not t["vgrid_abs"][t["vgrid_count"] == 0].any()
    assert (np.abs(t["vimage"][..., :3]) <= (t["gs_abs"] + np.array(br.C2G, np.float64) * t["gz_abs"][..., None]) * (1 + 1e-12)).all()
    c = br.coords(img, *size)
    assert (c["fx"][:, 2] == 0).all() and c["x"][0][0, 2] == 1
    assert not t["gz_abs"][~c["z_interior"]].any() and t["gz_abs"][c["z_interior"]].all()
    # every coefficient of an entry has the same terms: 12 equal counts, and they add up to the pixels' live corners
    assert (t["vgrid_count"] == t["vgrid_count"][:1]).all()
    live = sum(int((wt != 0).sum()) for *_, wt, _ in br._corners(c, size[2]))
    assert t["vgrid_count"][0].sum() == live < 8 * W * H


def test_the_clamped_corner_carries_no_weight():
    """A pixel whose cell is the last one (x0 = g - 1, so x1 is clamped onto x0) has fx == 0 in fp32, whatever the sizes:
    the coordinate never exceeds g - 1.  So the clamped corner adds nothing to ∇grid, and the pullback's sum kernel, which
    maps the last cell's second corner slot onto the last entry, adds exact zeros there: dropping that clamp cannot change
    a bit, and no test can tell."""
    for g in range(1, 34):
        for n in list(range(1, 80)) + [257, 1000, 1920, 4097]:
            x = br._axis(n, g)
            assert x.dtype == np.float32 and (np.diff(x) >= 0).all() and x.max() <= g - 1
            last = np.floor(x) == g - 1
            assert (last[-1] or n == 1) and (x[last] == np.float32(g - 1)).all(), (n, g)   # (one pixel sits at 0)
    # and on the whole path: the entries' terms of shape (2, 2, .)'s last column all come from corners with xc = 0 or x1 = x0 + 1
    img, grid, vout = _case(9, 7, 3, (2, 3, 2), 3)
    c = br.coords(img, 2, 3, 2)
    assert (c["fx"][c["x"][0] == c["x"][1]] == 0).all() and (c["fy"][c["y"][0] == c["y"][1]] == 0).all()


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 4, 2, 3), (2, 1, 5, 1), (22, 1, 1, 257)])
def test_tv_grad_terms_match_a_loop_and_tv_grad(shape):
    n, gz, gy, gx = shape
    grids = np.random.default_rng(sum(shape)).normal(size=(n, 12, gz, gy, gx)).astype(np.float32)
    g, A = br.tv_grad_terms(grids)
    assert np.array_equal(g, br.tv_grad(grids))
    a = grids.astype(np.float64)
    norms = (max(1, (gx - 1) * gy * gz), max(1, gx * (gy - 1) * gz), max(1, gx * gy * (gz - 1)))
    want = np.zeros_like(a)
    for z in range(gz):
        for y in range(gy):
            for x in range(gx):
                for (dz, dy, dx), norm in (((0, 0, 1), norms[0]), ((0, 1, 0), norms[1]), ((1, 0, 0), norms[2])):
                    for sgn in (-1, 1):
                        zz, yy, xx = z + sgn * dz, y + sgn * dy, x + sgn * dx
                        if 0 <= zz < gz and 0 <= yy < gy and 0 <= xx < gx:
                            want[:, :, z, y, x] += np.abs(a[:, :, z, y, x] - a[:, :, zz, yy, xx]) * (2.0 / (norm * 12 * n))
    np.testing.assert_allclose(A, want, rtol=1e-13, atol=0)
    assert (np.abs(g) <= A * (1 + 1e-12)).all()
    assert not br.tv_grad_terms(br.identity_grids(n, gx, gy, gz))[1].any()


def test_reference_testset_reexpressed():
    """test/runtests.jl:521-552: identity grids leave the image unchanged and have no variation; through slice + TV only
    the sliced view receives a gradient, the other views' is exactly zero."""
    w, h, n, idx = 64, 48, 4, 1
    grids = br.identity_grids(n, 8, 8, 4)
    r = np.random.default_rng(0)
    image = r.uniform(size=(h, w, 3)).astype(np.float32)
    out = br.slice_forward(image, grids[idx])
    np.testing.assert_allclose(out, image, atol=1e-6)
    assert br.tv_loss(grids) == 0.0
    target = r.uniform(size=(h, w, 3))
    vout = (np.sign(out - target) / out.size).astype(np.float32)      # ∂ mean|corrected - target|
    vimg, vgrid = br.slice_backward(image, grids[idx], vout)
    full = 10.0 * br.tv_grad(grids)
    full[idx] += vgrid
    others = [i for i in range(n) if i != idx]
    assert not full[others].any()
    assert np.abs(full[idx]).max() > 0 and np.isfinite(full).all() and np.isfinite(vimg).all()


def test_scheduler_matches_a_float32_restatement(pkg):
    from gaussiansplatting_jl_amd import bilateral_grid as bg   # noqa: F401 (needs torch only)
    lr, steps = np.float32(2e-3), 30_000
    sched = bg.bilateral_grid_scheduler(2e-3, steps)

    def expect(step):
        if step < 0:
            return np.float32(0)
        t = np.clip(np.array(step / steps, np.float32), np.float32(0), np.float32(1))
        la, lb = np.log(np.array([lr, np.float32(0.01) * lr], np.float32))
        decay = np.exp(la * (np.float32(1) - t) + lb * t)
        warm = np.float32(0.01) + np.float32(0.99) * np.float32(step / 1000) if step < 1000 else np.float32(1)
        return np.float32(warm * decay)

    for step in (-1, 0, 1, 999, 1000, 1001, 30_000, 40_000):
        got = sched(step)
        assert isinstance(got, np.float32)
        assert got == expect(step), (step, got, expect(step))
    assert sched(30_000) == sched(40_000)
    assert abs(float(sched(0)) - 2e-5) < 1e-10 and abs(float(sched(30_000)) - 2e-5) < 1e-10   # 1 % at both ends
    assert abs(float(sched(1000)) - 2e-3 * 0.01 ** (1000 / 30_000)) < 1e-9


class _Opt:
    def __init__(self, n, seed):
        r = np.random.default_rng(seed)
        self.mu = torch.from_numpy(r.normal(size=n).astype(np.float32))
        self.nu = torch.from_numpy(r.uniform(size=n).astype(np.float32))
        self.current_step = 3 + seed


class _Grid:  # the fields of bilateral_grid.BilateralGrid a checkpoint carries
    def __init__(self, n, size, seed):
        gx, gy, gz = size
        self.grids = torch.from_numpy(np.random.default_rng(seed).normal(size=(n, 12, gz, gy, gx)).astype(np.float32))
        self.optimizer = _Opt(self.grids.numel(), seed)


def _state(pkg, path, bgrid):
    r = np.random.default_rng(1)
    f = lambda *s: r.normal(size=s).astype(np.float32)  # noqa: E731
    n = 5
    g = pkg.ply.GaussianModel(f(n, 3), f(n, 1, 3), f(n, 3, 3), f(n, 3), f(n, 4), f(n, 1), 1, 1)
    sizes = dict(points=15, features_dc=15, features_rest=45, opacities=5, scales=15, rotations=20)
    opts = {k: _Opt(v, i) for i, (k, v) in enumerate(sizes.items())}
    pkg.checkpoint.save_state(path, g, opts, step=77, bilateral_grid=bgrid)
    return {k: _Opt(v, 50) for k, v in sizes.items()}


def test_checkpoint_roundtrip_of_grids_and_adam(pkg, tmp_path):
    ck = pkg.checkpoint
    path = str(tmp_path / "bg.safetensors")
    src = _Grid(3, (4, 3, 2), 7)
    fresh_opts = _state(pkg, path, src)
    c = ck.load_checkpoint(path)
    assert c.raw_tensor("bilateral.grids").shape == (4, 3, 2, 12, 3)     # Julia (gx, gy, gz, 12, n)
    assert c.raw_tensor("bilateral.opt.mu.1").shape == (4, 3, 2, 12, 3)
    assert c.meta["bilateral.opt.current_step"] == str(src.optimizer.current_step)
    dst = _Grid(3, (4, 3, 2), 8)
    _, step = ck.load_state(path, fresh_opts, bilateral_grid=dst)
    assert step == 77
    assert torch.equal(dst.grids, src.grids)
    assert torch.equal(dst.optimizer.mu, src.optimizer.mu) and torch.equal(dst.optimizer.nu, src.optimizer.nu)
    assert dst.optimizer.current_step == src.optimizer.current_step
    with pytest.raises(ValueError, match="bilateral.grids"):
        ck.load_state(path, fresh_opts, bilateral_grid=_Grid(2, (4, 3, 2), 9))


def test_checkpoint_without_grids_still_loads(pkg, tmp_path):
    ck = pkg.checkpoint
    path = str(tmp_path / "plain.safetensors")
    fresh_opts = _state(pkg, path, None)
    assert "bilateral.grids" not in ck.load_checkpoint(path)
    keep = _Grid(2, (2, 2, 2), 4)
    before = keep.grids.clone()
    _, step = ck.load_state(path, fresh_opts, bilateral_grid=keep)    # haskey semantics: left as it is
    assert step == 77 and torch.equal(keep.grids, before) and keep.optimizer.current_step == 7


def test_scratch_bytes_and_invalid_arguments(pkg):
    """Every check fails with GSR_E_INVALID_ARG before any HIP call (no device here).  Non-null dummies stand in for
    device pointers: they are never dereferenced when the call is refused."""
    L = pkg._lib
    lib = L.load()
    E = L.GSR_E_INVALID_ARG
    nchunk = -(-((1919 // 15 + 2) * (1079 // 15 + 2)) // 1024)
    assert lib.gsr_bilateral_scratch_bytes(1920, 1080, 16, 16, 8) == 16 * 16 * nchunk * 8 * 48 * 4
    assert lib.gsr_bilateral_scratch_bytes(0, 1080, 16, 16, 8) == 0
    assert lib.gsr_bilateral_tv_scratch_bytes(200) == 200 * 12 * 3 * 4
    assert lib.gsr_bilateral_tv_scratch_bytes(0) == 0
    p = C.c_void_p(16)
    fwd = lambda W=8, H=8, Cc=3, im=p, g=p, gx=2, gy=2, gz=2, out=p: lib.gsr_bilateral_slice_forward(W, H, Cc, im, g, gx, gy, gz, out, None)  # noqa: E731
    for kw in (dict(W=0), dict(H=-1), dict(Cc=4), dict(Cc=1), dict(im=None), dict(g=None), dict(out=None), dict(gx=0),
               dict(gz=65), dict(gx=64, gy=64, gz=8)):
        assert fwd(**kw) == E, kw
    nb = lib.gsr_bilateral_scratch_bytes(8, 8, 2, 2, 2)

    def bwd(W=8, H=8, Cc=5, im=p, g=p, gx=2, gy=2, gz=2, vo=p, vi=p, vg=p, sc=p, nsc=nb):
        return lib.gsr_bilateral_slice_backward(W, H, Cc, im, g, gx, gy, gz, vo, vi, vg, sc, nsc, None)
    for kw in (dict(W=0), dict(Cc=6), dict(im=None), dict(vo=None), dict(vi=None), dict(vg=None), dict(sc=None),
               dict(nsc=nb - 1), dict(gy=0)):
        assert bwd(**kw) == E, kw
    ntv = lib.gsr_bilateral_tv_scratch_bytes(3)

    def tv(n=3, gx=2, gy=2, gz=2, grids=p, loss=p, sc=p, nsc=ntv):
        return lib.gsr_bilateral_tv(n, gx, gy, gz, grids, 10.0, loss, None, sc, nsc, None)
    for kw in (dict(n=0), dict(gz=0), dict(grids=None), dict(loss=None), dict(sc=None), dict(nsc=ntv - 4)):
        assert tv(**kw) == E, kw

    def tail(n=3, gz=2, grids=p, mu=p, nu=p, vg=p, view=1, step=1, loss=p, sc=p, nsc=ntv):
        return lib.gsr_bilateral_adam_tail(n, 2, 2, gz, grids, mu, nu, vg, view, 10.0, 1e-3, step, 0.9, 0.999, 1e-15, loss,
                                           sc, nsc, None)
    for kw in (dict(n=0), dict(gz=0), dict(view=3), dict(view=-1), dict(grids=None), dict(mu=None), dict(nu=None),
               dict(vg=None), dict(loss=None), dict(sc=None), dict(step=0), dict(nsc=ntv - 1)):
        assert tail(**kw) == E, kw
    assert b"view 3 of 3" in (tail(view=3), lib.gsr_last_error_string())[1]
