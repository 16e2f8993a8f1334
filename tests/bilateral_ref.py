"""Float64 numpy restatement of src/bilateral_grid.jl (bilateral_slice, its pullback, tv_loss and its gradient), written
from the reference's semantics.  Layouts as the package: image (H, W, C), one grid (12, gz, gy, gx), all grids
(n, 12, gz, gy, gx).

The interpolation coordinates are evaluated in float32, as `_bgrid_coords` does (bilateral_grid.jl:122-150): which cell a
pixel falls in, and whether its guidance coordinate saturates or lands on a cell, are decided by those fp32 values; every
product and sum after that is float64."""
import numpy as np

C2G = (np.float32(0.299), np.float32(0.587), np.float32(0.114))
f32 = np.float32


def _axis(n, g):
    i = np.arange(n, dtype=np.float32)
    return (i / f32(n - 1)) * f32(g - 1) if n > 1 else np.zeros(n, np.float32)


def coords(image, gx, gy, gz):
    """-> dict of sanitized rgb s (H, W, 3) f64, corner indices, fractions (f64) and z_interior, as _bgrid_coords."""
    H, W = image.shape[:2]
    s = image[..., :3].astype(np.float32)
    s = np.where(np.isfinite(s), s, f32(0.5))
    x = np.broadcast_to(_axis(W, gx)[None, :], (H, W))
    y = np.broadcast_to(_axis(H, gy)[:, None], (H, W))
    with np.errstate(over="ignore", invalid="ignore"):
        g = (C2G[0] * s[..., 0] + C2G[1] * s[..., 1]) + C2G[2] * s[..., 2]
    g = np.minimum(np.maximum(g, f32(0.0)), f32(1.0)).astype(np.float32)
    z = (g * f32(gz - 1)).astype(np.float32)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    z0 = np.clip(np.floor(z).astype(np.int64), 0, gz - 1)
    x1, y1, z1 = np.minimum(x0 + 1, gx - 1), np.minimum(y0 + 1, gy - 1), np.minimum(z0 + 1, gz - 1)
    fx = (x - x0.astype(np.float32)).astype(np.float64)
    fy = (y - y0.astype(np.float32)).astype(np.float64)
    fz = (z - z0.astype(np.float32)).astype(np.float64)
    zi = (z0.astype(np.float32) != z) & (z1.astype(np.float32) != z)
    return dict(s=s.astype(np.float64), x=(x0, x1), y=(y0, y1), z=(z0, z1), fx=fx, fy=fy, fz=fz, z_interior=zi)


def _corners(c, gz):
    for corner in range(8):
        xc, yc, zc = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
        wxy = (c["fx"] if xc else 1 - c["fx"]) * (c["fy"] if yc else 1 - c["fy"])
        wt = wxy * (c["fz"] if zc else 1 - c["fz"])
        dwdz = wxy * (1.0 if zc else -1.0) * (gz - 1)
        yield c["x"][xc], c["y"][yc], c["z"][zc], wt, dwdz


def slice_forward(image, grid):
    """bilateral_slice(image, grid): (H, W, C) -> (H, W, C) float64; channels >= 3 copied."""
    gz, gy, gx = grid.shape[1:]
    c = coords(image, gx, gy, gz)
    G = grid.astype(np.float64)
    s4 = [c["s"][..., 0], c["s"][..., 1], c["s"][..., 2], np.ones_like(c["fx"])]
    out = image.astype(np.float64).copy()
    acc = np.zeros(image.shape[:2] + (3,))
    for xi, yi, zi, wt, _ in _corners(c, gz):
        for d in range(3):
            for si in range(4):
                acc[..., d] += G[d * 4 + si, zi, yi, xi] * wt * s4[si]
    out[..., :3] = np.where(np.isfinite(acc), acc, 0.5)
    return out


def slice_backward(image, grid, vout):
    """The pullback: -> (∇image (H, W, C) with channels >= 3 = vout's, ∇grid (12, gz, gy, gx)), float64."""
    gz, gy, gx = grid.shape[1:]
    c = coords(image, gx, gy, gz)
    G = grid.astype(np.float64)
    d = vout[..., :3].astype(np.float64)
    d = np.where(np.isfinite(d), d, 0.0)
    s4 = [c["s"][..., 0], c["s"][..., 1], c["s"][..., 2], np.ones_like(c["fx"])]
    gs = np.zeros(image.shape[:2] + (3,))
    gzs = np.zeros(image.shape[:2])
    vgrid = np.zeros(G.shape)
    for xi, yi, zi, wt, dwdz in _corners(c, gz):
        for di in range(3):
            for si in range(4):
                ci = di * 4 + si
                v = G[ci, zi, yi, xi]
                gb = s4[si] * d[..., di]
                if si < 3:
                    gs[..., si] += v * wt * d[..., di]
                gzs += dwdz * v * gb
                flat = (zi * gy + yi) * gx + xi
                vgrid[ci] += np.bincount(flat.ravel(), weights=(wt * gb).ravel(), minlength=gz * gy * gx).reshape(gz, gy, gx)
    gzs = np.where(c["z_interior"], gzs, 0.0)
    vimage = vout.astype(np.float64).copy()
    for k in range(3):
        vimage[..., k] = gs[..., k] + float(C2G[k]) * gzs
    return vimage, vgrid


def slice_forward_terms(image, grid):
    """What a per-pixel bound on the forward slice needs: -> (acc, A), both (H, W, 3) float64.  acc is the sum
    Σ G·wt·s4 over the 8 corners x 4 inputs BEFORE the finite check of slice_forward, A the sum of the absolute values
    of the same 32 terms."""
    gz, gy, gx = grid.shape[1:]
    c = coords(image, gx, gy, gz)
    G = grid.astype(np.float64)
    s4 = [c["s"][..., 0], c["s"][..., 1], c["s"][..., 2], np.ones_like(c["fx"])]
    acc = np.zeros(image.shape[:2] + (3,))
    A = np.zeros(image.shape[:2] + (3,))
    for xi, yi, zi, wt, _ in _corners(c, gz):
        for d in range(3):
            for si in range(4):
                t = G[d * 4 + si, zi, yi, xi] * wt * s4[si]
                acc[..., d] += t
                A[..., d] += np.abs(t)
    return acc, A


def slice_backward_terms(image, grid, vout):
    """The pullback of slice_backward with what an entry-by-entry bound needs.  -> dict of float64 arrays:
      vimage (H, W, C), vgrid (12, gz, gy, gx)   the sums, as slice_backward gives them
      vgrid_abs (12, gz, gy, gx)                 Σ|wt·s4·d| over the (pixel, corner) terms of the entry
      vgrid_count (12, gz, gy, gx) int64         the number of those terms with wt != 0
      gs_abs (H, W, 3)                           Σ|v·wt·d| over the 8 corners x 3 outputs, per input channel
      gz_abs (H, W)                              Σ|dwdz·v·gb| over the 96 terms; 0 where z_interior is False
    so that |∇image[..., k]|'s terms sum to gs_abs[..., k] + C2G[k]·gz_abs.  Cell, level, saturation and z_interior are
    decided by the fp32 coordinates of coords(), every product and sum is float64."""
    gz, gy, gx = grid.shape[1:]
    c = coords(image, gx, gy, gz)
    G = grid.astype(np.float64)
    d = vout[..., :3].astype(np.float64)
    d = np.where(np.isfinite(d), d, 0.0)
    s4 = [c["s"][..., 0], c["s"][..., 1], c["s"][..., 2], np.ones_like(c["fx"])]
    ng = gz * gy * gx
    gs, gs_abs = np.zeros(image.shape[:2] + (3,)), np.zeros(image.shape[:2] + (3,))
    gzs, gz_abs = np.zeros(image.shape[:2]), np.zeros(image.shape[:2])
    vgrid, vgrid_abs, count = np.zeros(G.shape), np.zeros(G.shape), np.zeros(G.shape, np.int64)
    for xi, yi, zi, wt, dwdz in _corners(c, gz):
        flat = ((zi * gy + yi) * gx + xi).ravel()
        hit = np.bincount(flat, weights=(wt != 0).ravel().astype(np.float64), minlength=ng).astype(np.int64).reshape(gz, gy, gx)
        for di in range(3):
            for si in range(4):
                ci = di * 4 + si
                v = G[ci, zi, yi, xi]
                gb = s4[si] * d[..., di]
                if si < 3:
                    t = v * wt * d[..., di]
                    gs[..., si] += t
                    gs_abs[..., si] += np.abs(t)
                t = dwdz * v * gb
                gzs += t
                gz_abs += np.abs(t)
                t = (wt * gb).ravel()
                vgrid[ci] += np.bincount(flat, weights=t, minlength=ng).reshape(gz, gy, gx)
                vgrid_abs[ci] += np.bincount(flat, weights=np.abs(t), minlength=ng).reshape(gz, gy, gx)
                count[ci] += hit
    gzs = np.where(c["z_interior"], gzs, 0.0)
    gz_abs = np.where(c["z_interior"], gz_abs, 0.0)
    vimage = vout.astype(np.float64).copy()
    for k in range(3):
        vimage[..., k] = gs[..., k] + float(C2G[k]) * gzs
    return dict(vimage=vimage, vgrid=vgrid, vgrid_abs=vgrid_abs, vgrid_count=count, gs_abs=gs_abs, gz_abs=gz_abs)


def tv_loss(grids):
    """tv_loss(grids) (bilateral_grid.jl:106-119), grids (n, 12, gz, gy, gx)."""
    n, _, gz, gy, gx = grids.shape
    a = grids.astype(np.float64)
    dx, dy, dz = np.diff(a, axis=4), np.diff(a, axis=3), np.diff(a, axis=2)
    return ((dx ** 2).sum() / max(1, (gx - 1) * gy * gz) + (dy ** 2).sum() / max(1, gx * (gy - 1) * gz)
            + (dz ** 2).sum() / max(1, gx * gy * (gz - 1))) / (12 * n)


def tv_grad(grids):
    n, _, gz, gy, gx = grids.shape
    a = grids.astype(np.float64)
    g = np.zeros_like(a)
    for axis, norm in ((4, max(1, (gx - 1) * gy * gz)), (3, max(1, gx * (gy - 1) * gz)), (2, max(1, gx * gy * (gz - 1)))):
        d = np.diff(a, axis=axis) * (2.0 / (norm * 12 * n))
        lo = [slice(None)] * 5
        hi = [slice(None)] * 5
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        g[tuple(lo)] -= d
        g[tuple(hi)] += d
    return g


def tv_grad_terms(grids):
    """-> (tv_grad(grids), A): A[entry] is the sum of the absolute values of the (up to six) scaled differences that enter
    the entry, 2/(norm·12·n)·|a[e] - a[neighbour]| over its neighbours along x, y and z."""
    n, _, gz, gy, gx = grids.shape
    a = grids.astype(np.float64)
    g, A = np.zeros_like(a), np.zeros_like(a)
    for axis, norm in ((4, max(1, (gx - 1) * gy * gz)), (3, max(1, gx * (gy - 1) * gz)), (2, max(1, gx * gy * (gz - 1)))):
        d = np.diff(a, axis=axis) * (2.0 / (norm * 12 * n))
        lo = [slice(None)] * 5
        hi = [slice(None)] * 5
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        g[tuple(lo)] -= d
        g[tuple(hi)] += d
        A[tuple(lo)] += np.abs(d)
        A[tuple(hi)] += np.abs(d)
    return g, A


def identity_grids(n, gx, gy, gz):
    g = np.zeros((n, 12, gz, gy, gx), np.float32)
    for d in range(3):
        g[:, d * 4 + d] = 1.0
    return g
