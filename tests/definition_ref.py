"""The forward's discrete structure and image from a per-pixel float64 DEFINITION, independent of
oracle/gsr_oracle.c: no keys, no prefix sums, no sort, no ranges array on the way.

  decide       per-Gaussian decisions (cull, radius, tile rect) in float64, each with its margin to the boundary it was decided on
  robust_scene the scene without the Gaussians whose own decisions sit on a rounding boundary (`fragile_gaussian`)
  tile_lists   per tile: the ids with rmin <= tile < rmax, ordered by (z, id); n_rendered / values_sorted / ranges by concatenation
  render       the A.8 walk per pixel in float64; flags the pixels whose skip / stop decisions sit on a boundary (`fragile_pixel`)
  blendable    per (tile, Gaussian) entry: does it surely / surely not reach alpha >= 1/255 on some in-image pixel of the tile
  define       all of it for one scene;  check_against_definition: the comparator of tests/test_definition_cpu.py and
               tests/test_gpu_definition.py

An fp32 evaluation (the oracle, the kernels, the reference) decides `near < z`, `ceil(3 sqrt(lambda))`, `floor((mu - r) / 16)` ...
on fp32 roundings of the quantities below.  Both are right wherever the float64 value is further from the boundary than the fp32
rounding error, and neither is "the" answer closer than that: those inputs are REMOVED (robust_scene), on both sides of every
comparison, instead of being tolerated.  What remains is compared exactly.

Imports: numpy, torch (float64), f64_model (per-Gaussian primal maths), fuzz_scenes and the plain Camera dataclass.  Nothing here
computes with the oracle or the product."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import torch

import f64_model as fm

EPS32 = float(np.finfo(np.float32).eps)
ALPHA_MIN = float(np.float32(1.0) / np.float32(255.0))   # A.1: the fp32 constant 1f0 / 255f0
ALPHA_MAX, T_MIN = float(np.float32(0.99)), float(np.float32(1e-4))
WINDOW = 1e-4          # relative window of a per-Gaussian decision
SIGMA_ULPS = 64        # blend-test window in fp32 ulps of the largest term (hip_helpers.blend_boundary_pixels uses 4 on fp32 inputs)
T_WINDOW = 1e-3        # relative window of the T' < 1e-4 stop and of the covisibility test T > 0.5
BLEND_MARGIN = 1e-3    # `blendable`: surely above (1 + m) / 255, surely not below (1 - m) / 255
MAX_REMOVED, MAX_UNDECIDED = 0.05, 0.02
CHANNELS = {"rgb": 3, "rgbd": 5, "rgbdn": 8}


def _f32(x):
    """The value an fp32 evaluation receives, as float64 (camera parameters cross the C ABI as fp32)."""
    return np.asarray(np.asarray(x, np.float32), np.float64)


def _tt(a):
    return torch.as_tensor(np.asarray(a, np.float64), dtype=fm.DT)


def _near_int(x, scale=None):
    """|x - nearest integer| within WINDOW relative (of max(|x|, 1) unless `scale` is given); also the nearest integer."""
    k = np.rint(x)
    s = np.maximum(np.abs(x), 1.0) if scale is None else scale
    return np.abs(x - k) <= WINDOW * s, k


def tile_rect(mu, radius, grid):
    """A.4: rmin = clamp(floor((mu - r) / 16), 0, grid), rmax = clamp(floor((mu + r + 16 - 1) / 16), 0, grid) — the ceil-div is the
    float one — for (N, 2) `mu`, (N,) `radius`, (2,) `grid`; also the two unfloored quotients."""
    mu, radius = np.asarray(mu, np.float64), np.asarray(radius, np.float64)
    fmin, fmax = (mu - radius[:, None]) / 16.0, (mu + radius[:, None] + 15.0) / 16.0
    grid = np.asarray(grid, np.float64)
    return np.clip(np.floor(fmin), 0, grid), np.clip(np.floor(fmax), 0, grid), fmin, fmax


def decide(means, scales, rots, cam):
    """Per-Gaussian decisions of A.2 / A.4 in float64.  Returns a namespace of (N,) / (N, k) numpy arrays:
    z, mu (N, 2), cov2 (N, 2, 2: Sigma_2 + eps I), conic (N, 3: a, b, c), det, lam, r3 (= 3 sqrt(lambda)), radius (ceil(r3), before
    any cull), visible, radii (radius where visible, else 0), rect (N, 4: x0, y0, x1, y1; zeros where culled), tiles_touched,
    fragile_gaussian, and the (3,) `zrow`, `tz` of p_c.z = zrow . p + tz."""
    n = np.asarray(means).shape[0]
    W, H = int(cam.width), int(cam.height)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    R, t = _f32(cam.R), _f32(cam.t)
    near, far, eps = float(_f32(cam.near_plane)), float(_f32(cam.far_plane)), float(_f32(cam.blur_eps))
    p = _f32(means)
    pc = p @ R.T + t
    z = pc[:, 2]
    with np.errstate(all="ignore"):
        Sig = fm.quat_scale_to_cov(_tt(_f32(rots)), _tt(_f32(scales)))
        Rt = _tt(R)
        S2, m2 = fm.perspective_projection(_tt(pc), Rt @ Sig @ Rt.T, _tt(_f32(cam.focal)), (W, H), _tt(_f32(cam.principal)))
        cov2 = S2.numpy() + eps * np.eye(2)
        mu = m2.numpy()
        a, b, c = cov2[:, 0, 0], 0.5 * (cov2[:, 0, 1] + cov2[:, 1, 0]), cov2[:, 1, 1]
        det = a * c - b * b
        mid = 0.5 * (a + c)
        lam = mid + np.sqrt(np.maximum(0.1, mid * mid - det))
        r3 = 3.0 * np.sqrt(lam)
        radius = np.ceil(r3)
        conic = np.stack([c / det, -b / det, a / det], 1)
        in_z = (z > near) & (z < far)
        lo, hi = mu - radius[:, None], mu + radius[:, None]
        on = (hi[:, 0] > 0) & (lo[:, 0] < W) & (hi[:, 1] > 0) & (lo[:, 1] < H)
        visible = in_z & (det > 0) & (radius > cam.radius_clip) & on & np.isfinite(r3) & np.isfinite(mu).all(1)
        grid = np.array([gx, gy], np.float64)
        rmin, rmax, fmin, fmax = tile_rect(mu, radius, grid)
        # ---- margins ----
        frag_z = (np.abs(z - near) <= WINDOW * near) | (np.abs(z - far) <= WINDOW * far)
        frag_r, _ = _near_int(r3)
        sc = np.maximum(np.abs(mu), radius[:, None])
        size = np.array([W, H], np.float64)
        frag_on = ((np.abs(hi) <= WINDOW * sc) | (np.abs(lo - size) <= WINDOW * np.maximum(sc, size))).any(1)
        # a floor that lands on k - 1 or k gives another clamped value only for 1 <= k <= grid
        nmin, kmin = _near_int(fmin)
        nmax, kmax = _near_int(fmax)
        frag_rect = ((nmin & (kmin >= 1) & (kmin <= grid)) | (nmax & (kmax >= 1) & (kmax <= grid))).any(1)
    reached = np.isfinite(z) & ((z > near * (1 - WINDOW)) & (z < far * (1 + WINDOW)))   # the later decisions are taken at all
    big = radius > cam.radius_clip
    fragile = frag_z | (reached & np.nan_to_num(det > 0) & (frag_r | (big & (frag_on | (on & frag_rect)))))
    radii = np.where(visible, radius, 0).astype(np.int32)
    rect = np.where(visible[:, None], np.concatenate([rmin, rmax], 1), 0).astype(np.int64)
    d = SimpleNamespace(n=n, W=W, H=H, grid=(gx, gy), z=z, mu=mu, cov2=cov2, conic=conic, det=det, lam=lam, r3=r3, radius=radius,
                        visible=visible, radii=radii, rect=rect, pc=pc, zrow=R[2], tz=float(t[2]),
                        tiles_touched=((rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])).astype(np.int32))
    d.fragile_gaussian = fragile | _depth_near_ties(d, p)
    return d


def _depth_near_ties(d, p):
    """For two visible Gaussians that share a tile and whose float64 depths differ by less than 8 eps32 (sum |R3j pj| + |tz|) — a
    few fp32 roundings of the dot product behind z — but are NOT equal: the one with the higher id.  Exactly equal depths are a
    defined case (A.6: id order) and stay."""
    out = np.zeros(d.n, bool)
    vis = np.flatnonzero(d.visible)
    if vis.size < 2:
        return out
    order = vis[np.lexsort((vis, d.z[vis]))]
    zs = d.z[order]
    win = 8.0 * EPS32 * (np.abs(p[order] * d.zrow).sum(1) + abs(d.tz))
    rc = d.rect[order]
    k = 1
    while k < order.size:
        dz = zs[k:] - zs[:-k]
        close = dz < np.maximum(win[k:], win[:-k])
        if not close.any():
            break                                   # zs ascends: no pair further apart in the order is closer in depth
        a, b = rc[:-k], rc[k:]
        share = (a[:, 0] < b[:, 2]) & (b[:, 0] < a[:, 2]) & (a[:, 1] < b[:, 3]) & (b[:, 1] < a[:, 3])
        hit = close & (dz > 0) & share
        out[np.maximum(order[k:], order[:-k])[hit]] = True
        k += 1
    return out


def robust_scene(fs):
    """`fs` (a fuzz_scenes.FuzzScene) without its fragile Gaussians, in every per-Gaussian array: a pure function of the scene, so
    that both sides of a comparison get the same inputs.  `note["removed"]` = (removed, of)."""
    d = decide(fs.means, fs.scales, fs.rots, fs.cam)
    keep = ~d.fragile_gaussian
    n = d.n
    cut = lambda a: np.ascontiguousarray(a[keep]) if isinstance(a, np.ndarray) and a.shape[:1] == (n,) else a  # noqa: E731
    note = {k: cut(v) for k, v in fs.note.items()}
    note["removed"] = (int(n - keep.sum()), n)
    out = dataclasses.replace(fs, means=cut(fs.means), shs=cut(fs.shs), opac=cut(np.asarray(fs.opac)),
                              scales=cut(fs.scales), rots=cut(fs.rots), note=note)
    again = decide(out.means, out.scales, out.rots, out.cam)
    assert not again.fragile_gaussian.any(), "the filter must leave nothing fragile behind"
    return out


def tile_lists(d):
    """Per tile (row-major, tile = ty * grid.x + tx): the visible ids with rmin <= (tx, ty) < rmax, ordered by (z, id).  Returns a
    namespace: lists (one int64 array per tile), n_rendered, tiles_touched, values_sorted (uint32), ranges (tiles, 2: uint32,
    (0, 0) for empty tiles, A.7)."""
    gx, gy = d.grid
    vis = np.flatnonzero(d.visible)
    rc, zv = d.rect[vis], d.z[vis]
    lists = []
    for ty in range(gy):
        in_y = (rc[:, 1] <= ty) & (ty < rc[:, 3])
        for tx in range(gx):
            m = in_y & (rc[:, 0] <= tx) & (tx < rc[:, 2])
            ids = vis[m]
            lists.append(ids[np.lexsort((ids, zv[m]))])
    lengths = np.array([len(l) for l in lists], np.int64)
    ends = np.cumsum(lengths)
    ranges = np.stack([ends - lengths, ends], 1)
    ranges[lengths == 0] = 0
    values = np.concatenate(lists).astype(np.uint32) if lists else np.zeros(0, np.uint32)
    return SimpleNamespace(lists=lists, n_rendered=int(lengths.sum()), tiles_touched=d.tiles_touched, values_sorted=values,
                           ranges=ranges.astype(np.uint32))


def features(d, means, shs, scales, rots, cam, deg, mode):
    """(N, C) float64 features of A.3 / A.8: max(0, SH + 0.5 + eps(Float32)) | z | 1 | the flipped normal of the shortest axis."""
    with np.errstate(all="ignore"):
        dirs = _tt(_f32(means) - _f32(cam.camera_center))
        dirs = dirs / dirs.norm(dim=-1, keepdim=True)
        basis = fm.sh_basis(dirs, deg).numpy()
        col = (basis[:, :, None] * _f32(shs)[:, :basis.shape[1], :]).sum(1) + 0.5 + EPS32
        out = [np.maximum(col, 0.0)]
        if CHANNELS[mode] > 3:
            out += [d.z[:, None], np.ones((d.n, 1))]
        if CHANNELS[mode] > 5:
            Rg = fm.quat2rot(_tt(_f32(rots))).numpy()
            k = np.argmin(_f32(scales), 1)                       # first minimum on ties
            ncam = Rg[np.arange(d.n), :, k] @ _f32(cam.R).T
            flip = (ncam * d.pc).sum(1) > 0
            out += [np.where(flip[:, None], -ncam, ncam)]
    return np.concatenate(out, 1)


def _tile_pixels(d, t):
    gx = d.grid[0]
    y0, x0 = (t // gx) * 16, (t % gx) * 16
    ys, xs = np.mgrid[y0:min(y0 + 16, d.H), x0:min(x0 + 16, d.W)]
    return ys.reshape(-1), xs.reshape(-1)


def _sigma(d, ids, ys, xs):
    """sigma (pixels, entries) and the magnitude of its largest term."""
    dx = d.mu[ids, 0][None, :] - xs[:, None].astype(np.float64)
    dy = d.mu[ids, 1][None, :] - ys[:, None].astype(np.float64)
    a, b, c = d.conic[ids, 0], d.conic[ids, 1], d.conic[ids, 2]
    t_xy, t_xx, t_yy = b * dx * dy, 0.5 * a * dx * dx, 0.5 * c * dy * dy
    return t_xy + (t_xx + t_yy), np.maximum(np.abs(t_xy), np.maximum(np.abs(t_xx), np.abs(t_yy)))


def render(d, tl, feat, opac, background, want_uncertainty=False, want_covisibility=False):
    """A.8 per pixel in float64 over the lists `tl`.  Returns a namespace: image (H, W, C), T (H, W), n_contrib (H, W: the 1-based
    list position of the last blended entry, skipped ones counted; 0 if none), fragile_pixel (H, W), weights (one (pixels, entries)
    array of blend weights alpha T per tile, for the comparator's own test), and optionally uncertainty (H, W), covisibility (N,)
    and covis_fragile (N,: Gaussians with a blended pixel at |T - 0.5| <= 1e-3 · 0.5).

    fragile_pixel: some entry met before the pixel's stop (the stopping entry included) has
      |sigma - ln(255 o)| <= 64 eps32 max(|sigma's terms|, |ln(255 o)|)   (o >= 1/255 only: alpha <= o, no boundary below), or
      sigma <= 64 eps32 max|sigma's terms| with o >= 1/255 (the `sigma < 0` skip, decided by fp32 cancellation), or
      |T' - 1e-4| <= 1e-3 · 1e-4 on an entry that passed the alpha test;  with covisibility, |T - 0.5| <= 1e-3 · 0.5 on a blended one."""
    C = feat.shape[1]
    o_all = _f32(opac).reshape(-1)
    bg = np.zeros(C)
    bg[:3] = _f32(background)
    img = np.zeros((d.H, d.W, C))
    Tout = np.ones((d.H, d.W))
    nc = np.zeros((d.H, d.W), np.int64)
    frag = np.zeros((d.H, d.W), bool)
    unc = np.zeros((d.H, d.W)) if want_uncertainty else None
    cov = np.zeros(d.n, bool) if want_covisibility else None
    cov_frag = np.zeros(d.n, bool) if want_covisibility else None
    weights = []
    for t, ids in enumerate(tl.lists):
        ys, xs = _tile_pixels(d, t)
        if tl.n_rendered == 0:
            Tout[ys, xs] = 0.0          # rasterizer.jl:338: nothing to render leaves the zero-filled outputs
            weights.append(np.zeros((ys.size, 0)))
            continue
        if ids.size == 0:
            img[ys, xs] = bg
            weights.append(np.zeros((ys.size, 0)))
            continue
        o = o_all[ids]
        sig, big = _sigma(d, ids, ys, xs)
        with np.errstate(all="ignore"):
            alpha = np.minimum(ALPHA_MAX, o[None, :] * np.exp(-sig))
            tau = np.log(255.0 * o)
        keep = (sig >= 0) & (alpha >= ALPHA_MIN)
        al = np.where(keep, alpha, 0.0)
        Tn = np.cumprod(1.0 - al, 1)                              # T' after each entry, were it blended
        stop = keep & (Tn < T_MIN)
        dead = np.cumsum(stop, 1) > 0                             # the stopping entry and everything behind it
        met = ~dead | (stop & (np.cumsum(stop, 1) == 1))          # entries the walk looks at
        blended = keep & ~dead
        al = np.where(blended, al, 0.0)
        Tincl = np.cumprod(1.0 - al, 1)
        Texcl = np.concatenate([np.ones((ys.size, 1)), Tincl[:, :-1]], 1)
        w = al * Texcl
        weights.append(w)
        img[ys, xs] = w @ feat[ids] + Tincl[:, -1:] * bg
        Tout[ys, xs] = Tincl[:, -1]
        pos = np.arange(1, ids.size + 1)
        nc[ys, xs] = (blended * pos).max(1)
        can = (o >= ALPHA_MIN)[None, :] & np.isfinite(tau)[None, :]
        with np.errstate(invalid="ignore"):
            near_a = can & (np.abs(sig - tau[None, :]) <= SIGMA_ULPS * EPS32 * np.maximum(big, np.abs(tau)[None, :]))
        near_0 = can & (sig <= SIGMA_ULPS * EPS32 * big)
        near_t = keep & (np.abs(Tn - T_MIN) <= T_WINDOW * T_MIN)
        f = met & (near_a | near_0 | near_t)
        if want_covisibility:
            half = blended & (np.abs(Texcl - 0.5) <= T_WINDOW * 0.5)
            f |= half
            cov_frag[ids[half.any(0)]] = True
            cov[ids[(blended & (Texcl > 0.5)).any(0)]] = True
        frag[ys, xs] = f.any(1)
        if want_uncertainty:
            unc[ys, xs] = w.sum(1)
    return SimpleNamespace(image=img, T=Tout, n_contrib=nc, fragile_pixel=frag, weights=weights, uncertainty=unc, covisibility=cov,
                           covis_fragile=cov_frag)


def blendable(d, tl, opac):
    """Per tile, per entry of its list: +1 `surely` (some in-image pixel of the tile has alpha >= (1 + 1e-3) / 255), -1 `surely not`
    (every one has alpha <= (1 - 1e-3) / 255), 0 undecided.  A list of int8 arrays parallel to tl.lists."""
    o_all = _f32(opac).reshape(-1)
    out = []
    for t, ids in enumerate(tl.lists):
        if ids.size == 0:
            out.append(np.zeros(0, np.int8))
            continue
        ys, xs = _tile_pixels(d, t)
        sig, _ = _sigma(d, ids, ys, xs)
        with np.errstate(all="ignore"):
            amax = np.where(sig >= 0, np.minimum(ALPHA_MAX, o_all[ids][None, :] * np.exp(-sig)), 0.0).max(0)
        out.append(np.where(amax >= (1 + BLEND_MARGIN) / 255.0, 1, np.where(amax <= (1 - BLEND_MARGIN) / 255.0, -1, 0)).astype(np.int8))
    return out


def define(fs, want_uncertainty=False, want_covisibility=False):
    """The whole definition of one (already filtered) scene: decision `d`, lists `tl`, render result `r`, `blend` and the measured
    shares; `got()` makes the record check_against_definition compares, from the definition itself."""
    d = decide(fs.means, fs.scales, fs.rots, fs.cam)
    tl = tile_lists(d)
    feat = features(d, fs.means, fs.shs, fs.scales, fs.rots, fs.cam, fs.deg, fs.mode)
    r = render(d, tl, feat, fs.opac, fs.bg, want_uncertainty, want_covisibility)
    blend = blendable(d, tl, fs.opac)
    entries = max(1, tl.n_rendered)
    undecided = int(sum(int((b == 0).sum()) for b in blend))
    shares = dict(removed=fs.note.get("removed", (0, d.n)), fragile_pixels=(int(r.fragile_pixel.sum()), d.W * d.H),
                  undecided=(undecided, tl.n_rendered), longest=int(max((len(l) for l in tl.lists), default=0)))
    fmax = float(max(1.0, np.abs(r.image).max()))
    return SimpleNamespace(fs=fs, d=d, tl=tl, feat=feat, r=r, blend=blend, shares=shares, fmax=fmax, entries=entries)


def conditions(defn):
    """The caps a scene must meet to be used at all, on the definition alone; prints the measured shares."""
    s = defn.shares
    print(f"definition: removed {s['removed'][0]} of {s['removed'][1]} Gaussians, fragile pixels {s['fragile_pixels'][0]} of "
          f"{s['fragile_pixels'][1]}, undecided entries {s['undecided'][0]} of {s['undecided'][1]}, longest list {s['longest']}")
    assert s["removed"][0] <= MAX_REMOVED * s["removed"][1], s
    assert s["fragile_pixels"][0] <= max(4, 0.02 * s["fragile_pixels"][1]), s
    assert s["undecided"][0] <= MAX_UNDECIDED * max(1, s["undecided"][1]), s
    assert not defn.d.fragile_gaussian.any()


def got_from_definition(defn):
    """The record of a forward that computes exactly what the definition does (writable copies: the mutation tests corrupt it)."""
    d, tl, r = defn.d, defn.tl, defn.r
    return SimpleNamespace(radii=d.radii.copy(), tiles_touched=d.tiles_touched.copy(), rect=d.rect.copy(), n_rendered=tl.n_rendered,
                           values_sorted=tl.values_sorted.copy(), ranges=tl.ranges.copy(), image=r.image.copy(), T=r.T.copy(),
                           n_contrib=r.n_contrib.copy())


def _got_lists(got, tiles):
    rg = np.asarray(got.ranges).astype(np.int64)
    vals = np.asarray(got.values_sorted).astype(np.int64)
    assert rg.shape == (tiles, 2), rg.shape
    assert (rg[:, 0] <= rg[:, 1]).all() and (rg >= 0).all() and (rg <= vals.size).all(), "ranges outside the sorted list"
    return [vals[a:b] for a, b in rg], rg


def check_against_definition(defn, got, lists="reference", outliers=0.0):
    """`got` (radii, tiles_touched, rect or None, n_rendered, values_sorted, ranges, image, T, n_contrib) against the definition.

    lists="reference": radii, tiles_touched, rect, n_rendered, values_sorted and ranges are the definition's, exactly.
    lists="culled":    radii, tiles_touched and rect exactly; the ranges tile the sorted list; every list is an order-preserving
                       subsequence of the definition's and holds every `surely` entry (so nothing the definition's rect excludes,
                       surely-not or otherwise, can be in it).
    Both: n_contrib names the definition's last blended entry on every non-fragile pixel; image and T on the non-fragile pixels
    within 1e-4 · fmax resp. 1e-4 except a share `outliers` of their values, which (like the fragile pixels) stay within
    2 / 255 · fmax resp. 2 / 255 — fmax = max(1, largest feature value of the definition's image).  Returns the measured figures."""
    d, tl, r = defn.d, defn.tl, defn.r
    tiles = d.grid[0] * d.grid[1]
    assert np.array_equal(np.asarray(got.radii).astype(np.int64), d.radii), "radii differ from ceil(3 sqrt(lambda)) / the cull"
    assert np.array_equal(np.asarray(got.tiles_touched).astype(np.int64)[d.visible], d.tiles_touched[d.visible]), "tiles per Gaussian"
    if got.rect is not None:
        assert np.array_equal(np.asarray(got.rect).astype(np.int64)[d.visible], d.rect[d.visible]), "tile rects"
    glists, rg = _got_lists(got, tiles)
    vals = np.asarray(got.values_sorted).astype(np.int64)
    assert int(got.n_rendered) == vals.size
    if lists == "reference":
        assert int(got.n_rendered) == tl.n_rendered, (got.n_rendered, tl.n_rendered)
        assert np.array_equal(vals, tl.values_sorted.astype(np.int64)), "sorted ids"
        assert np.array_equal(rg, tl.ranges.astype(np.int64)), "ranges"
    else:
        assert lists == "culled"
        assert sum(len(g) for g in glists) == vals.size, "the ranges do not tile the sorted list"
        for t, (g, ref, bl) in enumerate(zip(glists, tl.lists, defn.blend)):
            assert np.unique(g).size == g.size, f"tile {t}: an id twice"
            assert np.array_equal(ref[np.isin(ref, g)], g), f"tile {t}: not an order-preserving subsequence of the definition's list"
            assert np.isin(ref[bl > 0], g).all(), f"tile {t}: a surely blending entry is missing"
    # ---- per pixel ----
    ok = ~r.fragile_pixel
    nc = np.asarray(got.n_contrib).astype(np.int64).reshape(d.H, d.W)
    last_ref = np.full((d.H, d.W), -1, np.int64)
    last_got = np.full((d.H, d.W), -1, np.int64)
    for t in range(tiles):
        ys, xs = _tile_pixels(d, t)
        for dst, lst, cnt in ((last_ref, tl.lists[t], r.n_contrib[ys, xs]), (last_got, glists[t], nc[ys, xs])):
            assert (cnt <= len(lst)).all() and (cnt >= 0).all(), f"tile {t}: n_contrib beyond the list"
            if len(lst):
                dst[ys, xs] = np.where(cnt > 0, lst[np.maximum(cnt, 1) - 1], -1)
    bad_nc = ok & (last_ref != last_got)
    assert not bad_nc.any(), f"n_contrib differs on {int(bad_nc.sum())} non-fragile pixels, first at {np.argwhere(bad_nc)[0]}"
    im = np.asarray(got.image, np.float64).reshape(r.image.shape)
    T = np.asarray(got.T, np.float64).reshape(d.H, d.W)
    tol, loose = 1e-4 * defn.fmax, 2.0 / 255.0 * defn.fmax
    di, dT = np.abs(im - r.image).max(2), np.abs(T - r.T)
    assert np.isfinite(im).all() and np.isfinite(T).all()
    n_ok = max(1, int(ok.sum()))
    out_i, out_T = int((ok & (di > tol)).sum()), int((ok & (dT > 1e-4)).sum())
    worst = float(di[ok].max()) if ok.any() else 0.0
    worst_T = float(dT[ok].max()) if ok.any() else 0.0
    assert out_i <= outliers * n_ok, f"image: {out_i} of {n_ok} non-fragile pixels beyond {tol:.3g} (worst {worst:.3g})"
    assert out_T <= outliers * n_ok, f"T: {out_T} of {n_ok} non-fragile pixels beyond 1e-4 (worst {worst_T:.3g})"
    assert di.max() <= loose and dT.max() <= 2.0 / 255.0, f"a pixel beyond the one-flipped-pair bound: {di.max():.3g}, {dT.max():.3g}"
    return dict(worst_image=worst, worst_T=worst_T, outliers=(out_i, out_T), fragile=int((~ok).sum()),
                worst_fragile=float(di[~ok].max()) if (~ok).any() else 0.0)


# ---- the scenes of tests/test_definition_cpu.py and tests/test_gpu_definition.py ----
# deep-276 / deep-5911: the fuzz_scenes.deep_scene cases with a longest list of 2913 resp. 4317 entries (above the 1024 and the 4096
# sort tier) that meet `conditions`.  The family's ordinary cases do not: with alpha around 0.02 each blend multiplies T by 0.98, so
# T' lands in the 0.2 % window around 1e-4 at one pixel in ten (measured: 6 .. 25 % fragile pixels); the cases whose opacities stay
# near 1/255 reach their depth without reaching the stop.
DEEP = ("deep-276", "deep-5911")
SPECIAL = ("single-tile", "ragged", "ties")
CPU_SCENES = tuple(f"sweep-{c}" for c in range(12)) + tuple(f"edge-{c}" for c in range(12)) + DEEP + SPECIAL
# one of each mode; edge-0 / edge-4: cutting near and far planes, fx != fy, an arbitrary pose
GPU_SCENES = ("sweep-3", "sweep-5", "edge-0", "edge-4", "single-tile", "ragged", "ties") + DEEP
SIDE_SCENE = "edge-9"    # :rgb, opacities 0 / 1/255 / 0.995 / 1; covisibility and uncertainty (meets the caps with the T ~ 0.5 pixels flagged)
TIE_LEVELS = 8


def build_scene(pkg, name):
    """The unfiltered FuzzScene of one name of CPU_SCENES."""
    import fuzz_scenes as fz
    from oracle.oracle import Camera
    kind, _, case = name.partition("-")
    if kind in ("sweep", "edge", "deep"):
        return getattr(fz, kind + "_scene")(pkg, int(case))
    rng = np.random.default_rng(6200)
    if name == "single-tile":       # 16 x 16: one tile, no ragged edge
        s = pkg.synthetic.make_scene(150, 16, 16, 2, 6201, sigma_px=3.0)
        return fz.FuzzScene(s.means, s.shs, s.opacities, s.scales, s.rotations, Camera(16, 16, s.focal), 2, "rgbd", (0.2, 0.5, 0.1), rng)
    if name == "ragged":            # 37 x 21: 3 x 2 tiles, the last column 5 pixels wide, the last row 5 pixels high
        s = pkg.synthetic.make_scene(400, 37, 21, 1, 6202, sigma_px=4.0)
        R, t = pkg.synthetic.view_pose(2)
        return fz.FuzzScene(s.means, s.shs, s.opacities, s.scales, s.rotations, Camera(37, 21, s.focal, R=R, t=t), 1, "rgbdn",
                            (0.3, 0.1, 0.6), rng)
    assert name == "ties"           # identity pose, depths rounded to 8 values: z is exact in fp32, every tile holds long ties
    s = pkg.synthetic.make_scene(1000, 72, 40, 1, 6203, sigma_px=3.0)
    means = s.means.copy()
    k = np.clip(np.floor((means[:, 2].astype(np.float64) - 2.0) / 10.0 * TIE_LEVELS), 0, TIE_LEVELS - 1)
    means[:, 2] = (2.0 + 10.0 * (k + 0.5) / TIE_LEVELS).astype(np.float32)
    return fz.FuzzScene(means, s.shs, s.opacities, s.scales, s.rotations, Camera(72, 40, s.focal), 1, "rgb", (0.1, 0.3, 0.2), rng)


_definitions = {}


def _freeze(x):
    for v in (x if isinstance(x, (list, tuple)) else vars(x).values() if isinstance(x, SimpleNamespace) else [x]):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, (list, SimpleNamespace)):
            _freeze(v)


def definition(pkg, name, side=False):
    """The definition of robust_scene(build_scene(name)) — with uncertainty and covisibility if `side` —: computed once, shared,
    read-only."""
    if (name, side) not in _definitions:
        fs = robust_scene(build_scene(pkg, name))
        defn = define(fs, want_uncertainty=side, want_covisibility=side)
        defn.name = name
        _freeze(defn)
        for a in (fs.means, fs.shs, fs.opac, fs.scales, fs.rots):
            a.setflags(write=False)
        _definitions[name, side] = defn
    return _definitions[name, side]
