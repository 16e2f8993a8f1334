"""Shared plumbing of the -m gpu parity tests: run the HIP path through the C ABI
(via the host mirror) on the same inputs as the oracle."""
import numpy as np
import torch


def stream():
    """The package's own stream argument (pkg._lib.stream): the current torch stream as a hipStream_t."""
    import gsr_pkg
    return gsr_pkg.load()._lib.stream()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda().contiguous()


class HipRun:
    def __init__(self, pkg, means, shs, opac, scales, rots, cam, sh_degree, background=(0, 0, 0), mode="rgb",
                 want_covis=False, want_uncert=False, pose_dev=False, exact_tile_cull=False, bins_budget_bytes=0, grad_precision=None):
        R = pkg.rasterizer
        self.pkg, self.cam, self.deg, self.bg, self.mode = pkg, cam, sh_degree, tuple(float(b) for b in background), mode
        self.camera = pkg.Camera(cam.width, cam.height, tuple(cam.focal), tuple(cam.principal), np.asarray(cam.R),
                                 np.asarray(cam.t))
        self.rast = R.GaussianRasterizer(cam.width, cam.height, mode=mode, near_plane=cam.near_plane,
                                         far_plane=cam.far_plane, exact_tile_cull=exact_tile_cull,
                                         bins_budget_bytes=bins_budget_bytes, grad_precision=grad_precision)
        self.t = [dev(means), dev(shs), dev(np.asarray(opac).reshape(-1, 1)), dev(scales), dev(rots)]
        n = means.shape[0]
        self.covis = torch.zeros(n, dtype=torch.uint8, device="cuda") if want_covis else None
        self.unc = torch.zeros(cam.height, cam.width, device="cuda") if want_uncert else None
        self.Rd = self.td = None
        if pose_dev:
            self.Rd = dev(np.asarray(cam.R, np.float32).T)  # column-major (3,3)
            self.td = dev(np.asarray(cam.t, np.float32))

    def forward(self):
        img = self.rast.forward_raw(*self.t, self.camera, self.deg, self.bg, self.Rd, self.td, self.covis, self.unc)
        torch.cuda.synchronize()
        return img

    def backward(self, vpixels):
        out = self.rast.backward_raw(dev(vpixels), *self.t, self.camera, self.deg, self.bg, self.Rd, self.td)
        torch.cuda.synchronize()
        return out


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def frac_bad(a, b, rtol, atol):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) > rtol * np.abs(b) + atol).mean())


def blend_boundary_pixels(st, opacities, W, H, ulps=4, with_ids=False):
    """Pixels of the oracle state `st` at which some (pixel, splat) pair of the tile's list sits within `ulps` ulps of the
    blend-test boundary sigma = ln(255·o) (render.jl:92-95: alpha = 1/255 exactly).  There the decision depends on the last
    bit of the exp that produced alpha — two exp implementations disagree, and so may the kernels' single-compare test
    (tile_sort_device.h blend_threshold_bits) and the oracle's libm expf.  Small-image parity tests, where ONE pixel is
    already more than the 1e-4 outlier fraction, leave these pixels out of the count (measured case: seed 103, 80x64, pixel
    (20, 31), sigma == tau bit for bit, alpha·255 == 1.0f).  Small images only (pure numpy over every tile list).
    with_ids=True: also the set of Gaussian ids that own such a pair, and the set of ALL Gaussians that blend into one of
    those pixels (alpha >= half the threshold): a flipped pair changes the transmittance of everything behind it and the
    `accum_rec` recursion of everything in front of it at that pixel (render.jl:237-258), so that is where two evaluations
    that decide the pair differently may legitimately differ."""
    mask = np.zeros((H, W), bool)
    owners, touched = set(), set()
    tw = (W + 15) // 16
    op = np.asarray(opacities, np.float32).reshape(-1)
    for t, (a, b) in enumerate(np.asarray(st.ranges)):
        if b <= a:
            continue
        ids = st.values_sorted[a:b]
        m2, con, o = st.means2d[ids], st.conics[ids], op[ids]
        with np.errstate(divide="ignore", invalid="ignore"):
            tau = np.log(np.float32(255.0) * o, dtype=np.float32)
        y0, x0 = (t // tw) * 16, (t % tw) * 16
        ys, xs = np.mgrid[y0:min(y0 + 16, H), x0:min(x0 + 16, W)]
        dx = m2[:, 0][:, None, None] - xs[None].astype(np.float32)
        dy = m2[:, 1][:, None, None] - ys[None].astype(np.float32)
        t_xy = con[:, 1][:, None, None] * dx * dy
        t_xx = np.float32(0.5) * con[:, 0][:, None, None] * dx * dx
        t_yy = np.float32(0.5) * con[:, 2][:, None, None] * dy * dy
        sig = (t_xy + (t_xx + t_yy)).astype(np.float32)
        # the window is `ulps` ulps of the LARGEST term of the sum, not of its result: a pixel 60 px from the centre of a large
        # anisotropic footprint has three terms of +-100 that cancel to sigma = 5.3 — two orders of evaluation differ by ulps of
        # 100 there (fuzz edge case 7117: the pair sits 17 ulps of tau from the boundary, 0.5 ulp of its largest term)
        with np.errstate(invalid="ignore", over="ignore"):
            scale = np.maximum(np.maximum(np.abs(t_xy), np.maximum(np.abs(t_xx), np.abs(t_yy))), np.abs(tau)[:, None, None])
            near = np.abs(sig - tau[:, None, None]) <= ulps * np.spacing(scale.astype(np.float32))
        mask[y0:y0 + 16, x0:x0 + 16] |= near.any(0)
        if with_ids and near.any():
            owners.update(int(i) for i in ids[near.reshape(len(ids), -1).any(1)])
            px = near.any(0)                                             # boundary pixels of this tile
            with np.errstate(over="ignore"):
                alpha = o[:, None, None] * np.exp(-sig)
            blends = (sig >= 0) & (alpha >= 0.5 / 255.0) & px[None]
            touched.update(int(i) for i in ids[blends.reshape(len(ids), -1).any(1)])
    return (mask, owners, touched) if with_ids else mask


def compare_forward(st, run, img, opacities=None):
    geo = {k: v.cpu().numpy() for k, v in run.rast.geometry().items()}
    radii = run.rast.radii.cpu().numpy()
    assert np.array_equal(radii, st.radii), "radii must match exactly"
    vis = st.radii > 0
    assert run.rast.stats.n_visible == int(vis.sum())
    assert run.rast.stats.n_rendered == st.n_rendered
    for name, ref in (("means2d", st.means2d), ("conics", st.conics), ("depths", st.depths), ("rgbs", st.rgbs)):
        assert frac_bad(geo[name][vis], ref[vis], 1e-6, 1e-7) == 0.0, name
    cb = geo["clamped_bits"][vis]
    ref_bits = (st.clamped[vis].astype(np.int32) * np.array([1, 2, 4])).sum(1)
    assert np.array_equal(cb, ref_bits)
    rect = geo["rect"].astype(np.int64)
    tiles = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
    assert np.array_equal(tiles[vis], st.tiles_touched[vis]), "tile counts per Gaussian must match exactly"
    assert not st.tiles_touched[~vis].any()  # records of culled Gaussians are stale, as in the reference
    if st.normals is not None:
        assert frac_bad(geo["normals"][vis], st.normals[vis], 1e-6, 1e-7) == 0.0
    if st.n_rendered > 0:
        assert np.array_equal(run.rast.ranges.cpu().numpy().astype(np.uint32), st.ranges)
        assert np.array_equal(run.rast.values_sorted.cpu().numpy().astype(np.uint32), st.values_sorted)
    im = img.cpu().numpy()
    assert im.shape == st.image.shape
    T = run.rast.accum_alpha.cpu().numpy()
    nc = run.rast.n_contrib.cpu().numpy().astype(np.uint32)
    # (the last contributor moves by one where the saturation test T' < 1e-4 is decided by the last bits of T:
    #  one such pixel is already more than 1e-3 of a 25 x 32 image)
    sat = (nc != st.n_contrib).reshape(im.shape[:2])
    assert sat.sum() <= max(1, 1e-3 * nc.size)
    if opacities is not None and im.shape[0] * im.shape[1] < 20000:
        # (one pixel of a small image is already more than the 1e-4 outlier fraction: pixels with a pair ON the blend-test
        #  boundary, where the decision is the last bit of an exp, do not count — hip_helpers.blend_boundary_pixels — and
        #  neither does the at most one pixel whose walk stopped one entry apart, fuzz sweep case 14113)
        edge = blend_boundary_pixels(st, opacities, im.shape[1], im.shape[0])
        keep = ~(edge | sat)
        # a handful of pixels, not a tenth of the image (round-3 verdict / ADVICE: the measured worst case of 9 000 fuzzed
        # scenes was 17 of 1 634 pixels = 1.04 %, under 50 763 splats per pixel)
        assert (~keep).sum() <= max(4, 0.02 * keep.size), ((~keep).sum(), keep.size)
        assert frac_bad(im[keep], st.image[keep], 0.0, 1e-4) <= 1e-4
        assert frac_bad(T[keep], st.accum_alpha[keep], 0.0, 1e-4) <= 1e-4
        fmax = float(max(1.0, np.abs(st.image).max()))
        if edge.any():
            # ... and what is excluded may only differ by ONE flipped pair: its blend weight is alpha·T <= 1/255 (+ the
            # renormalisation of what lies behind it), times the largest feature value
            assert np.abs(im[edge] - st.image[edge]).max() <= 2.0 / 255.0 * fmax
            assert np.abs(T[edge] - st.accum_alpha[edge]).max() <= 2.0 / 255.0
        if (sat & ~edge).any():
            # ... or by the ONE entry blended on one side only: at most the transmittance the other side stopped at
            left = float((1.0 - np.minimum(T, st.accum_alpha.reshape(T.shape))[sat & ~edge]).max())
            assert np.abs(im[sat & ~edge] - st.image[sat & ~edge]).max() <= 2.0 * (left + 1e-4) * fmax
            assert np.abs(T[sat & ~edge] - st.accum_alpha.reshape(T.shape)[sat & ~edge]).max() <= 2.0 * (left + 1e-4)
    else:
        assert frac_bad(im, st.image, 0.0, 1e-4) <= 1e-4, np.abs(im - st.image).max()
        assert frac_bad(T, st.accum_alpha, 0.0, 1e-4) <= 1e-4


def compare_backward(g, out, vis):
    vm, vs, vo, vsc, vr, vR, vt = [None if o is None else o.cpu().numpy() for o in out]
    assert rel_l2(vm, g.vmeans) <= 1e-4
    assert rel_l2(vs, g.vshs) <= 1e-4
    assert rel_l2(vo.reshape(-1), g.vopacities) <= 1e-4
    assert rel_l2(vsc, g.vscales) <= 1e-4
    assert rel_l2(vr, g.vrots) <= 1e-4
    # culled Gaussians: exact zeros
    assert not vm[~vis].any() and not vs[~vis].any() and not vsc[~vis].any() and not vr[~vis].any()
    return vR, vt


def pose_grad_f64(means, shs, opac, scales, rots, cam, deg, bg, mode, st, vp):
    """∇R (9 values, column-major like the library's and the oracle's vR) and ∇t (3) of the float64 autograd model
    (f64_model.render_dense with R_w2c / t_w2c as leaves) on the oracle state `st`, for the cotangent `vp`.  The model detaches
    the normal channel from the pose (projection.jl:227-229)."""
    import f64_model as fm
    tt = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=fm.DT)  # noqa: E731
    Rl = tt(cam.R).requires_grad_(True)  # row-major R[r][c]
    tl = tt(cam.t).requires_grad_(True)
    img = fm.render_dense(tt(means), tt(shs), tt(np.asarray(opac).reshape(-1)), tt(scales), tt(rots), cam, deg,
                          np.asarray(bg, np.float32), mode, st.values_sorted, st.ranges, st.radii, R_w2c=Rl, t_w2c=tl)
    (img * torch.tensor(np.asarray(vp), dtype=fm.DT)).sum().backward()
    return Rl.grad.numpy().T.reshape(-1).copy(), tl.grad.numpy().reshape(-1).copy()


def pose_distances(hip, oracle, f64=None):
    """(rel-L2(HIP, oracle), rel-L2(oracle, f64), rel-L2(HIP, f64)) of one pose-gradient vector (vR or vt); the float64 legs are
    None without `f64`."""
    h, o = np.asarray(hip, np.float64).reshape(-1), np.asarray(oracle, np.float64).reshape(-1)
    if f64 is None:
        return rel_l2(h, o), None, None
    f = np.asarray(f64, np.float64).reshape(-1)
    return rel_l2(h, o), rel_l2(o, f), rel_l2(h, f)


def pose_ok(e_ho, e_o=None, e_h=None):
    """The pose-gradient criterion.  A pose gradient is ONE sum over every Gaussian of the view — signed terms that largely
    cancel — so its relative error is the per-Gaussian errors amplified by Σ|terms| / |Σ terms|: HIP meets 1e-4 against the
    oracle, or (where the float64 model was evaluated) meets 1e-4 against float64 or is no further from float64 than the fp32
    oracle is (x 4 + 1e-4)."""
    return e_ho <= 1e-4 or (e_h is not None and (e_h <= 1e-4 or e_h <= 4.0 * e_o + 1e-4))
