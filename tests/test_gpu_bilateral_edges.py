"""Bilateral grid on the MI355X, entry by entry: every element of the sliced colours, ∇image, ∇grid and the TV gradient
against the float64 restatement (bilateral_ref.py) under a DERIVED bound

    |got - ref| <= c · 2^-24 · A

A: the sum of the absolute values of the element's float64 terms (bilateral_ref's *_terms); c: the number of rounded
fp32 operations on the longest path to the element, counted from csrc/bilateral.hip (the constants below).  An element
with A == 0 (a grid entry no pixel reaches, a level no planted pixel touches, the TV gradient of identity grids) must be
exactly 0.  Nothing here is a tolerance taken from the kernels' own output.  The shapes are the ones where the pullback's
structure can go wrong unseen by a tensor norm: a cell cut into several chunks (full, ragged, nearly empty), pixels on
cell boundaries, cells without a pixel, degenerate image sides, the largest gz, guidance landing on a level.

Every test prints its largest observed error / bound (pytest -s); DESIGN.md §11 records them."""
import functools

import numpy as np
import pytest
import torch

import bilateral_ref as br
from hip_helpers import dev
from test_gpu_poisoned_buffers import _same_whatever_the_fill, _scratch_bytes, empty

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # the unit roundoff of fp32, round to nearest

# ---- the constants c: rounded fp32 operations on the longest path to an element, read off csrc/bilateral.hip ----------
# slice_fwd_kernel, one term G·wt·s4 of out[d]: three lerps, each (1 - f), a product and an add (9); ·s4 (1); the four adds
# of acc (4): 14, + 2 for the second-order terms.
C_FWD = 16
# slice_bwd_kernel, one term v·wt·d of gs[si]: wt = ((1-fx)·(1-fy))·(1-fz) is 5 roundings; v·wt, ·d (2); 24 terms, so 24
# adds; the add of C2G·gzs that forms the output (1): 32, + 2.
C_IMG_GS = 34
# slice_bwd_kernel, one term dwdz·v·gb of gzs: dwdz = ((1-fx)·(1-fy))·(±1)·dz is 4 roundings (the sign is exact); gb = s·d
# (1); dwdz·v, ·gb (2); 96 terms, so 96 adds; C2G·gzs and the add that forms the output (2): 105, + 2.
C_IMG_GZ = 107
# ∇grid, an entry of n_e terms: 1-fx, 1-fy, their product, 1-fz, ·wl, s·d, w·a and the add form a term (8); then at most
# n_e - 1 additions in any order (registers, wave halving, LDS slots, the four waves, the chunks and cells of
# slice_bwd_sum_kernel; an addition of an exact zero rounds nothing): n_e + 7, + 5 for the second-order terms.


def c_grid(n_e):
    return n_e + 12


# tv_slab_kernel, one entry: a difference (1); the two differences of an axis combined (1); r = 2/(norm·12n), a product and
# a quotient (2); ·r (1); the two adds over the axes (2); ·weight (1): 8, + 2.
C_TV = 10


def c_tv_loss(n, G):
    """tv_slab_kernel -> block_sum -> tv_final_kernel, all terms >= 0 so A is the loss itself: d and d·d (3: the rounding of
    d counts twice in the square); a thread's ceil(G/256) adds; wave_sum (6) and block_sum's three adds; in
    tv_final_kernel a thread's ceil(12n/256) adds, wave_sum (6), three adds; /norm, the two adds over the axes, /12n,
    ·weight (5); + 2."""
    return 3 + -(-G // 256) + 9 + -(-12 * n // 256) + 9 + 5 + 2


def held(got, ref, bound, what):
    """Every element within its bound (NaN fails; a zero bound asks for equality).  -> the largest error / bound."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == bound.shape, what
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        worst = np.nanmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside their bound, first at {i}: got {got[i]!r}, "
                             f"float64 {ref[i]!r}, bound {bound[i]:.3e}; largest error / bound {worst:.4g}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def report(what, **ratios):
    print(f"\n[bilateral edges] {what}: largest error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


# ---- the shapes: W, H, C, (gx, gy, gz), the chunks a cell is cut into, pixels that also get a non-finite value --------
CASES = {
    # one cell of 1056 pixels in 2 chunks of 528: the third pixel slot of a thread is partly filled
    "a-33x32-1.1.1": (33, 32, 3, (1, 1, 1), 2, [(31, 16)]),
    # 2 chunks of exactly 1024: every lane and slot full
    "b-64x32-1.1.1": (64, 32, 5, (1, 1, 1), 2, [(15, 63), (16, 0)]),
    "b-40x30-1.1.2": (40, 30, 8, (1, 1, 2), 2, [(14, 39), (15, 0)]),
    # cell (0,0) 69 x 69 in 5 chunks; cell (1,0) 1 x 69 in chunks of 14 and a last of 13; cell (1,1) one pixel and four empty
    # chunks; the clamped last column and row
    "c-70x70-2.2.3": (70, 70, 5, (2, 2, 3), 5, [(68, 68), (35, 69), (69, 35), (13, 69), (14, 69)]),
    # a ragged split over two chunks
    "d-65x33-3.2.4": (65, 33, 8, (3, 2, 4), 2, [(31, 31), (31, 32), (32, 64), (16, 63)]),
    # (W-1)/(gx-1) = 4 and (H-1)/(gy-1) = 7: columns 0, 4, .., 28 and rows 0, 7, 14, 21 sit on cell boundaries
    "e-29x22-8.4.5": (29, 22, 3, (8, 4, 5), 1, [(7, 4), (14, 8), (7, 5), (6, 4)]),
    # more cells than pixels
    "f-5x3-8.6.4": (5, 3, 3, (8, 6, 4), 1, []),
    "f-2x2-4.4.2": (2, 2, 5, (4, 4, 2), 1, []),
    # degenerate image sides
    "g-1x1-3.3.2": (1, 1, 3, (3, 3, 2), 1, []),
    "g-1x7-3.3.2": (1, 7, 8, (3, 3, 2), 1, []),
    "g-7x1-3.3.2": (7, 1, 5, (3, 3, 2), 1, []),
    # the largest gz (the pullback's full LDS), and grid sides of 1
    "h-17x9-2.2.64": (17, 9, 3, (2, 2, 64), 1, [(4, 8)]),
    "h-17x9-5.4.1": (17, 9, 5, (5, 4, 1), 1, [(4, 8)]),
    "h-17x9-1.4.3": (17, 9, 8, (1, 4, 3), 1, [(4, 8)]),
}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """image and grid of a case (shared by every test of it; never written)."""
    W, H, Cc, (gx, gy, gz), _, extra = CASES[name]
    r = np.random.default_rng(sorted(CASES).index(name) + 100)
    img = r.uniform(-0.5, 1.5, (H, W, Cc)).astype(np.float32)
    grid = (br.identity_grids(1, gx, gy, gz)[0] + r.normal(0, 0.3, (12, gz, gy, gx))).astype(np.float32)
    if W * H >= 4:   # non-finite pixels on the border rows and columns, and on the case's own boundaries
        img[0, W - 1, 1] = np.nan
        img[H - 1, 0, 2] = np.inf
        for k, (h, w) in enumerate(extra[::2]):
            img[h, w, k % 3] = (np.nan, -np.inf)[k % 2]
    return img, grid


@functools.lru_cache(maxsize=None)
def _cotangent(name, sign):
    W, H, Cc, _, _, extra = CASES[name]
    r = np.random.default_rng(sorted(CASES).index(name) + (200 if sign == "positive" else 300))
    # all positive: A ~ |sum|, the bound is relative to the entry itself; signed: cancellation inside an entry
    vout = (r.uniform(0.5, 1.5, (H, W, Cc)) if sign == "positive" else r.normal(size=(H, W, Cc))).astype(np.float32)
    if W * H >= 4:
        vout[H - 1, W - 1, 0] = np.nan
        vout[0, 0, 2] = -np.inf
        for k, (h, w) in enumerate(extra[1::2]):
            vout[h, w, (k + 1) % 3] = (np.inf, np.nan)[k % 2]
    return vout


@functools.lru_cache(maxsize=None)
def _forward_ref(name):
    return br.slice_forward_terms(*_inputs(name))


@functools.lru_cache(maxsize=None)
def _backward_ref(name, sign):
    return br.slice_backward_terms(*_inputs(name), _cotangent(name, sign))


def check_forward(out, img, acc, A):
    r = held(out[..., :3], np.where(np.isfinite(acc), acc, 0.5), C_FWD * U * A, "sliced colours")
    assert np.array_equal(out[..., 3:].view(np.uint32), img[..., 3:].view(np.uint32))   # bit-exact copy, NaN/Inf included
    return r


def check_backward(vi, vg, vout, t):
    """∇image and ∇grid against slice_backward_terms' dict; -> their largest error / bound."""
    c2g = np.array(br.C2G, np.float64)
    bound = U * (C_IMG_GS * t["gs_abs"] + C_IMG_GZ * c2g * t["gz_abs"][..., None])
    ratios, failed = [], []
    for what, got, ref, b in (("∇image", vi[..., :3], t["vimage"][..., :3], bound),
                              ("∇grid", vg, t["vgrid"], c_grid(t["vgrid_count"]) * U * t["vgrid_abs"])):
        try:      # both are judged before either is reported
            ratios.append(held(got, ref, b, what))
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    assert np.array_equal(vi[..., 3:].view(np.uint32), vout[..., 3:].view(np.uint32))
    return tuple(ratios)


def _chunks(pkg, W, H, size):
    gx, gy, gz = size
    return int(pkg._lib.load().gsr_bilateral_scratch_bytes(W, H, gx, gy, gz)) // (gx * gy * gz * 48 * 4)


@pytest.fixture(scope="module")
def bg(pkg):
    return pkg.bilateral_grid


def test_the_shapes_are_what_they_are_here_for(pkg):
    """From the reference's coordinates and the library's own chunk count (no GPU work): the multi-chunk shapes are
    multi-chunk, shape e has pixels on cell boundaries, shape f cells without a pixel, every C is used."""
    for name, (W, H, Cc, size, nchunk, _) in CASES.items():
        assert _chunks(pkg, W, H, size) == nchunk, name
    assert {c[2] for c in CASES.values()} == {3, 5, 8}
    c = br.coords(_inputs("e-29x22-8.4.5")[0], 8, 4, 5)
    assert [w for w in range(29) if c["fx"][0, w] == 0] == list(range(0, 29, 4))
    assert [h for h in range(22) if c["fy"][h, 0] == 0] == [0, 7, 14, 21]
    assert ((c["fx"] == 0) & (c["x"][0] > 0) & (c["x"][0] < 7)).sum() == 6 * 22    # interior boundaries, fx == 0
    c = br.coords(_inputs("c-70x70-2.2.3")[0], 2, 2, 3)
    assert (c["x"][0][0] == 1).sum() == 1 and (c["y"][0][:, 0] == 1).sum() == 1     # cells 69 x 69, 1 x 69, 69 x 1, 1 x 1
    for name in ("f-5x3-8.6.4", "f-2x2-4.4.2"):
        t = _backward_ref(name, "signed")
        assert (t["vgrid_count"] == 0).any() and (t["vgrid_count"] > 0).any(), name


@pytest.mark.parametrize("name", CASES)
def test_sliced_colours_per_pixel(bg, name):
    img, grid = _inputs(name)
    out = bg.slice_forward(dev(img), dev(grid))
    torch.cuda.synchronize()
    report(f"forward {name}", out=check_forward(out.cpu().numpy(), img, *_forward_ref(name)))


@pytest.mark.parametrize("sign", ["positive", "signed"])
@pytest.mark.parametrize("name", CASES)
def test_pullback_per_pixel_and_per_grid_entry(bg, name, sign):
    img, grid = _inputs(name)
    vout = _cotangent(name, sign)
    ti, tg, tv = dev(img), dev(grid), dev(vout)
    vimg, vgrid = bg.slice_backward(ti, tg, tv)
    tv_in = tv.clone()
    vimg2, vgrid2 = bg.slice_backward(ti, tg, tv_in, vimage=tv_in)    # in place on the cotangent: the same bits
    torch.cuda.synchronize()
    ri, rg = check_backward(vimg.cpu().numpy(), vgrid.cpu().numpy(), vout, _backward_ref(name, sign))
    report(f"pullback {name} {sign}", vimage=ri, vgrid=rg)
    assert vimg2.data_ptr() == tv_in.data_ptr()
    assert torch.equal(vimg.view(torch.int32), vimg2.view(torch.int32)) and torch.equal(vgrid.view(torch.int32), vgrid2.view(torch.int32))


@pytest.mark.parametrize("gz", [3, 5, 9])
def test_guidance_landing_on_a_level(bg, gz):
    """Grey pixels (v, v, v), v = k/(gz-1), land exactly on interior level k; (0,0,0) and (2,2,2) saturate.  No guidance
    term in ∇image there (its bound has none: gz_abs is 0), and the full weight on one level of ∇grid.  In the second
    image EVERY pixel sits on level 1, so every other level of ∇grid has no term and must be exactly 0."""
    W, H, Cc, size = 24, 20, 3, (3, 2, gz)
    r = np.random.default_rng(gz)
    img = r.uniform(-0.5, 1.5, (H, W, Cc)).astype(np.float32)
    classes = [(k, np.float32(k) / np.float32(gz - 1)) for k in range(1, gz - 1)] + [(0, np.float32(0)), (gz - 1, np.float32(2))]
    planted = []
    for j, (level, v) in enumerate(classes):     # four pixels of each class, border rows and columns among them
        for h, w in ((j, 2 * j + 1), (H - 1 - j, W - 2 - j), (H // 2, (5 * j + 3) % W), (0, W - 1 - j)):
            img[h, w] = v
            planted.append((level, h, w))
    grid = (br.identity_grids(1, *size)[0] + r.normal(0, 0.3, (12, gz, 2, 3))).astype(np.float32)
    vout = r.normal(size=(H, W, Cc)).astype(np.float32)
    c = br.coords(img, *size)
    t = br.slice_backward_terms(img, grid, vout)
    assert len({(h, w) for _, h, w in planted}) == 4 * len(classes)
    for level, h, w in planted:    # each class is present, decided by the reference's fp32 coordinates
        assert not c["z_interior"][h, w] and c["fz"][h, w] == 0 and c["z"][0][h, w] == level, (level, h, w)
        assert t["gz_abs"][h, w] == 0
    assert c["z_interior"].sum() > W * H // 4
    vimg, vgrid = bg.slice_backward(dev(img), dev(grid), dev(vout))
    torch.cuda.synchronize()
    ri, rg = check_backward(vimg.cpu().numpy(), vgrid.cpu().numpy(), vout, t)
    # every pixel on level 1
    img1 = np.full((H, W, Cc), np.float32(1) / np.float32(gz - 1), np.float32)
    t1 = br.slice_backward_terms(img1, grid, vout)
    others = [l for l in range(gz) if l != 1]
    assert not t1["vgrid_count"][:, others].any() and t1["vgrid_count"][:, 1].all() and not t1["gz_abs"].any()
    vimg1, vgrid1 = bg.slice_backward(dev(img1), dev(grid), dev(vout))
    torch.cuda.synchronize()
    ri1, rg1 = check_backward(vimg1.cpu().numpy(), vgrid1.cpu().numpy(), vout, t1)
    assert not vgrid1[:, others].any().item()
    report(f"guidance on a level gz={gz}", vimage=max(ri, ri1), vgrid=max(rg, rg1))


# ---- TV and the fused tail ---------------------------------------------------------------------------------------------
TV_SIZES = [(1, 1, 1), (1, 4, 3), (5, 1, 1), (7, 3, 1), (257, 1, 1), (5, 4, 3)]
TV_N = [1, 22]    # 22 x 12 = 264 slabs: more than tv_final_kernel's 256 threads


def _grids(n, size, seed, sigma=0.1):
    gx, gy, gz = size
    r = np.random.default_rng(seed)
    return (br.identity_grids(n, gx, gy, gz) + r.normal(0, sigma, (n, 12, gz, gy, gx))).astype(np.float32)


@pytest.mark.parametrize("n", TV_N)
@pytest.mark.parametrize("size", TV_SIZES)
def test_tv_loss_and_gradient_per_entry(bg, size, n):
    weight = 10.0
    grids = _grids(n, size, 7 * n + sum(size))
    loss, grad = bg.tv(dev(grids), weight=weight, grad=True)
    loss_only = bg.tv(dev(grids), weight=weight)
    iloss, igrad = bg.tv(dev(br.identity_grids(n, *size)), weight=weight, grad=True)
    torch.cuda.synchronize()
    ref, A = br.tv_grad_terms(grids)
    rg = held(grad.cpu().numpy(), weight * ref, C_TV * U * weight * A, "TV gradient")
    want = weight * br.tv_loss(grids)
    rl = held(np.float64(loss.item()), want, c_tv_loss(n, size[0] * size[1] * size[2]) * U * want, "TV loss")
    assert loss_only.item() == loss.item()
    if min(size) == max(size) == 1:
        assert want == 0.0 and not A.any()     # a single cell has no variation
    # identity grids: exactly 0, loss and every entry (+0 or -0)
    assert iloss.item() == 0.0 and not igrad.any().item()
    report(f"TV {size} n={n}", gradient=rg, loss=rl)


@pytest.mark.parametrize("n", TV_N)
@pytest.mark.parametrize("size", TV_SIZES)
def test_fused_tail_equals_the_unfused_composition_bit_for_bit(pkg, bg, size, n):
    gx, gy, gz = size
    for view in sorted({0, n - 1}):
        r = np.random.default_rng(31 * n + view + sum(size))
        B = bg.BilateralGrid(n, size, lr=2e-3, device="cuda:0")
        B.grids.copy_(dev(_grids(n, size, 5 * n + view, sigma=0.05)))
        B.scheduler = lambda s: np.float32(2e-3 * (1.0 - 0.1 * s))
        theta = B.grids.clone()
        ref_opt = pkg.optim.Adam(theta, 2e-3, eps=1e-15)
        for step in range(1, 4):
            vgrid = dev(r.normal(0, 1e-2, (12, gz, gy, gx)).astype(np.float32))
            B.vgrid.copy_(vgrid)
            B.vgrid_view = view
            tv_term = B.step(view, step, tv_weight=10.0)
            # unfused: gsr_bilateral_tv (gradient) -> add the view's ∇grid -> gsr_adam_step
            ref_opt.lr = float(np.float32(2e-3 * (1.0 - 0.1 * step)))
            loss, g = bg.tv(theta, weight=10.0, grad=True)
            g[view] += vgrid
            ref_opt.step(theta, g)
            torch.cuda.synchronize()
            assert tv_term.item() == loss.item(), (view, step)
            assert torch.equal(B.grids.view(torch.int32), theta.view(torch.int32)), (view, step)
            assert torch.equal(B.optimizer.mu.view(torch.int32), ref_opt.mu.view(torch.int32)), (view, step)
            assert torch.equal(B.optimizer.nu.view(torch.int32), ref_opt.nu.view(torch.int32)), (view, step)
            assert B.optimizer.current_step == ref_opt.current_step == step
        # identity grids: the TV gradient is zero, so only the sliced view moves
        I = bg.BilateralGrid(n, size, device="cuda:0")
        before = I.grids.clone()
        I.vgrid.copy_(dev(r.normal(0, 1e-2, (12, gz, gy, gx)).astype(np.float32)))
        I.vgrid_view = view
        term = I.step(view, 1000)
        torch.cuda.synchronize()
        assert term.item() == 0.0
        others = [v for v in range(n) if v != view]
        assert torch.equal(I.grids[others].view(torch.int32), before[others].view(torch.int32))
        assert not torch.equal(I.grids[view], before[view])


# ---- poisoned buffers at a multi-chunk shape ---------------------------------------------------------------------------
def test_poisoned_outputs_and_scratch_at_the_multi_chunk_shape(pkg, bg):
    """Shape c (5 chunks per cell, four of them empty for the one-pixel cell): outputs and the caller-owned slice scratch
    pre-filled with 0xFF bytes, then 0x7F bytes, must give the clean run's bits; so must the in-place form and a second
    run on the scratch the first one left."""
    name = "c-70x70-2.2.3"
    W, H, Cc, (gx, gy, gz), _, _ = CASES[name]
    img, grid = _inputs(name)
    vout = _cotangent(name, "signed")
    ti, tg, tv = dev(img), dev(grid), dev(vout)
    nb = int(pkg._lib.load().gsr_bilateral_scratch_bytes(W, H, gx, gy, gz))

    def run(fill):
        out = bg.slice_forward(ti, tg, out=empty(H, W, Cc, fill=fill))
        scratch = {"slice": _scratch_bytes(nb, fill)}
        vimage, vgrid = bg.slice_backward(ti, tg, tv, vimage=empty(H, W, Cc, fill=fill), vgrid=empty(12, gz, gy, gx, fill=fill),
                                          scratch=scratch)
        vimage, vgrid = vimage.clone(), vgrid.clone()
        vo = tv.clone()      # in place, on the scratch the first run left
        _, vgrid_inplace = bg.slice_backward(ti, tg, vo, vimage=vo, vgrid=empty(12, gz, gy, gx, fill=fill), scratch=scratch)
        again, vgrid_again = bg.slice_backward(ti, tg, tv, vimage=empty(H, W, Cc, fill=fill),
                                               vgrid=empty(12, gz, gy, gx, fill=fill), scratch=scratch)
        torch.cuda.synchronize()
        return dict(out=out, vimage=vimage, vgrid=vgrid, inplace=vo, vgrid_inplace=vgrid_inplace, again=again,
                    vgrid_again=vgrid_again)

    clean = _same_whatever_the_fill(run)
    for a, b in (("vimage", "inplace"), ("vimage", "again"), ("vgrid", "vgrid_inplace"), ("vgrid", "vgrid_again")):
        assert torch.equal(clean[a].view(torch.int32), clean[b].view(torch.int32)), (a, b)
    check_forward(clean["out"].cpu().numpy(), img, *_forward_ref(name))
    check_backward(clean["vimage"].cpu().numpy(), clean["vgrid"].cpu().numpy(), vout, _backward_ref(name, "signed"))
