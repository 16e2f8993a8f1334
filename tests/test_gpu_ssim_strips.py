"""The strip geometry of ssim.hip: one wave owns 54 output columns (+ 5 halo lanes on each side) and walks down a strip of
rows, the vertical pass lives in a register ring.  What a rewrite of that shape can break: image sizes that are not multiples
of anything (a 1-pixel image, a last strip with a single column or row, sizes just below / at / above a strip's width and
height), the bit-exact twin's accumulation order, the per-wave partial sums of the loss and the zero fill of channels >= 3.

Criteria are those of tests/test_gpu_parity.py (test_ssim_vs_oracle: bit for bit;
test_default_ssim_arithmetic_vs_oracle_at_fp32_tolerance: 1e-5 on the map, 2e-5 relative L2 on the derivative maps and the
pullback; test_loss_head_vs_oracle) and of tests/test_gpu_poisoned_buffers.py (poisoned outputs and scratch equal the clean
run bit for bit)."""
import contextlib
import os

import numpy as np
import pytest
import torch

from hip_helpers import dev, frac_bad, rel_l2
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu

# (W, H): widths and heights of 1, 5, 11, 53, 54, 55, 64, 65.  The strip height is chosen per launch (ssim_strip_h): 8 rows for
# images with fewer waves than the GPU has SIMDs, as all of these are, so heights 7, 8, 9 sit just below / at / above it; the
# heights around 16 and 32 are those of the fixed-height builds of the knob series.  130 x 70 is wider than two strips and
# taller than two strips of any of these heights.
SIZES = [(1, 1), (5, 1), (1, 5), (11, 11), (53, 17), (54, 31), (55, 33), (64, 16), (65, 15), (130, 70),
         (17, 53), (31, 54), (33, 55), (16, 64), (15, 65), (9, 32), (12, 7), (20, 8), (7, 9)]
PLANES = [(2, 3), (1, 1)]
WORDS = {"nan": -1, "big": 0x7F7F7F7F}  # int32 views of 0xFFFFFFFF and 0x7F7F7F7F


def _inputs(B, CH, H, W, seed):
    rng = np.random.default_rng(seed)
    shape = (B, CH, H, W)
    return (rng.uniform(size=shape).astype(np.float32), rng.uniform(size=shape).astype(np.float32),
            rng.standard_normal(shape).astype(np.float32))


@pytest.mark.parametrize("planes", PLANES)
@pytest.mark.parametrize("size", SIZES)
def test_exact_build_is_the_oracle_bit_for_bit(pkg, orc, size, planes):
    (W, H), (B, CH) = size, planes
    x, y, dl = _inputs(B, CH, H, W, 1000 * W + H)
    m, d0, d1, d2 = orc.ssim_forward(x, y, train=True)
    g = orc.ssim_backward(x, y, dl, d0, d1, d2)
    F = pkg.fused_ssim
    with F.exact_arithmetic():
        hm, h0, h1, h2 = F._fused_ssim(dev(x), dev(y), train=True)
        hg = F.fused_ssim_bwd(dev(x), dev(y), dev(dl), h0, h1, h2)
        torch.cuda.synchronize()
    for name, a, b in (("map", hm, m), ("d0", h0, d0), ("d1", h1, d1), ("d2", h2, d2), ("pullback", hg, g)):
        a = a.cpu().numpy()
        print(f"{W}x{H} {planes} {name}: words that differ {(a.view(np.int32) != b.view(np.int32)).sum()} of {a.size}")
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("planes", PLANES)
@pytest.mark.parametrize("size", SIZES)
def test_default_build_at_fp32_tolerance(pkg, orc, size, planes):
    (W, H), (B, CH) = size, planes
    x, y, dl = _inputs(B, CH, H, W, 1000 * W + H)
    m, d0, d1, d2 = orc.ssim_forward(x, y, train=True)
    g = orc.ssim_backward(x, y, dl, d0, d1, d2)
    F = pkg.fused_ssim
    hm, h0, h1, h2 = F._fused_ssim(dev(x), dev(y), train=True)
    hg = F.fused_ssim_bwd(dev(x), dev(y), dev(dl), h0, h1, h2).cpu().numpy()
    dm = np.abs(hm.cpu().numpy() - m)
    print(f"{W}x{H} {planes} ssim map max / mean |diff|:", dm.max(), dm.mean())
    assert dm.max() <= 1e-5 and dm.mean() <= 5e-7
    for a, b in ((h0, d0), (h1, d1), (h2, d2)):
        a = a.cpu().numpy()
        print("   derivative map rel-L2:", rel_l2(a, b), "frac bad:", frac_bad(a, b, 1e-4, 1e-5 * float(np.abs(b).max())))
        assert rel_l2(a, b) <= 2e-5
        assert frac_bad(a, b, 1e-4, 1e-5 * float(np.abs(b).max())) <= 1e-3
    print("   pullback rel-L2:", rel_l2(hg, g))
    assert rel_l2(hg, g) <= 2e-5
    assert frac_bad(hg, g, 1e-4, 1e-5 * float(np.abs(g).max())) <= 1e-3


# ---- poisoned outputs and scratch ----
@contextlib.contextmanager
def debug_fill(fill):
    """GSR_DEBUG_FILL for the handles created inside the block: the library fills its own allocations (d0..d2 and the
    partial pairs of the loss head among them) with the word."""
    old = os.environ.pop("GSR_DEBUG_FILL", None)
    if fill:
        os.environ["GSR_DEBUG_FILL"] = fill
    try:
        yield
    finally:
        os.environ.pop("GSR_DEBUG_FILL", None)
        if old is not None:
            os.environ["GSR_DEBUG_FILL"] = old


def empty(*shape, fill):
    t = torch.empty(*shape, device="cuda", dtype=torch.float32)
    if fill is None:
        t.zero_()
    else:
        t.view(torch.int32).fill_(WORDS[fill])
    return t


def same_bits(a, b, what):
    assert a.shape == b.shape, what
    a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    if not torch.equal(a, b):
        d = (a != b).reshape(-1).nonzero()
        raise AssertionError(f"{what}: {d.numel()} of {a.numel()} words differ from the clean run (first at {int(d[0])})")


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("planes", PLANES)
@pytest.mark.parametrize("size", [(1, 1), (55, 33), (65, 15), (130, 70)])
def test_planar_outputs_are_written_whole(pkg, size, planes, exact):
    """Every element of the map, d0..d2 and the pullback is written, and nothing is read before it is: outputs that start as
    0xFFFFFFFF / 0x7F7F7F7F words end as the clean run's, bit for bit."""
    (W, H), (B, CH) = size, planes
    shape = (B, CH, H, W)
    x, y, dl = (dev(a) for a in _inputs(B, CH, H, W, 7 * W + H))
    lib = pkg._lib.load()
    res = {}
    with pkg.fused_ssim.exact_arithmetic(exact):
        for fill in (None, "nan", "big"):
            m, d0, d1, d2, gi = (empty(*shape, fill=fill) for _ in range(5))
            pkg._lib.check(lib.gsr_ssim_forward(W, H, CH, B, x.data_ptr(), y.data_ptr(), 0.01 ** 2, 0.03 ** 2, 1,
                                                m.data_ptr(), d0.data_ptr(), d1.data_ptr(), d2.data_ptr(), _stream()))
            pkg._lib.check(lib.gsr_ssim_backward(W, H, CH, B, x.data_ptr(), y.data_ptr(), dl.data_ptr(), d0.data_ptr(),
                                                 d1.data_ptr(), d2.data_ptr(), gi.data_ptr(), _stream()))
            torch.cuda.synchronize()
            res[fill] = dict(m=m, d0=d0, d1=d1, d2=d2, grad=gi)
    assert all(torch.isfinite(t).all() for t in res[None].values())
    for fill in ("nan", "big"):
        for k, v in res[None].items():
            same_bits(v, res[fill][k], f"{k} [{fill}]")


def _loss_call(pkg, rast, di, dt, fill):
    H, W, Cn = di.shape
    lo, vpx = empty(1, fill=fill), empty(H, W, Cn, fill=fill)
    L = pkg._lib
    L.check(L.load().gsr_loss_l1_ssim(rast._h, di.data_ptr(), dt.data_ptr(), 0.2, lo.data_ptr(), vpx.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return lo.clone(), vpx.clone()


# 1920 x 1080 is the benchmark's size (strips 39 rows high on 256 CUs: the last strip column and the last strip row are partly
# filled); 200 x 123 has a partly filled last strip in both directions for strips 54 wide and 8, 16 or 32 high; 55 x 17 has
# one column / one row in the last strips
@pytest.mark.parametrize("mode", ["rgb", "rgbd"])
@pytest.mark.parametrize("W,H", [(1920, 1080), (200, 123), (55, 17)])
def test_loss_head_reproducible_and_fast_against_exact(pkg, orc, W, H, mode):
    """Two consecutive calls give the same loss and cotangent bit for bit (per-wave partial pairs, fixed summation order);
    the default build against the exact twin within the tolerances of test_loss_head_vs_oracle; at the small sizes both
    builds against the oracle itself at those tolerances, the exact twin's loss to 1e-6.  (The exact twin's COTANGENT is the
    oracle's bit for bit only at sizes where λ·(1/(3WH)) rounds like λ/(3WH): the host passes the reciprocal of the pixel
    count to the kernel, the oracle divides, and at 200 x 123 the two constants differ by one ulp = 6e-8 relative.  That is the
    host's constant, as before the strips, not the kernels' arithmetic: the maps and the pullback themselves are compared bit
    for bit in test_exact_build_is_the_oracle_bit_for_bit, the loss head at the reference's size in test_loss_head_vs_oracle.)"""
    rng = np.random.default_rng(W + H)
    Cn = {"rgb": 3, "rgbd": 5}[mode]
    img = rng.uniform(0, 1, (H, W, Cn)).astype(np.float32)
    tgt = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    di, dt = dev(img), dev(tgt)
    out = {}
    for prec in ("fast", "exact"):
        rast = pkg.rasterizer.GaussianRasterizer(W, H, mode=mode, ssim_precision=prec)
        l1, v1 = pkg.fused_ssim.l1_ssim_loss(rast, di, dt)
        l1, v1 = l1.clone(), v1.clone()
        l2, v2 = pkg.fused_ssim.l1_ssim_loss(rast, di, dt)
        torch.cuda.synchronize()
        assert torch.equal(l1, l2) and torch.equal(v1, v2), prec
        assert not v1[:, :, 3:].view(torch.int32).any()
        out[prec] = (float(l1), v1.cpu().numpy())
        rast.close()
    (lf, vf), (le, ve) = out["fast"], out["exact"]
    print(f"{W}x{H} {mode}: loss fast {lf!r} exact {le!r}  cotangent rel-L2 {rel_l2(vf, ve)}")
    assert abs(lf - le) <= 1e-5 * max(1.0, abs(le))
    assert rel_l2(vf, ve) <= 1e-5
    if W * H <= 200 * 123:
        loss_o, vp_o = orc.loss_head(np.ascontiguousarray(img[:, :, :3]), tgt)
        print(f"   oracle loss {float(loss_o)!r}")
        print(f"   exact cotangent: words that differ from the oracle {(ve[:, :, :3].view(np.int32) != vp_o[:, :, :3].view(np.int32)).sum()}"
              f" of {vp_o[:, :, :3].size}, rel-L2 {rel_l2(ve[:, :, :3], vp_o[:, :, :3])}")
        assert abs(le - float(loss_o)) <= 1e-6
        assert rel_l2(ve[:, :, :3], vp_o[:, :, :3]) <= 1e-5
        assert abs(lf - float(loss_o)) <= 1e-5 * max(1.0, abs(float(loss_o)))
        assert rel_l2(vf[:, :, :3], vp_o[:, :, :3]) <= 1e-5


@pytest.mark.parametrize("prec", ["fast", "exact"])
@pytest.mark.parametrize("mode", ["rgb", "rgbd"])
@pytest.mark.parametrize("W,H", [(200, 123), (55, 17), (1, 1)])
def test_loss_head_on_poisoned_buffers(pkg, W, H, mode, prec):
    """Loss, cotangent (channels >= 3 exact zeros in :rgbd) and, through them, every element of the handle's d0..d2 and every
    partial pair: a pair or a derivative the kernels did not write would reach the loss or the cotangent as the fill word."""
    rng = np.random.default_rng(3 * W + H)
    Cn = {"rgb": 3, "rgbd": 5}[mode]
    di = dev(rng.uniform(0, 1, (H, W, Cn)).astype(np.float32))
    dt = dev(rng.uniform(0, 1, (3, H, W)).astype(np.float32))
    res = {}
    for fill in (None, "nan", "big"):
        with debug_fill(fill):
            rast = pkg.rasterizer.GaussianRasterizer(W, H, mode=mode, ssim_precision=prec)
            res[fill] = _loss_call(pkg, rast, di, dt, fill)
            rast.close()
    lo, vp = res[None]
    assert torch.isfinite(lo).all() and torch.isfinite(vp).all()
    assert not vp[:, :, 3:].view(torch.int32).any()
    for fill in ("nan", "big"):
        same_bits(lo, res[fill][0], f"loss [{fill}]")
        same_bits(vp, res[fill][1], f"vpixels [{fill}]")
