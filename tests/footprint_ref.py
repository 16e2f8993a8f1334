"""numpy fp32 restatements around the per-instance footprint masks (csrc/tile_mask.h instance_row_mask), shared by
tests/test_footprint_mask_math.py (no GPU) and tests/test_gpu_footprint_masks.py.

  * kernel_sigma:     the compositing kernels' sigma (composite.hip sigma_x / sigma_of), operation by operation;
  * threshold_bits:   X of a Gaussian (tile_mask.h blend_threshold_bits): bits(S) + 1, S the largest sigma that passes
                      fl(min(0.99, o · fl(exp(-sigma)))) >= fl(1/255) with a correctly rounded exp, 0 when none does;
  * active_pixels:    the kernels' blend test bits(sigma) < X on the 16 x 16 pixel centres of a tile;
  * mask_words:       the mask word as instance_row_mask derives it (clamped-vertex minimum of sigma per row and half, sign bits);
  * check_masks:      conservativeness and row counts of mask words against active_pixels.

Every array is float32 and every operation rounds once: a product of two floats is exact in float64, so a fused multiply-add
is float32(float64(x) · float64(y) + float64(z)).  (That sum rounds twice, which can differ from the hardware's single rounding
in the last bit: one ulp of sigma, against a mask slack of 2e-3 + 4e-6 of sigma's largest term.)
Instances are vectors of length n; pixel arrays are (n, 16, 16) = (instance, row, column)."""
import numpy as np

F = np.float32


def fma(x, y, z):
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(F)


def kernel_sigma(mx, my, a, b, c, X0, Y0):
    """sigma at the 16 x 16 pixel centres of the tile at (X0, Y0): dx = mx - px, dy = my - py,
    sigma = fma(b·dx, dy, fma(c/2, dy·dy, (a/2)·(dx·dx)))."""
    cols = np.arange(16, dtype=np.int64)
    dx = (mx[:, None] - (X0[:, None] + cols).astype(F))[:, None, :]   # (n, 1, 16)
    dy = (my[:, None] - (Y0[:, None] + cols).astype(F))[:, :, None]   # (n, 16, 1)
    ha, hc, b = (F(0.5) * a)[:, None, None], (F(0.5) * c)[:, None, None], b[:, None, None]
    with np.errstate(over="ignore", invalid="ignore"):
        hxx, bdx = ha * (dx * dx), b * dx
        return fma(np.broadcast_to(bdx, (len(mx), 16, 16)), np.broadcast_to(dy, (len(mx), 16, 16)), fma(hc, dy * dy, hxx))


def threshold_bits(o):
    """X = bits(S) + 1 per opacity (0: not even sigma = +0 passes).  The test is monotone in sigma: bisection over bit patterns."""
    o = np.asarray(o, F)

    def passes(bits):
        g = np.exp(-bits.astype(np.uint32).view(F).astype(np.float64)).astype(F)
        with np.errstate(invalid="ignore"):
            return np.minimum(F(0.99), o * g) >= F(1.0) / F(255.0)

    lo = np.zeros(o.shape, np.int64)                      # passes (where anything does)
    hi = np.full(o.shape, int(np.array(8.0, F).view(np.uint32)), np.int64)  # exp(-8) < 1/255: fails for every opacity <= 1
    any_pass = passes(lo)
    for _ in range(32):
        mid = (lo + hi) >> 1
        p = passes(mid)
        lo, hi = np.where(p, mid, lo), np.where(p, hi, mid)
    return np.where(any_pass, lo + 1, 0).astype(np.uint32)


def active_pixels(mx, my, a, b, c, X, X0, Y0):
    """(n, 16, 16) bool: bits(sigma) < X (a negative sigma has the sign bit set and never passes)."""
    return kernel_sigma(mx, my, a, b, c, X0, Y0).view(np.uint32) < X[:, None, None]


def mask_words(mx, my, a, b, c, X, X0, Y0):
    """The 20-bit word of csrc/tile_mask.h instance_row_mask, row by row as the device code has it."""
    n = len(mx)
    ha, hc = F(0.5) * a, F(0.5) * c
    l_hi, l_lo = mx - X0.astype(F), mx - (X0 + 7).astype(F)
    r_hi, r_lo = mx - (X0 + 8).astype(F), mx - (X0 + 15).astype(F)
    dy0 = my - Y0.astype(F)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        xm, ym = np.maximum(np.abs(l_hi), np.abs(r_lo)), np.maximum(np.abs(dy0), np.abs(dy0 - F(15.0)))
        M = ha * (xm * xm) + np.abs(b) * (xm * ym) + hc * (ym * ym)
        S = (X - np.uint32(1)).astype(np.uint32).view(F)
        ts = S + F(2e-3) + F(4e-6) * M
        nboa = -b * (F(1.0) / a)
        ml, mr = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        for r in range(15, -1, -1):
            dy = dy0 - F(r)
            v, bdy = nboa * dy, b * dy
            k = fma(dy, hc * dy, -ts)
            xl = np.maximum(np.minimum(v, l_hi), l_lo)    # med3(v, lo, hi), lo <= hi
            xr = np.maximum(np.minimum(v, r_hi), r_lo)
            sl, sr = fma(xl, fma(ha, xl, bdy), k), fma(xr, fma(ha, xr, bdy), k)
            ml = (ml << np.uint32(1)) | (sl.view(np.uint32) >> np.uint32(31))
            mr = (mr << np.uint32(1)) | (sr.view(np.uint32) >> np.uint32(31))
    m = (ml | mr).astype(np.uint32)
    for bit, half, rows in ((16, ml, 0xFF), (17, mr, 0xFF), (18, ml, 0xFF00), (19, mr, 0xFF00)):
        m |= ((half & np.uint32(rows)) != 0).astype(np.uint32) << np.uint32(bit)
    with np.errstate(invalid="ignore"):
        m = np.where(a > 0, m, np.uint32(0xFFFFF))
    return np.where(X == 0, np.uint32(0), m).astype(np.uint32)


def check_masks(words, act):
    """Counts for mask words (n,) against the active pixels (n, 16, 16):
    (rows active but not flagged, quadrants active but not flagged, active rows, flagged rows, active quadrants, flagged quadrants)."""
    words = np.asarray(words).astype(np.int64)
    rows_act = act.any(2)                                                     # (n, 16)
    rows_flag = ((words[:, None] >> np.arange(16)) & 1).astype(bool)
    quad_act = np.stack([act[:, 8 * qy:8 * qy + 8, 8 * qx:8 * qx + 8].any((1, 2)) for qy in (0, 1) for qx in (0, 1)], 1)
    quad_flag = ((words[:, None] >> (16 + np.arange(4))) & 1).astype(bool)   # bit 16 + 2 qy + qx
    return (int((rows_act & ~rows_flag).sum()), int((quad_act & ~quad_flag).sum()), int(rows_act.sum()), int(rows_flag.sum()),
            int(quad_act.sum()), int(quad_flag.sum()))


def hostile_instances(n, seed):
    """Seeded instances that stress the mask: axis ratios up to 100 : 1 at every angle (a sixth snapped to multiples of 45 degrees),
    axis lengths (standard deviations) 0.3 .. 300 px, a fifth of the opacities within 0.02 of 1/255 (below it too), tiles anywhere
    on a 1920 x 1088 grid, centres up to 3 standard deviations outside the tile.  Returns float32 mx, my, a, b, c, opacity and int64 X0, Y0."""
    rng = np.random.default_rng(seed)
    ratio = np.exp(rng.uniform(0.0, np.log(100.0), n))
    minor = np.exp(rng.uniform(np.log(0.3), np.log(300.0), n))
    small = rng.random(n) < 0.5                          # half of them: a thin minor axis, so that the ratio is not clipped away
    minor[small] = np.exp(rng.uniform(np.log(0.3), np.log(3.0), int(small.sum())))
    major = np.minimum(minor * ratio, 300.0)
    th = rng.uniform(0.0, np.pi, n)
    snap = rng.random(n) < 1.0 / 6.0
    th[snap] = rng.integers(0, 4, int(snap.sum())) * (np.pi / 4)
    cs, sn = np.cos(th), np.sin(th)
    cxx = cs * cs * major ** 2 + sn * sn * minor ** 2
    cyy = sn * sn * major ** 2 + cs * cs * minor ** 2
    cxy = cs * sn * (major ** 2 - minor ** 2)
    det = cxx * cyy - cxy * cxy
    a, b, c = cyy / det, -cxy / det, cxx / det           # the conic: sigma = (a dx² + c dy²)/2 + b dx dy
    X0, Y0 = 16 * rng.integers(0, 120, n), 16 * rng.integers(0, 68, n)
    mx = X0 + 7.5 + rng.uniform(-1.0, 1.0, n) * (8.0 + 3.0 * np.sqrt(cxx))
    my = Y0 + 7.5 + rng.uniform(-1.0, 1.0, n) * (8.0 + 3.0 * np.sqrt(cyy))
    o = rng.uniform(0.004, 1.0, n)
    edge = rng.random(n) < 0.2
    o[edge] = np.maximum(1.0 / 255.0 + rng.uniform(-0.02, 0.02, int(edge.sum())), 1e-4)
    return tuple(v.astype(F) for v in (mx, my, a, b, c, o)) + (X0.astype(np.int64), Y0.astype(np.int64))
