"""The geometry frames (scripts/render-views.jl:264-308 `depth_image` / `normal_image`; rasterizer.jl:163-198 `to_depth`;
gui/worker.jl:688-726 `handle_pick!`) restated for the tests: no product code.  Plain numpy, every fp32 operation as the
kernels write it (csrc/frames.hip), `np.fmax` / `np.fmin` where the kernels say fmaxf / fminf (a NaN operand loses).

- `keys` / `values`  : the monotone key of a float and back: unsigned key order == Julia's `sort` order (-0.0 < +0.0).
- `depth_stats`      : n, the two order statistics by `np.sort` on the keys, Statistics.jl's definition 7 with aleph through
                       `fractions.Fraction` rounded once to double (an fma), and the white level.
- `depth16`, `normal8`, `pick` : the encoders and the pick.
- `word_tie_set`     : fp32 inputs around rounding boundaries (k + 0.5) / 65535 of the 16-bit quantiser.
- `make_case`        : frames whose covered depths form the adversarial sets of the selection.

Layouts: a frame is (H, W, C); the depth picture (H, W) uint16; the normal picture (H, W, 3) uint8."""
import math
from fractions import Fraction

import numpy as np

f32 = np.float32
MIN_ALPHA = f32(1e-3)
TINY = f32(1e-6)
NEAR = f32(1e-2)
KINDS = ("random", "none", "one", "two", "equal", "lowbits", "clusters", "signed")


def keys(e):
    """uint32 keys of fp32 values: bits ^ (sign ? 0xFFFFFFFF : 0x80000000)."""
    u = np.ascontiguousarray(e, dtype=f32).view(np.uint32)
    return np.where(u >> np.uint32(31) != 0, ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def values(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k >> np.uint32(31) != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(f32)


def covered_mask(frame, min_alpha=MIN_ALPHA):
    with np.errstate(invalid="ignore"):
        return np.asarray(frame, f32)[..., 4] >= f32(min_alpha)


def expected_depth(frame, min_alpha=MIN_ALPHA):
    """e = depth / fmaxf(alpha, min_alpha), one fp32 division per pixel (every pixel: mask with `covered_mask`)."""
    frame = np.asarray(frame, f32)
    with np.errstate(all="ignore"):
        return (frame[..., 3] / np.fmax(frame[..., 4], f32(min_alpha))).astype(f32)


def rank(n, percentile):
    """Statistics.jl definition 7 for n >= 2 -> (j, gamma): p = percentile / 100, m = 1 - p, aleph = fma(n, p, m) — the exact
    rational n·p + m rounded once to double —, j = clamp(trunc(aleph), 1, n - 1), gamma = clamp(aleph - j, 0, 1)."""
    p = float(percentile) / 100.0
    m = 1.0 - p
    aleph = float(Fraction(n) * Fraction(p) + Fraction(m))
    j = min(max(math.trunc(aleph), 1), n - 1)
    return j, min(max(aleph - float(j), 0.0), 1.0)


def scale_from(a, b, gamma):
    """d = b - a in fp32; q = (double)a + gamma · (double)d, two double operations; fmaxf((float)q, 1e-6f)."""
    with np.errstate(all="ignore"):
        d = f32(f32(b) - f32(a))
        q = float(a) + gamma * float(d)
        return f32(np.fmax(f32(q), TINY))


def depth_stats(frame, percentile, min_alpha=MIN_ALPHA):
    """-> dict(scale fp32, n, a_bits, b_bits, j, gamma) as gsr_depth_scale defines them."""
    e = expected_depth(frame, min_alpha)[covered_mask(frame, min_alpha)]
    n = int(e.size)
    if n == 0:
        return dict(scale=f32(1), n=0, a_bits=0, b_bits=0, j=0, gamma=0.0)
    v = values(np.sort(keys(e)))
    if n == 1:
        j, gamma, a, b = 1, 0.0, v[0], v[0]
    else:
        j, gamma = rank(n, percentile)
        a, b = v[j - 1], v[j]
    bits = lambda x: int(np.asarray(x, f32).reshape(1).view(np.uint32)[0])  # noqa: E731
    return dict(scale=scale_from(a, b, gamma), n=n, a_bits=bits(a), b_bits=bits(b), j=j, gamma=gamma)


def stats_words(st):
    """The 16 bytes of stats_out as four uint32."""
    return np.array([int(np.asarray(st["scale"], f32).reshape(1).view(np.uint32)[0]), st["n"], st["a_bits"], st["b_bits"]], np.uint32)


def words(y):
    """floorf(y · 65535 + 0.5) of y already clamped to [0, 1], as uint16."""
    y = np.asarray(y, f32)
    return np.floor(y * f32(65535) + f32(0.5)).astype(np.uint16)


def depth16(frame, scale, expected=True, min_alpha=MIN_ALPHA, flip_rows=False):
    """(H, W) uint16: x = covered ? e : 0 (expected) or the raw depth; inv = 1 / scale; y = fminf(fmaxf(x · inv, 0), 1)."""
    frame = np.asarray(frame, f32)
    if expected:
        x = np.where(covered_mask(frame, min_alpha), expected_depth(frame, min_alpha), f32(0)).astype(f32)
    else:
        x = frame[..., 3]
    with np.errstate(all="ignore"):
        inv = f32(1) / f32(scale)
        y = np.fmin(np.fmax((x * inv).astype(f32), f32(0)), f32(1))
    pic = words(y)
    return np.ascontiguousarray(pic[::-1]) if flip_rows else pic


def levels8(x):
    """(uint8) floorf(fminf(fmaxf(x, 0), 1) · 255 + 0.5): eval_ref.levels with the kernels' NaN-losing min / max."""
    x = np.asarray(x, f32)
    return np.floor(np.fmin(np.fmax(x, f32(0)), f32(1)) * f32(255) + f32(0.5)).astype(np.uint8)


def normal8(frame, R_c2w=None, min_alpha=MIN_ALPHA):
    """(H, W, 3) uint8.  R_c2w: (3, 3) matrix M; row i of M·n = (M[i,0]·x + M[i,1]·y) + M[i,2]·z."""
    frame = np.asarray(frame, f32)
    with np.errstate(all="ignore"):
        den = np.fmax(frame[..., 4], f32(min_alpha))
        nx, ny, nz = (frame[..., 5] / den).astype(f32), (frame[..., 6] / den).astype(f32), (frame[..., 7] / den).astype(f32)
        length = np.sqrt((nx * nx + ny * ny) + nz * nz).astype(f32)
        degenerate = (length < TINY) | ~covered_mask(frame, min_alpha)
        l = np.fmax(length, TINY)
        nx, ny, nz = nx / l, ny / l, nz / l
        zero = f32(0)
        nx, ny, nz = np.where(degenerate, zero, nx), np.where(degenerate, zero, ny), np.where(degenerate, zero, nz)
        if R_c2w is not None:
            M = np.asarray(R_c2w, f32)
            rows = [(M[i, 0] * nx + M[i, 1] * ny) + M[i, 2] * nz for i in range(3)]
            nx, ny, nz = [np.where(degenerate, zero, r).astype(f32) for r in rows]
        return np.stack([levels8(c * f32(0.5) + f32(0.5)) for c in (nx, ny, nz)], axis=-1)


def pick_window(frame, px, py, hw):
    """The raw depths > 1e-2 of the clipped window around the 1-based pixel (None: the pixel lies outside the frame)."""
    frame = np.asarray(frame, f32)
    H, W = frame.shape[:2]
    if not (1 <= px <= W and 1 <= py <= H):
        return None
    win = frame[max(1, py - hw) - 1:min(H, py + hw), max(1, px - hw) - 1:min(W, px + hw), 3]
    return win[win > NEAR]


def pick_from_z(z, W, H, camera, px, py):
    """The three coordinates from the mean depth z, in fp32 as frames.hip orders them.  camera: focal, principal, R
    (world->camera, row-major (3, 3)), camera_center."""
    z = f32(z)
    fx, fy = f32(camera.focal[0]), f32(camera.focal[1])
    cx, cy = f32(camera.principal[0]) * f32(W), f32(camera.principal[1]) * f32(H)
    p0 = ((f32(px) - f32(0.5)) - cx) * z / fx
    p1 = ((f32(py) - f32(0.5)) - cy) * z / fy
    R = np.asarray(camera.R, f32)             # Rᵀ row i = column i of R
    cc = np.asarray(camera.camera_center, f32)
    return np.array([((R[0, i] * p0 + R[1, i] * p1) + R[2, i] * z) + cc[i] for i in range(3)], f32)


def word_tie_set(step=257):
    """For k = 0, step, 2·step, ... < 65535 (and 65534) the fp32 nearest to (k + 0.5) / 65535 and its 4 fp32 neighbours on each
    side -> (inputs, k of each)."""
    ks = sorted(set(list(range(0, 65535, step)) + [65534]))
    out, kk = [], []
    for k in ks:
        c = f32((k + 0.5) / 65535.0)
        lo = c
        for _ in range(4):
            lo = np.nextafter(lo, f32(-1))
        v = [lo]
        for _ in range(8):
            v.append(np.nextafter(v[-1], f32(2)))
        out.extend(v)
        kk.extend([k] * len(v))
    return np.asarray(out, f32), np.asarray(kk, np.int64)


def words_closed_form(y):
    """What floorf(fl(y · 65535) + 0.5) is, from exact arithmetic: t = the exact product rounded once to fp32 (through float64,
    where the 24 x 16-bit product is exact); the sum t + 0.5 is exact in fp32 below 2^16 only when t has a bit to spare, so it
    is rounded to fp32 too — from float64, where it is exact."""
    y64 = np.asarray(y, f32).astype(np.float64)
    t = (y64 * 65535.0).astype(f32)                    # exact product (40 bits), one rounding
    s = (t.astype(np.float64) + 0.5).astype(f32)       # exact sum, one rounding
    return np.floor(s).astype(np.uint16)


def make_case(W, H, C, seed=0, kind="random", percentile=50.0):
    """A frame (H, W, C >= 5) whose covered expected depths form the set `kind`:
    random   : depths 0.5..6 and a few negatives, alpha from {inside (0, 1), exact 0, exact 1, above 1, exactly MIN_ALPHA, just
               below it, NaN}; with 8 pixels or more the first ones are forced: alpha == MIN_ALPHA, just below, 0, and (C = 8)
               normal sums of length just under and exactly 1e-6 at alpha = 1;
    none     : no covered pixel;          one / two : exactly that many covered pixels;
    equal    : every covered e equal;     lowbits   : e differ only in their lowest 14 key bits (alpha = 1: e = depth);
    clusters : two clusters ~1 and ~100 of which the lower holds exactly j elements for `percentile`: v[j] and v[j+1] fall in
               different top-level bins;
    signed   : -0.0, +0.0, negatives, denormals, and ordinary values."""
    r = np.random.default_rng(seed)
    n = W * H
    frame = r.uniform(0.0, 1.0, (H, W, C)).astype(f32)
    depth = r.uniform(0.5, 6.0, n).astype(f32)
    alpha = np.ones(n, f32)
    just_below = np.nextafter(MIN_ALPHA, f32(0))
    if kind == "random":
        depth[r.integers(0, 16, n) == 0] *= f32(-1)
        alpha = r.uniform(0.0, 1.0, n).astype(f32)
        pa = r.integers(0, 12, n)
        for v, val in enumerate((0.0, 1.0, 1.125, MIN_ALPHA, just_below, np.nan)):
            alpha[pa == v] = val
        if n >= 8:
            alpha[:3] = (MIN_ALPHA, just_below, 0.0)
    elif kind == "none":
        alpha = r.uniform(0.0, float(just_below), n).astype(f32)
    elif kind in ("one", "two"):
        alpha[:] = 0.0
        alpha[r.choice(n, min(n, 1 if kind == "one" else 2), replace=False)] = 0.75
    else:
        cov = r.integers(0, 4, n) != 0
        if not cov.any():
            cov[:] = True
        alpha = np.where(cov, f32(1), f32(0)).astype(f32)
        m = int(cov.sum())
        if kind == "equal":
            alpha[cov] = 0.5
            depth[:] = 1.25
        elif kind == "lowbits":
            depth[cov] = (np.uint32(0x40490000) + r.integers(0, 1 << 14, m).astype(np.uint32)).view(f32)
        elif kind == "clusters":
            j = rank(m, percentile)[0] if m >= 2 else 0
            vals = np.concatenate([r.uniform(0.9, 1.1, j), r.uniform(90.0, 110.0, m - j)]).astype(f32)
            depth[cov] = r.permutation(vals)
        elif kind == "signed":
            pool = np.array([-0.0, 0.0, -1.5, -1e-30, 1e-45, -1e-45, 3e-39, -3e-39, 2.0, 1e-30, 1.17549435e-38], f32)
            depth[cov] = np.where(r.integers(0, 3, m) == 0, r.uniform(-4.0, 4.0, m).astype(f32), pool[r.integers(0, pool.size, m)])
        else:
            raise ValueError(kind)
    frame[..., 3] = depth.reshape(H, W)
    frame[..., 4] = alpha.reshape(H, W)
    if C >= 8:
        nrm = r.normal(0.0, 1.0, (n, 3)).astype(f32) * r.uniform(0.0, 1.0, (n, 1)).astype(f32)
        nrm[r.integers(0, 16, n) == 0] = 0.0
        if kind == "random" and n >= 8:
            alpha[3:5] = 1.0
            frame[..., 4] = alpha.reshape(H, W)
            nrm[3] = (np.nextafter(TINY, f32(0)), 0.0, 0.0)
            nrm[4] = (0.0, TINY, 0.0)
        frame[..., 5:8] = nrm.reshape(H, W, 3)
    frame.setflags(write=False)
    return frame


def rejected_calls(lib, cam, base=0):
    """Every call the five entry points must refuse on their arguments alone (no pointer is dereferenced) ->
    [(what, return code, message)].  `cam`: a gsr_camera by reference, as the binding passes it; `base`: the address of a
    buffer of 8 KiB that stands for every array (the caller checks that none of its bytes changes), or 0."""
    import ctypes as C
    one, two, odd = C.c_void_p(base + 64), C.c_void_p(base + 4096), C.c_void_p(base + 65)
    nan, inf = float("nan"), float("inf")
    rot9 = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    out = []

    def scale(what, W=8, H=8, Cn=8, image=one, ma=1e-3, pct=99.0, stats=one, scratch=two):
        rc = lib.gsr_depth_scale(W, H, Cn, image, ma, pct, stats, scratch, None)
        out.append(("scale: " + what, rc, lib.gsr_last_error_string().decode()))

    def d16(what, W=8, H=8, Cn=8, image=one, expected=1, ma=1e-3, dmax=5.0, sdev=None, dst=one):
        rc = lib.gsr_frame_depth16(W, H, Cn, image, expected, ma, dmax, sdev, 0, dst, None)
        out.append(("depth16: " + what, rc, lib.gsr_last_error_string().decode()))

    def n8(what, W=8, H=8, Cn=8, image=one, ma=1e-3, rot=None, dst=one):
        rc = lib.gsr_frame_normal8(W, H, Cn, image, ma, rot, dst, None)
        out.append(("normal8: " + what, rc, lib.gsr_last_error_string().decode()))

    def pick(what, W=8, H=8, Cn=8, image=one, camera=cam, px=3, py=3, hw=4, dst=one):
        rc = lib.gsr_pick_point(W, H, Cn, image, camera, px, py, hw, dst, None)
        out.append(("pick: " + what, rc, lib.gsr_last_error_string().decode()))

    for call in (scale, d16, n8, pick):
        call("W = 0", W=0)
        call("H < 0", H=-3)
        call("null image", image=None)
        call("2^32 elements", W=65536, H=8192, Cn=8)
        call("2^32 elements and more", W=1 << 20, H=1 << 20, Cn=8)
    for call in (scale, d16, n8):
        call("min_alpha = 0", ma=0.0)
        call("min_alpha < 0", ma=-1e-3)
        call("min_alpha NaN", ma=nan)
    scale("C = 4", Cn=4)
    d16("expected with C = 4", Cn=4)
    d16("raw with C = 3", Cn=3, expected=0)
    n8("C = 7", Cn=7)
    n8("C = 5", Cn=5)
    pick("C = 3", Cn=3)
    for p in (0.0, -1.0, 100.0000001, nan, inf):
        scale(f"percentile = {p}", pct=p)
    scale("null stats_out", stats=None)
    scale("null scratch", scratch=None)
    scale("scratch not 8-byte aligned", scratch=C.c_void_p(base + 4100))
    d16("both depth_max and scale_dev", dmax=5.0, sdev=two)
    d16("neither depth_max nor scale_dev", dmax=0.0, sdev=None)
    d16("depth_max < 0", dmax=-1.0)
    d16("depth_max < 0 with scale_dev", dmax=-1.0, sdev=two)
    d16("depth_max NaN", dmax=nan, sdev=two)
    d16("depth_max Inf", dmax=inf)
    d16("null output", dst=None)
    d16("output not 2-byte aligned", dst=odd)
    n8("null output", dst=None, rot=rot9)
    pick("null output", dst=None)
    pick("null camera", camera=None)
    pick("half_window = -1", hw=-1)
    pick("half_window = 17", hw=17)
    return out
