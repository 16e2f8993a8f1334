"""The float64 DEFINITION of adaptive density control: what csrc/densify.hip and the findall / gather / non-finite passes of
csrc/trainer.hip are held to by tests/test_gpu_density_edges.py, and what tests/test_densify_ref_cpu.py compares with the fp32
restatement oracle/densify.py.  Plain numpy, statement by statement from include/gsr.h (the block above gsr_densify_grad_mean)
and oracle/densify.py; TEST INFRASTRUCTURE ONLY.

Three kinds of statement:
  exact      grad_mean (one IEEE fp32 division), morton (fp32 as written), compose / gather / nonfinite (indexing), the
             uniforms of the split noise (integers and one exact fp32 sum): compared bit for bit;
  decided    masks: evaluated in float64 from the fp32 inputs; a row whose exp or sigmoid lies within MARGIN of the threshold
             it is compared with is reported as undecided and left out of a comparison;
  float64    split_children, reset_opacity: everything after the fp32 inputs in float64; compared within the error that the
             fp32 restatement itself has against them (test_densify_ref_cpu.py measures it) times TOL_FACTOR.

The second half of the file holds the inputs that the CPU test and the GPU test share, so that the tolerances of the GPU test
are measured on the GPU test's own rows without either test importing the other.
"""
import numpy as np

from oracle import densify as dz

f32, f64 = np.float32, np.float64
CLONE, SPLIT, PRUNE = 0, 1, 2          # GSR_DENSIFY_*
COMPOSE_WORDS = 2048                   # csrc/densify.hip: words one workgroup of compose_rows_kernel composes
FLT_MAX = f64(np.finfo(f32).max)

# A row is undecided when its float64 max(exp(scales)) lies within a relative MARGIN of gamma, or its sigmoid(opacity) within a
# relative MARGIN of min_opacity.  2^-19 is 16 to 32 fp32 ulps (an ulp is 2^-23 to 2^-24 of the value): the HIP math library
# documents expf at 1 ulp, the sigmoid adds one rounded sum and one correctly rounded division (under 3 ulps together), glibc
# is below 1 ulp — the margin is an order above any of them, and still leaves a random model with (almost) no undecided row.
MARGIN = 2.0 ** -19


def _flat32(a):
    return np.ascontiguousarray(a, f32).reshape(-1)


def grad_mean(accum, denom):
    """accum ./ denom as ONE IEEE fp32 division, NaN -> 0, +-Inf kept (densification.jl:7-10).  Exact."""
    with np.errstate(invalid="ignore", divide="ignore", under="ignore", over="ignore"):
        g = (_flat32(accum) / _flat32(denom)).astype(f32)
    g[np.isnan(g)] = 0
    return g


def max_exp_scale64(scales, n):
    """float64 maximum(exp.(scales); dims=1); a NaN on any axis gives NaN (np.max, Julia's maximum)."""
    s = np.asarray(scales, f32).reshape(n, -1).astype(f64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(s).max(axis=1)


def _near(v, ref, exact):
    """|v - ref| within the relative MARGIN, unless v is exact in every implementation (exp(+-0) == 1)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(v - ref) <= MARGIN * abs(ref)) & ~exact


def masks(kind, grad, n_grad, scales, opacities, max_radii, thr, gamma, min_opacity, max_screen_size):
    """(mask, decided) of gsr_densify_mask.  thr, gamma, min_opacity are taken as the fp32 values the C ABI receives.
      CLONE: padded_grad >  thr && max(exp(scales)) < gamma        SPLIT: padded_grad >= thr && max(exp(scales)) > gamma
      PRUNE: sigmoid(opacity) > min_opacity [&& max_radii < max_screen_size && max(exp(scales)) < gamma, if max_screen_size > 0]
    padded_grad is grad[:n_grad] followed by zeros.  A NaN grad, scale or opacity makes every comparison on its row false.  The
    grad and max_radii comparisons are exact, never undecided."""
    thr, gamma, min_opacity = f64(f32(thr)), f64(f32(gamma)), f64(f32(min_opacity))
    if kind == PRUNE:
        o = _flat32(opacities).astype(f64)
        n = o.shape[0]
        with np.errstate(over="ignore", invalid="ignore"):
            sg = 1.0 / (1.0 + np.exp(-o))
            mask = sg > min_opacity
        decided = ~_near(sg, min_opacity, np.zeros(n, bool))
        if max_screen_size > 0:
            mx = max_exp_scale64(scales, n)
            exact = _exact_exp(scales, n)
            with np.errstate(invalid="ignore"):
                mask = mask & (np.asarray(max_radii).reshape(-1) < max_screen_size) & (mx < gamma)
            decided &= ~_near(mx, gamma, exact)
        return mask, decided
    n = np.asarray(scales).shape[0]                            # scales: (n, scale_dims)
    padded = np.zeros(n, f64)
    if n_grad > 0:
        padded[:n_grad] = _flat32(grad)[:n_grad]
    mx = max_exp_scale64(scales, n)
    with np.errstate(invalid="ignore"):
        mask = (padded > thr) & (mx < gamma) if kind == CLONE else (padded >= thr) & (mx > gamma)
    return mask, ~_near(mx, gamma, _exact_exp(scales, n))


def _exact_exp(scales, n):
    """Rows whose largest scale is exactly +-0: exp is exactly 1 there in every implementation (C Annex F), so a comparison
    of it with gamma == 1 is decided although it sits ON the threshold."""
    s = np.asarray(scales, f32).reshape(n, -1)
    with np.errstate(invalid="ignore"):
        return s.max(axis=1) == 0


def normals(seed, n):
    """The split noise of rows 0..n-1: (xi, r), both (n,3) float64.  The four uniforms are oracle.densify.uniform01 — integers,
    one exact fp32 sum and one exact scaling by 2^-24 — and the angle is the fp32-rounded product two_pi * u; the logarithm, the
    square root and the cosine / sine are float64.  r is the Box-Muller radius that multiplies each component: an error of the
    cosine is scaled by it, so errors of xi are measured in units of max(1, r)."""
    rows = np.arange(n, dtype=np.uint32)
    u1, u2, u3, u4 = (dz.uniform01(seed, rows, d) for d in range(4))
    tp = f32(6.2831853071795864)
    a1, a2 = (tp * u2).astype(f32).astype(f64), (tp * u4).astype(f32).astype(f64)
    r1, r2 = np.sqrt(-2.0 * np.log(u1.astype(f64))), np.sqrt(-2.0 * np.log(u3.astype(f64)))
    return np.stack([r1 * np.cos(a1), r1 * np.sin(a1), r2 * np.cos(a2)], 1), np.stack([r1, r1, r2], 1)


def quat2rot64(q):
    """unnorm_quat2rot (render.jl:322-333) in float64, (n,3,3) row-major; a zero quaternion gives NaN."""
    q = np.asarray(q, f32).reshape(-1, 4).astype(f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.sqrt((q * q).sum(1))
        w, x, y, z = (q[:, k] * inv for k in range(4))
    R = np.empty((q.shape[0], 3, 3), f64)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def split_children(points, rots, scales, seed, scale_dims):
    """gsr_split_transform on n appended rows: (new points (n,3), new scales (n,scale_dims), sigma * xi (n,3)), float64.
      sigma = exp(scale);  point += R(q) (sigma .* xi);  scale = log(sigma / (0.8f0 * 2))      (densification.jl:80-104,121-135)"""
    p = np.asarray(points, f32).reshape(-1, 3).astype(f64)
    n = p.shape[0]
    s = np.asarray(scales, f32).reshape(n, scale_dims).astype(f64)
    sigma = np.exp(s)
    xi, _ = normals(seed, n)
    sx = sigma * xi                                            # (n,1) broadcasts: the isotropic model
    step = np.einsum("nij,nj->ni", quat2rot64(rots), sx)
    return p + step, np.log(sigma / f64(f32(0.8) * f32(2))), sx


def reset_opacity(o):
    """inverse_sigmoid(min(0.1f0, sigmoid(o))) in float64 (gaussians.jl:118-126,137).  A NaN stays a NaN (Julia's min and
    np.minimum propagate it).  Where the fp32 sigmoid underflows — exp(-o) beyond FLT_MAX, so 1 / (1 + Inf) = 0 — the result is
    log(0) = -Inf, as in the restatement."""
    o = _flat32(o).astype(f64)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        e = np.exp(-o)
        sg = np.where(e > FLT_MAX, 0.0, 1.0 / (1.0 + e))
        m = np.minimum(f64(f32(0.1)), sg)
        return np.log(m / (1.0 - m))


def morton(points, lo, hi, bits=21):
    """gsr_morton_codes, exact: the fp32 arithmetic of the entry point (inv = 1 / (hi - lo), 0 on a degenerate axis) and of the
    kernel (t = (v - lo) * inv; NaN -> 0; clamp to [0, 1]; cell = trunc(t * (2^bits - 1))), x in the lowest bit of each triple."""
    p = np.asarray(points, f32).reshape(-1, 3)
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    ext = (hi - lo).astype(f32)
    assert (ext >= 0).all(), "box_hi < box_lo: GSR_E_INVALID_ARG"
    inv = np.where(ext > 0, f32(1.0) / np.where(ext > 0, ext, f32(1.0)), f32(0.0)).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((p - lo).astype(f32) * inv).astype(f32)
        t = np.where(np.isnan(t), f32(0.0), np.clip(t, f32(0.0), f32(1.0))).astype(f32)
    cells = (t * f32(2 ** bits - 1)).astype(f32).astype(np.uint64)
    codes = np.zeros(p.shape[0], np.uint64)
    for b in range(bits):
        for a in range(3):
            codes |= ((cells[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + a)
    return codes


def compose(src, keep_idx, n_keep, sel_idx, n_sel, reps, new_zero):
    """gsr_compose_rows for one array of rows:  dst[r] = src[keep_idx[r]] (keep_idx None: r) for r < n_keep;
    dst[n_keep + k * n_sel + j] = new_zero ? 0 : src[sel_idx[j]] for j < n_sel, k < reps."""
    kept = src[:n_keep] if keep_idx is None else src[np.asarray(keep_idx, np.int64)[:n_keep]]
    m = n_sel * reps
    if new_zero or m == 0:
        new = np.zeros((m, src.shape[1]), src.dtype)
    else:
        new = np.tile(src[np.asarray(sel_idx, np.int64)[:n_sel]], (reps, 1))
    return np.concatenate([kept, new], 0)


def gather(src, idx):
    """gsr_gather_rows: dst[r] = src[idx[r]]"""
    return src[np.asarray(idx)]


def nonfinite(arrays):
    """gsr_count_nonfinite: per array of rows, (number of rows with a NaN or +-Inf entry, index of the first one or
    0xFFFFFFFF), as uint32 vectors."""
    counts, first = [], []
    for a in arrays:
        bad = np.flatnonzero(~np.isfinite(np.asarray(a, f32).reshape(a.shape[0], -1)).all(axis=1))
        counts.append(bad.size)
        first.append(bad[0] if bad.size else 0xFFFFFFFF)
    return np.asarray(counts, np.uint32), np.asarray(first, np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# The inputs that tests/test_densify_ref_cpu.py and tests/test_gpu_density_edges.py share.

# What the fp32 restatement (oracle/densify.py: numpy fp32 on glibc) is off the float64 definition by, on the rows below —
# measured by test_densify_ref_cpu.py, which fails if a figure here is exceeded — rounded up to two digits:
#   normal   |xi error| / max(1, r)                 per component of the Box-Muller normals
#   step     |point error| / |sigma .* xi|          3-vector norms; the rounding of the sum onto the parent's position is in it
#   scale    |new scale error|                      absolute
#   reset    |reset opacity error|                  absolute, rows with sigmoid(o) < 0.1
RESTATEMENT_ERR = dict(normal=1.3e-7, step=1.2e-5, scale=2.8e-7, reset=2.4e-7)
# The kernel is allowed TOL_FACTOR times that: the device's expf / logf / sinf / cosf are documented at 1 to 2 ulps where
# glibc's are below one, and everything else in the kernels is the restatement's own fp32 arithmetic.
TOL_FACTOR = 4.0

MASK_ROWS = 4096
MASK_N = (1, 255, 256, 257, MASK_ROWS)
GAMMAS = (0.05, 0.5, float(np.exp(-1.0)))
MIN_OPACITIES = (0.005, 0.3)
MASK_THR, MASK_SCREEN = 2e-4, 20


def mask_case(sd):
    """The random model of the mask tests (its first n rows are the case of n rows): scales N(-3, 1), opacities N(-1, 2),
    gradients around the threshold MASK_THR, radii around MASK_SCREEN."""
    rng = np.random.default_rng(0)
    scales = rng.normal(-3.0, 1.0, (MASK_ROWS, sd)).astype(f32)
    opac = rng.normal(-1.0, 2.0, (MASK_ROWS, 1)).astype(f32)
    grad = rng.gamma(2.0, 1e-4, MASK_ROWS).astype(f32)
    radii = rng.integers(0, 2 * MASK_SCREEN, MASK_ROWS).astype(np.int32)
    return scales, opac, grad, radii


SPLIT_ROWS, SPLIT_N, SPLIT_SEEDS = 257, (1, 255, 256, 257), (77, 78)


def split_cases(sd):
    """name -> (points, rotations, scales) of SPLIT_ROWS rows: a make_model-like random model; the same with its quaternions
    scaled by 1e-3 and by 1e3; and the identity frame at scale 0 on the origin, whose children ARE the normal triples."""
    rng = np.random.default_rng(100 + sd)
    p = rng.normal(size=(SPLIT_ROWS, 3)).astype(f32)
    q = rng.normal(size=(SPLIT_ROWS, 4)).astype(f32)
    s = rng.normal(-3.0, 1.0, (SPLIT_ROWS, sd)).astype(f32)
    ident = np.tile(f32([1, 0, 0, 0]), (SPLIT_ROWS, 1))
    return {"random": (p, q, s), "q*1e-3": (p, (q * f32(1e-3)).astype(f32), s), "q*1e3": (p, (q * f32(1e3)).astype(f32), s),
            "identity": (np.zeros((SPLIT_ROWS, 3), f32), ident, np.zeros((SPLIT_ROWS, sd), f32))}


RESET_CUT = float(np.log(1.0 / 9.0))   # sigmoid(o) == 0.1


def reset_case():
    """(o, above): opacities N(-1, 2) behind the hand rows — the fp32 neighbours of the cut on either side, rows well above it
    (`above`: their sigmoid exceeds 0.1 by more than MARGIN, so the kernel must return min's constant branch), +-100, +Inf."""
    c = f32(RESET_CUT)
    hand = f32([np.nextafter(c, f32(-9)), c, np.nextafter(c, f32(9)), c + f32(2.0 ** -10), -2.0, -0.0, 0.0, 1.0, 5.0, 100.0, np.inf,
                -100.0, c - f32(2.0 ** -10), -5.0, -6.0, -7.5])
    o = np.concatenate([hand, np.random.default_rng(5).normal(-1.0, 2.0, 1024).astype(f32)])
    sg = 1.0 / (1.0 + np.exp(-o.astype(f64)))
    return o, sg > f64(f32(0.1)) * (1.0 + MARGIN)


def hand_mask_calls(sd):
    """The hand rows of gsr_densify_mask as calls: dicts of the entry point's arguments (numpy arrays or None) plus `expect`,
    the mask written down by hand, and `name`.  A scale row is given as a triple; the isotropic model takes the NaN if the triple
    has one and its largest entry otherwise, which leaves every expectation as it is."""
    nan, inf = f32(np.nan), f32(np.inf)
    T = f32(MASK_THR)

    def S(*rows):
        a = f32(rows).reshape(-1, 3)
        if sd == 3:
            return a
        return np.where(np.isnan(a).any(1), nan, np.nanmax(np.where(np.isnan(a), -inf, a), axis=1)).astype(f32).reshape(-1, 1)

    def call(name, kind, scales=None, grad=None, n_grad=None, opac=None, radii=None, thr=T, gamma=1.0, min_opacity=0.005, mss=0,
             expect=None):
        n = len(expect)
        grad = None if grad is None else f32(grad)
        return dict(name=f"{name}/{('clone', 'split', 'prune')[kind]}/sd{sd}", kind=kind, n=n,
                    n_grad=(0 if grad is None else len(grad)) if n_grad is None else n_grad, grad=grad, scales=scales,
                    opacities=None if opac is None else f32(opac).reshape(-1, 1),
                    max_radii=None if radii is None else np.asarray(radii, np.int32), thr=float(thr), gamma=float(gamma),
                    min_opacity=float(min_opacity), max_screen_size=mss, expect=np.asarray(expect, np.uint8))

    small, big = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)           # exp < 1 = gamma < exp
    up, down = np.nextafter(T, inf), np.nextafter(T, f32(0))
    g8 = [T, up, down, nan, inf, -inf, 1.0, 1.0]                # the last two lie beyond n_grad = 6: they count as 0
    calls = [
        # grad == thr, one ulp either side, NaN, +-Inf; rows at and beyond n_grad under a positive threshold
        call("grad edges", CLONE, S(*[small] * 8), g8, n_grad=6, expect=[0, 1, 0, 0, 1, 0, 0, 0]),
        call("grad edges", SPLIT, S(*[big] * 8), g8, n_grad=6, expect=[1, 1, 0, 0, 1, 0, 0, 0]),
        # ... and the other side of the scale test switches every row off
        call("grad edges, wrong size", CLONE, S(*[big] * 8), g8, n_grad=6, expect=[0] * 8),
        call("grad edges, wrong size", SPLIT, S(*[small] * 8), g8, n_grad=6, expect=[0] * 8),
        # thr = 0: a padded row is 0, not > 0 but >= 0; the split still needs the scale
        call("thr 0", CLONE, S(small, small, small, small), [0.0, 1.0], thr=0.0, expect=[0, 1, 0, 0]),
        call("thr 0", SPLIT, S(big, big, big, small), [0.0, -0.0], thr=0.0, expect=[1, 1, 1, 0]),
        # a negative threshold: padded rows pass both
        call("thr < 0", CLONE, S(small, small, small, big), [-2.0, -0.5], thr=-1.0, expect=[0, 1, 1, 0]),
        call("thr < 0", SPLIT, S(big, big, big, small), [-2.0, -1.0], thr=-1.0, expect=[0, 1, 1, 0]),
        # n_grad = 0 with a NULL grad: every row is padded
        call("no grad", CLONE, S(small, big, small), None, thr=0.0, expect=[0, 0, 0]),
        call("no grad", SPLIT, S(small, big, big), None, thr=0.0, expect=[0, 1, 1]),
        call("no grad", CLONE, S(small, big, small), None, thr=-1.0, expect=[1, 0, 1]),
    ]
    # the scale test: exp(0) == 1 == gamma exactly is neither < nor >; the largest scale on each axis in turn; a NaN on each axis
    rows = [(0.0, 0.0, 0.0), (0.0, -1.0, -1.0), (-1.0, 0.0, -1.0), (-1.0, -1.0, -0.0), (2.0, -1.0, -1.0), (-1.0, 2.0, -1.0),
            (-1.0, -1.0, 2.0), small, (nan, -1.0, -1.0), (-1.0, nan, 2.0), (2.0, -1.0, nan), (nan, nan, nan), (-inf, -inf, -inf),
            (-1.0, inf, -1.0)]
    n = len(rows)
    calls += [
        call("scales", CLONE, S(*rows), [1.0] * n, expect=[0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]),
        call("scales", SPLIT, S(*rows), [1.0] * n, expect=[0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1]),
        call("scales", PRUNE, S(*rows), opac=[0.0] * n, radii=[0] * n, mss=20, expect=[0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]),
        # max_radii == max_screen_size is not below it; one below is
        call("radii", PRUNE, S(*[small] * 5), opac=[0.0] * 5, radii=[20, 19, 21, 0, -1], mss=20, expect=[0, 1, 0, 1, 1]),
        # max_screen_size = 0: the scales hold poison and are not read, max_radii is NULL; opacity +-100, NaN, +-Inf
        call("opacity only", PRUNE, S(*[(nan, nan, nan)] * 7), opac=[100.0, -100.0, nan, 0.0, -30.0, inf, -inf], expect=[1, 0, 0, 1, 0, 1, 0]),
        call("opacity", PRUNE, S(*[small] * 7), opac=[100.0, -100.0, nan, 0.0, -30.0, inf, -inf], radii=[0] * 7, mss=20,
             expect=[1, 0, 0, 1, 0, 1, 0]),
    ]
    return calls
