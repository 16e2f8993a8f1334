"""numpy restatement of the 3-D smoothing filter (csrc/filter3d.hip, include/gsr.h gsr_filter3d_*), by dtype:
float32 in the stated association — every numpy operation on float32 arrays is one rounded fp32 operation, which is what
the kernel compiles to under -ffp-contract=off — and the float64 twin of the same expressions on the same fp32 inputs.
Also the rig, the points and the hand-placed rows the CPU and GPU tests share.  Pure numpy; no product code, no GPU code."""
import collections
import math

import numpy as np

f32 = np.float32
CAMERA_FLOATS = 22
MARGIN, VARIANCE, NEAR = 0.15, 0.2, 0.2
K = f32(math.sqrt(VARIANCE))

Cam = collections.namedtuple("Cam", "width height focal principal R t")   # the fields smoothing_filter.camera_table reads


# ---- the camera table, restated (include/gsr.h) ----
def camera_table(cameras, margin=MARGIN):
    table = np.zeros((len(cameras), CAMERA_FLOATS), f32)
    for row, cam in zip(table, cameras):
        R = np.asarray(cam.R, f32)
        res = np.array([cam.width, cam.height], f32)
        focal = np.array(cam.focal, f32)
        for i in range(3):
            for j in range(3):
                row[i + 3 * j] = R[i, j]
        row[9:12] = np.asarray(cam.t, f32)
        row[12:14] = focal
        row[14:16] = np.array(cam.principal, f32) * res
        row[16:18] = f32(-margin) * res
        row[18:20] = f32(1.0 + margin) * res
        row[20] = f32(1) / max(focal[0], focal[1])
    return table


# ---- the sweep ----
Sweep = collections.namedtuple("Sweep", "filter seen count valid tau zmag")


def sweep(points, table, near=NEAR, k=K, dtype=f32):
    """gsr_filter3d_compute on (N, 3) points and a (V, 22) table, both fp32 data, evaluated in `dtype`.  -> Sweep: filter (N,),
    seen (N,) bool, count, valid (V, N) bool, tau (V, N), zmag (V, N) = Σ_j |R[2+3j]·p_j| + |t[2]| (the magnitude the
    roundings of z scale with)."""
    P = np.asarray(points, f32).astype(dtype)
    T = np.asarray(table, f32).astype(dtype)
    near, k = dtype(f32(near)), dtype(f32(k))
    n, V = P.shape[0], T.shape[0]
    p0, p1, p2 = P[:, 0], P[:, 1], P[:, 2]
    tmin = np.full(n, np.inf, dtype)
    seen = np.zeros(n, bool)
    valid_all, tau_all, zmag = np.zeros((V, n), bool), np.zeros((V, n), dtype), np.zeros((V, n), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for v, c in enumerate(T):
            xc = [((c[i] * p0 + c[i + 3] * p1) + c[i + 6] * p2) + c[9 + i] for i in range(3)]
            z = xc[2]
            valid = z > near
            for j in range(2):
                u = c[12 + j] * xc[j] + c[14 + j] * z
                valid = valid & (c[16 + j] * z <= u) & (u <= c[18 + j] * z)
            tau = z * c[20]
            tmin = np.where(valid, np.fmin(tmin, tau), tmin)
            seen |= valid
            valid_all[v], tau_all[v] = valid, tau
            c64 = c.astype(np.float64)
            zmag[v] = np.abs(c64[2] * P[:, 0]) + np.abs(c64[5] * P[:, 1]) + np.abs(c64[8] * P[:, 2]) + abs(c64[11])
        filt = k * tmin
        fill = np.fmax.reduce(filt[seen]) if seen.any() else dtype(0)
        filt = np.where(seen, filt, fill).astype(dtype)
    return Sweep(filt, seen, int(seen.sum()), valid_all, tau_all, zmag)


def sweep_bound(twin, table, k=K):
    """The bound on |filter32 - filter64| per SEEN point whose validity sets agree: 3e-7 · k · inv_f · (Σ_j |R[2+3j]·p_j| + |t[2]|)
    of the camera that attains the twin's minimum — four roundings of z, magnitude-weighted because the sum can cancel, one
    each for tau and k·, a margin of about 2 (7 · 2^-24 = 4.2e-7 would be every rounding at its worst at once)."""
    T = np.asarray(table, np.float64)
    tau = np.where(twin.valid, twin.tau, np.inf)
    arg = tau.argmin(0)
    cols = np.arange(tau.shape[1])
    return 3e-7 * float(k) * T[arg, 20] * twin.zmag[arg, cols]


# ---- apply and its pullback ----
Row = collections.namedtuple("Row", "se r c o_eff")


def _row(o, s, f, dtype):
    o, s, f = np.asarray(o, f32).astype(dtype).reshape(-1), np.asarray(s, f32).astype(dtype), np.asarray(f, f32).astype(dtype)
    f2 = (f * f)[:, None]
    se = np.sqrt(s * s + f2)
    r = s / se
    c = (r[:, 0] * r[:, 1]) * r[:, 2]
    return o, s, f2, Row(se, r, c, o * c)


def apply(o, s, f, dtype=f32):
    """gsr_filter3d_apply: (opacities_eff (N,), scales_eff (N, 3))."""
    _, _, _, w = _row(o, s, f, dtype)
    return w.o_eff, w.se


def apply_raw(o, s, f, dtype=f32):
    """raw != 0: (logit(o_eff), log(se)), 1 - o_eff formed without cancellation as the kernel does."""
    o, s, f2, w = _row(o, s, f, dtype)
    d = f2 / (w.se * (w.se + s))
    one_minus_c = d[:, 0] + w.r[:, 0] * (d[:, 1] + w.r[:, 1] * d[:, 2])
    one_minus_oe = (dtype(1) - o) + o * one_minus_c
    with np.errstate(divide="ignore"):
        return np.log(w.o_eff / one_minus_oe), np.log(w.se)


def apply_backward(o, s, f, g_o, g_s, dtype=f32, terms=False):
    """gsr_filter3d_apply_backward: (vo (N,), vs (N, 3)); terms=True: also the two terms of vs, g_s·r and the filter's."""
    o, s, f2, w = _row(o, s, f, dtype)
    g_o, g_s = np.asarray(g_o, f32).astype(dtype).reshape(-1), np.asarray(g_s, f32).astype(dtype)
    r = w.r
    P = np.stack([r[:, 1] * r[:, 2], r[:, 0] * r[:, 2], r[:, 0] * r[:, 1]], 1)
    first = g_s * r
    second = ((g_o * o)[:, None] * P) * (f2 / ((w.se * w.se) * w.se))
    vo, vs = g_o * w.c, first + second
    return (vo, vs, first, second) if terms else (vo, vs)


# ---- the rig and the points of the sweep tests ----
N_CASES = (1, 63, 64, 65, 257, 1025)   # 257: the lone thread of a second workgroup of the fill; 1025: past one workgroup's 4 x 256 points
V_CASES = (1, 2, 3, 33)                # 33: past any 32-camera staging chunk
SHAPES = ((64, 48, (64.0, 80.0), (0.5, 0.375)), (33, 17, (21.5, 19.25), (0.47, 0.55)), (80, 64, (90.0, 70.0), (0.52, 0.46)))


def make_rig(V):
    """V cameras on an arc around the origin looking along +z: three resolutions in turn (33 x 17 among them), fx != fy, an
    off-centre principal.  Camera 0 is the identity pose with power-of-two friendly intrinsics: the hand-placed rows are
    exact against it."""
    cams = []
    for v in range(V):
        W, H, focal, principal = SHAPES[v % 3]
        a = math.radians(2.5 * ((v + 1) // 2) * (-1 if v % 2 else 1))   # 33 cameras: within +-40 degrees
        R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
        t = -R @ np.array([0.25 * v * (-1 if v % 2 else 1), 0.05 * (v % 5), -0.1 * (v % 4)])
        cams.append(Cam(W, H, focal, principal, R.astype(f32), t.astype(f32)))
    return cams


def _solve_u(c, j, edge, z):
    """A coordinate x (fp32) with focal[j]*x + pp[j]*z == edge[j]*z in fp32, exactly, for camera row `c` at the identity pose."""
    z = f32(z)
    want = c[edge + j] * z
    x0 = f32((want - c[14 + j] * z) / c[12 + j])
    cand = [x0]
    lo = hi = x0
    for _ in range(64):
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        cand += [lo, hi]
    for x in cand:
        if f32(c[12 + j] * f32(x)) + c[14 + j] * z == want:
            return f32(x)
    return None


HAND = ("z == near", "z just past near", "u0 == hi0 z", "u0 == lo0 z", "u1 == hi1 z", "u1 == lo1 z", "behind every camera", "NaN")


def hand_rows(table, near=NEAR):
    """The hand-placed points, in the order of HAND, exact against camera row 0 (identity pose)."""
    c = np.asarray(table, f32)[0]
    assert np.array_equal(c[:12], np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)), "camera 0 must be the identity pose"
    rows = [(0.0, 0.0, f32(near)), (0.0, 0.0, np.nextafter(f32(near), f32(np.inf)))]
    for j in range(2):
        for edge in (18, 16):
            # (the sum focal*x + pp*z is exact on the grid of its larger operand: only a depth whose edge*z falls on that
            # grid has a solution — one in four or so)
            for z in (1.0, 2.0) + tuple(1.0 + i / 32.0 for i in range(1, 64)):
                x = _solve_u(c, j, edge, z)
                if x is not None:
                    break
            assert x is not None, ("no exact edge point", j, edge)
            rows.append((x, 0.0, z) if j == 0 else (0.0, x, z))
    rows += [(0.1, -0.2, -5.0), (np.nan, 0.0, 1.0)]
    return np.array(rows, f32)


def make_points(n, table=None, seed=0):
    """normal · 3 around the rig; with a table, the hand rows first (as many as fit)."""
    pts = (np.random.default_rng(1000 * seed + n).standard_normal((n, 3)) * 3.0 + np.array([0.0, 0.0, 1.5])).astype(f32)
    if table is not None:
        hand = hand_rows(table)
        m = min(n, hand.shape[0])
        pts[:m] = hand[:m]
    return pts


def unseen_points(n, seed=0):
    """A cloud behind every camera of make_rig: no point is seen."""
    pts = (np.random.default_rng(77 + seed).standard_normal((n, 3)) * 0.5).astype(f32)
    pts[:, 2] = -np.abs(pts[:, 2]) - f32(3.0)
    return pts


# ---- the final fold past two partials: (n, the workgroup of the sweep that holds the largest filter) ----
WG_POINTS = 1024                        # points per workgroup of the sweep: one partial maximum and count each
FOLD_V = 2
FOLD_CASES = ((64 * 1024 + 1, 64),      # 65 partials: the final's wave 1 holds one, the LAST, and with it the maximum
              (257 * 1024 + 1, 257),    # 258 partials: threads 0 and 1 take a second trip; the maximum comes in on thread 1's
              (257 * 1024 + 1, 200))    # ... and from thread 200 (wave 3) on the first trip
FOLD_FAR = 64.0                         # make_points stays within z < 20 (1.5 + 6 sigma)


def fold_points(n, wg, table):
    """make_points with the hand rows, and ONE point far out on camera 0's axis — seen, with the largest filter of all — in
    workgroup `wg` of the sweep: the last point of the array when that is the last workgroup (which holds nothing else)."""
    pts = make_points(n, table, seed=3)
    at = min(wg * WG_POINTS + 517, n - 1)
    pts[at] = (0.0, 0.0, FOLD_FAR)
    return pts, at


_fold = {}


def fold_case(n, wg):
    """-> (table, points, the index of the far point, the fp32 sweep) of a FOLD_CASES entry; computed once, read-only."""
    if (n, wg) not in _fold:
        table = camera_table(make_rig(FOLD_V))
        pts, at = fold_points(n, wg, table)
        _fold[n, wg] = table, pts, at, sweep(pts, table, dtype=f32)
    return _fold[n, wg]


# ---- the rows of the apply tests ----
def apply_rows(n, seed=0):
    """o in [0.004, 0.999], s log-uniform in [1e-4, 10], f log-uniform in [1e-4, 1], normal cotangents."""
    rng = np.random.default_rng(4242 + seed)
    s = np.exp(rng.uniform(math.log(1e-4), math.log(10.0), (n, 3))).astype(f32)
    f = np.exp(rng.uniform(math.log(1e-4), math.log(1.0), n)).astype(f32)
    o = rng.uniform(0.004, 0.999, n).astype(f32)
    return o, s, f, rng.standard_normal(n).astype(f32), rng.standard_normal((n, 3)).astype(f32)


def edge_rows(n=257, seed=1):
    """apply_rows with every third row f == 0 (pass-through) and every fifth s = 1e-6, f = 1; the last row — the lone thread of
    a second workgroup — is a pass-through row."""
    o, s, f, g_o, g_s = apply_rows(n, seed)
    f[::3] = 0.0
    s[1::5] = f32(1e-6)
    f[1::5] = 1.0
    f[n - 1] = 0.0
    return o, s, f, g_o, g_s


def rel(a, b):
    """|a - b| / |b| elementwise in float64 (0 where both are 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a == b, 0.0, np.abs(a - b) / np.abs(b))
