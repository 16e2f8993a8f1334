"""numpy restatement of the TSDF fusion and the surface-nets extraction (csrc/tsdf.hip, include/gsr.h gsr_tsdf_integrate /
gsr_mesh_count / gsr_mesh_emit), by dtype: float32 in the stated association — every numpy operation on float32
arrays is one rounded fp32 operation, which is what the kernels compile to under -ffp-contract=off — and the float64 twin of
the same expressions on the same fp32 inputs.  Also the analytic sphere scene, the random frames and volumes and the mesh
conditions the CPU and GPU tests share.  Pure numpy; no product code, no GPU code.

Arrays of a volume are shaped (nz, ny, nx): C order is the linear index l = i + nx·(j + ny·k)."""
import collections
import math

import numpy as np

f32 = np.float32
EPS = 2.0 ** -24           # the unit roundoff of fp32
MIN_ALPHA, NEAR = 1e-3, 0.2

Cam = collections.namedtuple("Cam", "width height focal principal R t")   # R (3, 3) world -> camera, row-major; t (3,)
Mesh = collections.namedtuple("Mesh", "vertices faces colors n_vertices n_quads")


class Volume:
    """dims = (nx, ny, nz); sample (i, j, k) at origin + h·(i, j, k).  A fresh volume is tsdf = 1, weight = 0."""

    def __init__(self, dims, origin, h, trunc, color=False, dtype=f32):
        nx, ny, nz = (int(d) for d in dims)
        self.dims, self.dtype = (nx, ny, nz), dtype
        self.origin = np.asarray(origin, f32)
        self.h, self.trunc = f32(h), f32(trunc)
        self.tsdf = np.ones((nz, ny, nx), dtype)
        self.weight = np.zeros((nz, ny, nx), dtype)
        self.color = np.zeros((nz, ny, nx, 3), dtype) if color else None
        # float64 twin only: the largest per-view bound on the error of s that fp32 may make at this sample (`integrate`)
        self.s_bound = np.zeros((nz, ny, nx), np.float64)
        self.views = []     # per view: (ok, iu, iv) — the decision and the pixel of every sample

    def packed(self):
        """(nz, ny, nx, 2): the device's {tsdf, weight} pairs."""
        return np.stack([self.tsdf, self.weight], -1)


def integrate(vol, image, cam, min_alpha=MIN_ALPHA, near=NEAR):
    """gsr_tsdf_integrate of one (H, W, C >= 5) fp32 frame into `vol`, evaluated in vol.dtype."""
    T = vol.dtype
    nx, ny, nz = vol.dims
    img = np.asarray(image, f32).astype(T)
    H, W = img.shape[:2]
    o, h, trunc = vol.origin.astype(T), T(vol.h), T(vol.trunc)
    R, t = np.asarray(cam.R, f32).astype(T), np.asarray(cam.t, f32).astype(T)
    fx, fy = T(f32(cam.focal[0])), T(f32(cam.focal[1]))
    cx, cy = T(f32(cam.principal[0])) * T(f32(W)), T(f32(cam.principal[1])) * T(f32(H))
    min_alpha, near = T(f32(min_alpha)), T(f32(near))
    px = (o[0] + h * np.arange(nx).astype(T))[None, None, :]
    py = (o[1] + h * np.arange(ny).astype(T))[None, :, None]
    pz = (o[2] + h * np.arange(nz).astype(T))[:, None, None]
    with np.errstate(all="ignore"):
        pc = [((R[r, 0] * px + R[r, 1] * py) + R[r, 2] * pz) + t[r] for r in range(3)]
        z = np.broadcast_to(pc[2], (nz, ny, nx))
        ok = z > near
        u = (fx * pc[0]) / z + cx
        v = (fy * pc[1]) / z + cy
        fu, fv = np.floor(u + T(0.5)), np.floor(v + T(0.5))
        ok = ok & (fu >= 0) & (fu < T(W)) & (fv >= 0) & (fv < T(H))      # the range, tested in float
        iu, iv = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
        alpha = img[iv, iu, 4]
        ok = ok & (alpha >= min_alpha)
        d = img[iv, iu, 3] / alpha
        sdf = d - z
        ok = ok & (sdf >= -trunc)
        s = np.minimum(T(1), sdf / trunc)
        w = vol.weight
        w1 = w + T(1)
        new_tsdf = (vol.tsdf * w + s) / w1
        if vol.color is not None:
            q = np.fmin(np.fmax(img[iv, iu, :3] / alpha[..., None], T(0)), T(1))     # fmaxf / fminf: a NaN becomes 0
            new_color = (vol.color * w[..., None] + q) / w1[..., None]
            vol.color = np.where(ok[..., None], new_color, vol.color).astype(T)
        vol.tsdf = np.where(ok, new_tsdf, vol.tsdf).astype(T)
        vol.weight = np.where(ok, w1, w).astype(T)
        if T is np.float64:
            # what fp32 may lose on s here: 8 roundings on the way to z, each of a value of at most zmag; one on d; one on
            # sdf = d - z (at most |d| + |z|); one on the quotient (|s| <= 1 where the clamp does not hide it)
            zmag = (np.abs(R[2, 0]) * (abs(o[0]) + np.abs(h * np.arange(nx)))[None, None, :]
                    + np.abs(R[2, 1]) * (abs(o[1]) + np.abs(h * np.arange(ny)))[None, :, None]
                    + np.abs(R[2, 2]) * (abs(o[2]) + np.abs(h * np.arange(nz)))[:, None, None] + abs(t[2]))
            es = EPS * ((8.0 * zmag + 2.0 * np.abs(d) + np.abs(z)) / trunc + 1.0)
            vol.s_bound = np.where(ok, np.maximum(vol.s_bound, es), vol.s_bound)
    vol.views.append((ok, iu, iv))
    return ok


def tsdf_bound(vol64):
    """|tsdf32 - tsdf64| of a sample whose decisions and pixels agree in every view: the running mean passes the largest
    per-view error of s on undamped at worst, and each of its w updates adds three roundings of values of at most 1 (after the
    division): max_v e_s + 3·EPS·w, second-order terms in the 8 (not 6) of e_s."""
    return vol64.s_bound + 3.0 * EPS * vol64.weight


def agreement(a, b):
    """Samples at which two evaluations of the same views took the same decision at the same pixel, every view."""
    same = np.ones(a.tsdf.shape, bool)
    for (ok_a, iu_a, iv_a), (ok_b, iu_b, iv_b) in zip(a.views, b.views):
        same &= (ok_a == ok_b) & (~ok_a | ((iu_a == iu_b) & (iv_a == iv_b)))
    return same


# ---- extraction ----
def _corner(a, dx, dy, dz):
    nz, ny, nx = a.shape[:3]
    return a[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1]


_CORNERS = [(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)]


def active_cells(tsdf, weight):
    """(nz-1, ny-1, nx-1) bool: the cells with a vertex — all 8 corners observed, not all on one side.  Vertex ids count the
    True entries in C order."""
    inside, obs = np.asarray(tsdf) < 0, np.asarray(weight) > 0
    all_obs = np.logical_and.reduce([_corner(obs, *c) for c in _CORNERS])
    n_in = np.sum([_corner(inside, *c) for c in _CORNERS], 0)
    return all_obs & (n_in > 0) & (n_in < 8)


def extract(tsdf, weight, color, origin, h, dtype=f32):
    """gsr_mesh_count + gsr_mesh_emit -> Mesh(vertices (M, 3), faces (F, 3) int32, colors (M, 3) | None, M, quads)."""
    T = dtype
    tsdf, weight = np.asarray(tsdf).astype(T), np.asarray(weight).astype(T)
    nz, ny, nx = tsdf.shape
    empty = Mesh(np.zeros((0, 3), T), np.zeros((0, 3), np.int32), None if color is None else np.zeros((0, 3), T), 0, 0)
    if min(nx, ny, nz) < 2:
        return empty
    o, h = np.asarray(origin, f32).astype(T), T(f32(h))
    inside, obs = tsdf < 0, weight > 0
    corners = _CORNERS
    active = active_cells(tsdf, weight)                                         # (nz-1, ny-1, nx-1)
    M = int(active.sum())
    vid = np.full(active.shape, -1, np.int64)
    vid[active] = np.arange(M)                                                  # ascending i + (nx-1)·(j + (ny-1)·k)
    # vertices: the crossing points of the 4 x-edges, then y, then z; the two fixed coordinates count up, the lower axis fastest
    s = [np.zeros(active.shape, T) for _ in range(3)]
    n = np.zeros(active.shape, np.int32)
    with np.errstate(all="ignore"):
        for axis in range(3):
            for e in range(4):
                lo, hi = e & 1, e >> 1
                a = [(0, lo, hi), (lo, 0, hi), (lo, hi, 0)][axis]
                b = tuple(a[d] + (1 if d == axis else 0) for d in range(3))
                Ta, Tb = _corner(tsdf, *a), _corner(tsdf, *b)
                cross = (Ta < 0) != (Tb < 0)
                t = Ta / (Ta - Tb)
                for d in range(3):
                    add = t if d == axis else T(a[d])
                    s[d] = np.where(cross, s[d] + add, s[d])
                n += cross
        kk, jj, ii = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
        fn = n.astype(T)
        verts = np.stack([o[d] + h * (idx.astype(T) + s[d] / fn) for d, idx in enumerate((ii, jj, kk))], -1)[active].astype(T)
    colors = None
    if color is not None:
        col = np.asarray(color).astype(T)
        acc = _corner(col, *corners[0])
        for c in corners[1:]:
            acc = acc + _corner(col, *c)
        colors = (acc * T(0.125))[active].astype(T)
    # quads: edge p -> p + e_a, ascending 3·l(p) + a.  p is a cell (p + e_a is a sample and c2 = p exists)
    masks = np.zeros(active.shape + (3,), bool)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        e = [0, 0, 0]
        e[a] = 1
        m = _corner(obs, 0, 0, 0) & _corner(obs, *e) & (_corner(inside, 0, 0, 0) != _corner(inside, *e))
        idx = (ii, jj, kk)
        m = m & (idx[b] >= 1) & (idx[c] >= 1)
        cells = []
        for n_ in range(4):      # c0 = p - e_b - e_c, c1 = p - e_c, c2 = p, c3 = p - e_b
            sh = [0, 0, 0]
            if n_ in (0, 3):
                sh[b] = -1
            if n_ in (0, 1):
                sh[c] = -1
            cells.append(sh)
            m = m & np.roll(active, tuple(-x for x in sh[::-1]), (0, 1, 2))     # rolled-in cells are masked by idx >= 1
        masks[..., a] = m
    K, J, I, Aa = np.nonzero(masks)                                             # C order: ascending (k, j, i, a)
    faces = np.zeros((2 * len(K), 3), np.int32)
    for q, (k, j, i, a) in enumerate(zip(K, J, I, Aa)):
        b, c = (a + 1) % 3, (a + 2) % 3
        v = []
        for n_ in range(4):
            p = [i, j, k]
            if n_ in (0, 3):
                p[b] -= 1
            if n_ in (0, 1):
                p[c] -= 1
            v.append(vid[p[2], p[1], p[0]])
        assert min(v) >= 0
        if not _corner(inside, 0, 0, 0)[k, j, i]:
            v = v[::-1]
        faces[2 * q], faces[2 * q + 1] = (v[0], v[1], v[2]), (v[0], v[2], v[3])
    return Mesh(verts, faces, colors, M, len(K))


def extract_volume(vol, dtype=None):
    return extract(vol.tsdf, vol.weight, vol.color, vol.origin, vol.h, vol.dtype if dtype is None else dtype)


# ---- the mesh conditions of the sphere scenes ----
def mesh_report(vertices, faces, h):
    """-> dict: every undirected edge in exactly two triangles, once per direction (`closed`); V - E + F (`euler`); every face
    normal away from the centre (`outward`); max | |v| - 1 | / h (`radius_h`)."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    directed = collections.Counter()
    for a, b, c in f:
        for e in ((a, b), (b, c), (c, a)):
            directed[e] += 1
    undirected = {tuple(sorted(e)) for e in directed}
    closed = all(n == 1 for n in directed.values()) and all(directed.get((b, a), 0) == 1 for (a, b) in directed)
    nrm = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    cen = v[f].mean(1)
    return dict(closed=closed, euler=len(v) - len(undirected) + len(f), outward=bool(((nrm * cen).sum(1) > 0).all()),
                radius_h=float(np.abs(np.linalg.norm(v, axis=1) - 1.0).max() / float(h)), used=len(np.unique(f)) == len(v))


# ---- the analytic scene: the unit sphere at the origin seen by 14 cameras ----
SPHERE_W, SPHERE_H, SPHERE_F = 128, 96, 120.0
SPHERE_CASES = {"A": (17, 2.0), "B": (24, 3.0)}       # n, trunc / h


def sphere_cameras():
    centres = [(4, 0, 0), (-4, 0, 0), (0, 4, 0), (0, -4, 0), (0, 0, 4), (0, 0, -4)]
    centres += [(2.3 * a, 2.3 * b, 2.3 * c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    cams = []
    for c in centres:
        c = np.asarray(c, np.float64)
        z = -c / np.linalg.norm(c)
        up = np.array([0.0, 1.0, 0.0]) if abs(z[2]) >= 0.9 else np.array([0.0, 0.0, 1.0])
        x = np.cross(up, z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        cams.append(Cam(SPHERE_W, SPHERE_H, (SPHERE_F, SPHERE_F), (0.5, 0.5), R.astype(f32), (-R @ c).astype(f32)))
    return cams


def sphere_frame(cam, channels=5):
    """(H, W, channels) fp32: alpha = 1 where the pixel's ray ((i - cx)/fx, (j - cy)/fy, 1) hits the sphere, D the z-depth of the
    first hit, rgb = 0.5 + 0.5·(the world normal there); zeros elsewhere."""
    W, H = cam.width, cam.height
    R, t = np.asarray(cam.R, np.float64), np.asarray(cam.t, np.float64)
    cx, cy = cam.principal[0] * W, cam.principal[1] * H
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    d = np.stack([(ii - cx) / cam.focal[0], (jj - cy) / cam.focal[1], np.ones((H, W))], -1)
    dd, dt = (d * d).sum(-1), d @ t                      # |s·d - t|² = 1: the sphere's centre is t in camera coordinates
    disc = dt * dt - dd * (t @ t - 1.0)
    hit = disc > 0
    s = (dt - np.sqrt(np.where(hit, disc, 0.0))) / dd
    normal = (s[..., None] * d - t) @ R                  # world = Rᵀ (pc - t), row-vector form
    img = np.zeros((H, W, channels), f32)
    img[..., 0:3] = np.where(hit[..., None], 0.5 + 0.5 * normal, 0.0)
    img[..., 3] = np.where(hit, s, 0.0)
    img[..., 4] = hit
    return img


def sphere_volume(case, color=False, dtype=f32):
    n, k = SPHERE_CASES[case]
    h = f32(2.6 / (n - 1))
    return Volume((n, n + 1, n + 2), (-1.3, -1.3, -1.3), h, f32(k) * h, color, dtype)


_sphere = {}


def sphere_fused(case, color=False, dtype=f32, n_views=14):
    """The volume of `case` after its first `n_views` views; computed once per argument set, treat as read-only."""
    key = (case, color, dtype, n_views)
    if key not in _sphere:
        vol = sphere_volume(case, color, dtype)
        for cam in sphere_cameras()[:n_views]:
            integrate(vol, sphere_frame(cam), cam)
        _sphere[key] = vol
    return _sphere[key]


# ---- random frames, cameras and volumes ----
RANDOM_DIMS = [(2, 2, 2), (1, 5, 3), (65, 3, 2), (41, 13, 11)]
EDGE_W, EDGE_H = 64, 32


def random_frame(seed, W, H, C=5):
    """A frame with alpha = 0 (10 %), 0 < alpha < MIN_ALPHA (10 %), NaN alpha (2 %), NaN depths (3 %), negative depths (5 %),
    NaN and out-of-range colours; premultiplied like the rasterizer's."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.3, 1.0, (H, W))
    r = rng.uniform(0, 1, (H, W))
    alpha[r < 0.10] = 0.0
    alpha[(r >= 0.10) & (r < 0.20)] = 5e-4
    alpha[(r >= 0.20) & (r < 0.22)] = np.nan
    depth = rng.uniform(0.3, 3.0, (H, W))
    r = rng.uniform(0, 1, (H, W))
    depth[r < 0.03] = np.nan
    depth[(r >= 0.03) & (r < 0.08)] *= -1.0
    img = np.zeros((H, W, C), f32)
    rgb = rng.uniform(-0.3, 1.4, (H, W, 3))
    rgb[rng.uniform(0, 1, (H, W, 3)) < 0.02] = np.nan
    img[..., :3] = rgb * np.nan_to_num(alpha)[..., None]
    img[..., 3] = depth * np.nan_to_num(alpha)
    img[..., 4] = alpha
    if C > 5:
        img[..., 5:] = rng.standard_normal((H, W, C - 5))
    return img


def edge_setup(dims):
    """A volume and an axis-aligned camera in exact binary fractions: h = 1/16, origin (-2, -1, z0), R = I, fx = fy = 32,
    (cx, cy) = (31.5, 15.5) on a 64 x 32 frame, and z = 2 exactly on the plane k = 1, where u = i - 0.5 and v = j - 0.5: i = 0 and
    j = 0 project EXACTLY onto the frame's low edge (u + 0.5 = 0: inside), i = 64 exactly onto its high edge (u + 0.5 = W:
    outside).  The plane k = 0 has z = 1.9375."""
    cam = Cam(EDGE_W, EDGE_H, (32.0, 32.0), (31.5 / 64.0, 15.5 / 32.0), np.eye(3, dtype=f32), np.array([0, 0, 3.0], f32))
    return Volume(dims, (-2.0, -1.0, -1.0625), 1.0 / 16.0, 4.0 / 16.0), cam


def oblique_camera(seed, W, H, vol):
    """A camera INSIDE the volume's box, looking along a random direction: part of the samples are behind it, part project
    outside the frame."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = vol.dims
    ext = np.array([nx - 1, ny - 1, nz - 1]) * float(vol.h)
    c = vol.origin.astype(np.float64) + ext * rng.uniform(0.3, 0.7, 3)
    z = rng.standard_normal(3)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0] if abs(z[2]) < 0.9 else [0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    c = c - 0.6 * z                                  # step back: the nearer samples are in front of it beyond `near`
    return Cam(W, H, (0.9 * W, 0.8 * W), (0.47, 0.55), R.astype(f32), (-R @ c).astype(f32))


def random_views(dims, color=False):
    """-> (fresh fp32 volume, [(frame, camera)] x 3): the exact-edge camera and two oblique ones, on random frames."""
    vol, cam = edge_setup(dims)
    vol = Volume(dims, vol.origin, vol.h, vol.trunc, color)
    seed = 1000 * dims[0] + 10 * dims[1] + dims[2]
    views = [(random_frame(seed, EDGE_W, EDGE_H), cam)]
    for v in (1, 2):
        views.append((random_frame(seed + v, 48, 40, 5 + 3 * (v - 1)), oblique_camera(seed + v, 48, 40, vol)))
    return vol, views


WIDE_DIMS = [(257, 3, 2), (300, 4, 3), (513, 5, 3), (770, 3, 2)]      # more than one 256-sample block of the integration in x
WIDE_W, WIDE_H = 512, 32
WIDE_POSES = ((+1, 1.0, 0.5), (-1, 1.5, -0.5), (+1, 0.7, 1.0), (-1, 1.2, 0.75), (+1, 0.9, -1.0))     # side, distance, turn in degrees
# the first seed offset with which the case meets the conditions of tests/test_tsdf_cpu.py: with 0 no sample of the low edge
# i = 0 of plane k = 1 is fused ((257, 3, 2), (770, 3, 2)), two of the 15 samples of column 512 meet a usable pixel in no view
WIDE_RESEED = {(257, 3, 2): 100, (513, 5, 3): 100, (770, 3, 2): 100}


def wide_camera(vol, side, dist, turn, W=WIDE_W, H=WIDE_H):
    """A camera `dist` in front of the box's long face, looking across it (side = +1: along +z from below, -1: along -z from
    above), turned `turn` degrees about its axis, with a focal length so short that the whole length of the box projects into
    the frame: every sample is dist .. dist + 0.2 deep, within the truncation of most of random_frame's depths (0.3 .. 3.0) —
    the oblique cameras of random_views see 3.25 deep at most, 52 samples of x."""
    nx, ny, nz = vol.dims
    ext = np.array([nx - 1, ny - 1, nz - 1]) * float(vol.h)
    c = vol.origin.astype(np.float64) + 0.5 * ext
    c[2] = float(vol.origin[2]) + (-dist if side > 0 else ext[2] + dist)
    a = math.radians(turn)
    z = np.array([0.0, 0.0, float(side)])
    x = np.array([math.cos(a), math.sin(a), 0.0])
    R = np.stack([x, np.cross(z, x), z])
    fx = 0.46 * W * dist / (0.5 * ext[0])          # the ends of the box at 0.46·W from the centre at depth `dist`
    return Cam(W, H, (fx, 12.0), (0.5, 0.45), R.astype(f32), (-R @ c).astype(f32))


def wide_views(dims, color=False):
    """-> (fresh fp32 volume, [(frame, camera)] x 7) for a volume longer than 256 samples in x: the exact-edge camera of
    edge_setup (binary fractions; it sees i < 64), an oblique camera inside the box, and the five wide_cameras of WIDE_POSES,
    which reach every 256-block of x; random frames with all their populations, one of them with 8 channels."""
    vol, cam = edge_setup(dims)
    vol = Volume(dims, vol.origin, vol.h, vol.trunc, color)
    seed = 1000 * dims[0] + 10 * dims[1] + dims[2] + WIDE_RESEED.get(tuple(dims), 0)
    views = [(random_frame(seed, EDGE_W, EDGE_H), cam),
             (random_frame(seed + 1, 48, 40), oblique_camera(seed + 1, 48, 40, vol))]
    for n, pose in enumerate(WIDE_POSES):
        views.append((random_frame(seed + 2 + n, WIDE_W, WIDE_H, 8 if n == 0 else 5), wide_camera(vol, *pose)))
    return vol, views


def random_volume(dims, seed, color=True, p_zero=0.3):
    """tsdf uniform in [-1, 1], 30 % of the weights zero: ambiguous faces, missing cells, every edge case of the indexing
    (at 30 % one cell in 17 is active and quads are rare; p_zero = 0.05 gives the dense counterpart)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    vol = Volume(dims, (-0.7, 0.3, 1.1), 0.173, 0.5, color)
    vol.tsdf = rng.uniform(-1, 1, (nz, ny, nx)).astype(f32)
    vol.weight = np.where(rng.uniform(0, 1, (nz, ny, nx)) < p_zero, 0.0, rng.integers(1, 9, (nz, ny, nx))).astype(f32)
    if color:
        vol.color = rng.uniform(0, 1, (nz, ny, nx, 3)).astype(f32)
    return vol


# ---- the extraction's plan, restated, and the volumes that take it past one run, one workgroup, one scan round ----
MESH_RUN_CELLS, SCAN_ROUND = 2048, 1024


def mesh_plan(dims):
    """-> (rows, nruns, nblk, ncells): a wave walks a run of `rows` whole x-rows of cells of one slab k, `nruns` runs per slab,
    `nblk` runs in all (the length of the scan)."""
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) < 2:
        return 1, 0, 0, 0
    rows = max(1, MESH_RUN_CELLS // (nx - 1))
    nruns = (ny - 1 + rows - 1) // rows
    return rows, nruns, nruns * (nz - 1), (nx - 1) * (ny - 1) * (nz - 1)


def run_of(dims, j, k):
    """The index of the run of cell row (j, k) in the per-run words; j and k may be arrays."""
    rows, nruns, _, _ = mesh_plan(dims)
    return j // rows + nruns * k


def mesh_scratch_bytes(dims):
    """gsr_mesh_scratch_bytes: one 4-byte word per cell, one 8-byte word per run and the 8-byte total."""
    _, _, nblk, ncells = mesh_plan(dims)
    return 4 * ncells + 8 * (nblk + 1) if ncells else 0


MultiRun = collections.namedtuple("MultiRun", "dims seed p_zero color plan")      # plan = (rows, nruns, nblk)
MULTI_RUN_CASES = (
    MultiRun((64, 5, 3), 21, 0.05, True, (32, 1, 2)),          # nx - 1 = 63: the cells fill one step, lane 63 carries the last column
    MultiRun((65, 5, 3), 22, 0.05, True, (32, 1, 2)),          # 64: the second step holds one cell
    MultiRun((127, 4, 3), 23, 0.05, True, (16, 1, 2)),         # 126: two full steps
    MultiRun((130, 40, 5), 24, 0.05, True, (15, 3, 12)),       # three waves live, the fourth leaves; the last run has 9 rows of 15
    MultiRun((513, 12, 4), 25, 0.05, True, (4, 3, 9)),         # the last run has 3 rows of 4
    MultiRun((1025, 7, 3), 26, 0.05, False, (2, 3, 6)),        # nx - 1 = 1024: the last width with rows = 2; no colour
    MultiRun((1026, 10, 3), 27, 0.05, True, (1, 9, 18)),       # rows = 1; three workgroups, the last with one live wave
    MultiRun((2050, 4, 3), 28, 0.05, True, (1, 3, 6)),         # nx - 1 > 2048: the clamp of rows
    MultiRun((1026, 42, 26), 29, 0.3, True, (1, 41, 1025)),    # nblk = 1024 + 1: a second scan round, the carry into one entry
)
_multi = {}


def multi_run_name(case):
    return f"multi-run {case.dims}" + ("" if case.color else ", no colour")


def multi_run(case):
    """-> (volume, its fp32 mesh) of a MULTI_RUN_CASES entry; computed once, treat as read-only."""
    if case.dims not in _multi:
        vol = random_volume(case.dims, case.seed, case.color, case.p_zero)
        _multi[case.dims] = vol, extract_volume(vol)
    return _multi[case.dims]


def vertex_runs(vol):
    """-> (run, slab, j) per vertex of `vol`'s mesh, in vertex order: the run id (run_of), the slab k and the cell row j."""
    K, J, _ = np.nonzero(active_cells(vol.tsdf, vol.weight))
    return run_of(vol.dims, J, K), K, J


def one_cell_volume():
    """(2, 2, 2): one active cell (one corner inside), a vertex and no face."""
    vol = Volume((2, 2, 2), (0.0, 0.0, 0.0), 0.5, 1.0, True)
    vol.weight[:] = 1
    vol.tsdf[:] = f32(0.75)
    vol.tsdf[0, 0, 0] = f32(-0.25)
    vol.color = np.random.default_rng(5).uniform(0, 1, (2, 2, 2, 3)).astype(f32)
    return vol


# ---- PLY ----
def quantize8(x):
    """frame_rgb8's quantiser rule: floor(clamp(x, 0, 1)·255 + 0.5), every step one fp32 operation."""
    x = np.asarray(x, f32)
    return np.floor(np.fmin(np.fmax(x, f32(0)), f32(1)) * f32(255) + f32(0.5)).astype(np.uint8)


def parse_ply(data):
    """Binary little-endian PLY bytes of `mesh_ply_bytes` -> (vertices (M, 3) f32, colors (M, 3) u8 | None, faces (F, 3) i32)."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    elements, props = [], {}
    for line in head[2:]:
        w = line.split()
        if w[:1] == ["element"]:
            elements.append((w[1], int(w[2])))
            props[w[1]] = []
        elif w[:1] == ["property"]:
            props[elements[-1][0]].append(w[1:])
    assert [e[0] for e in elements] == ["vertex", "face"]
    M, F = elements[0][1], elements[1][1]
    has_color = len(props["vertex"]) == 6
    assert props["vertex"][:3] == [["float", "x"], ["float", "y"], ["float", "z"]]
    if has_color:
        assert props["vertex"][3:] == [["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    assert props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    vdt = np.dtype([("p", "<f4", 3)] + ([("c", "u1", 3)] if has_color else []))
    fdt = np.dtype([("n", "u1"), ("v", "<i4", 3)])
    assert len(data) == end + M * vdt.itemsize + F * fdt.itemsize
    vert = np.frombuffer(data, vdt, M, end)
    face = np.frombuffer(data, fdt, F, end + M * vdt.itemsize)
    assert (face["n"] == 3).all()
    return vert["p"].copy(), (vert["c"].copy() if has_color else None), face["v"].copy()
