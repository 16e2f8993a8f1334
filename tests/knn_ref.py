"""numpy reference of the point-cloud initialisation (csrc/knn.hip, gsr_knn_scales): brute force over all pairs, chunked,
with the kernel's fp32 expressions exactly — d2 = (dx*dx + dy*dy) + dz*dz, self excluded by index —, a float64 twin of the
whole formula as the tolerance yardstick, and the point-cloud families the tests run.  No product code, no GPU."""
import functools

import numpy as np

f32 = np.float32
SIZES = (4, 5, 63, 64, 65, 129, 257, 1031, 4099)   # the minimum; both sides of the 64-point group; several blocks
FAMILIES = ("uniform", "blob_outliers", "identical", "duplicated", "planar", "collinear", "lattice")


def dist2_three(points, dtype=np.float32, chunk=512):
    """(n, 3): the three smallest d2(i, j), j != i, ascending, in `dtype` arithmetic."""
    p = np.ascontiguousarray(points, dtype)
    n = p.shape[0]
    assert n >= 4
    out = np.empty((n, 3), dtype)
    for a in range(0, n, chunk):
        q = p[a:a + chunk]
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == dtype
        r = np.arange(q.shape[0])
        d2[r, a + r] = np.inf                      # by index: a duplicate at distance 0 stays a neighbour
        out[a:a + chunk] = np.sort(np.partition(d2, 2, axis=1)[:, :3], axis=1)
    return out


def scales_from_dist2(d2, point_size=1.0, isotropic=False, dtype=np.float32):
    """dataset.jl:245-246 on the tree's distances: q = sqrt(d2)·sqrt(d2); md = ((q0 + q1) + q2) / 3;
    s = log(sqrt(max(1f-7, md) · point_size)); all three columns, or their mean ((s + s) + s) / 3."""
    t = dtype
    d2 = np.asarray(d2, t)
    q = np.sqrt(d2) * np.sqrt(d2)
    md = ((q[:, 0] + q[:, 1]) + q[:, 2]) / t(3)
    s = np.log(np.sqrt(np.maximum(t(f32(1e-7)), md) * t(f32(point_size))))
    assert s.dtype == t
    if isotropic:
        return (((s + s) + s) / t(3))[:, None]
    return np.repeat(s[:, None], 3, 1)


def knn_ref(points, point_size=1.0, isotropic=False):
    """(scales, dist2) in fp32, as the kernel computes them (log / sqrt are numpy's: equal up to ulps)."""
    d2 = dist2_three(points, np.float32)
    return scales_from_dist2(d2, point_size, isotropic, np.float32), d2


def knn_ref64(points, point_size=1.0, isotropic=False):
    """The float64 twin: the same fp32 coordinates, every operation in float64."""
    d2 = dist2_three(points, np.float64)
    return scales_from_dist2(d2, point_size, isotropic, np.float64), d2


def scale_tolerance(s64):
    """|Δ| <= 1e-5 · max(1, |s|): md carries about 6 fp32 roundings, through ½·log that is <= 4e-7; logf adds 1-2 ulp of a
    value with |s| <~ 16; together <= 2e-6; the bound is that with a 5x margin."""
    return 1e-5 * np.maximum(1.0, np.abs(s64))


@functools.lru_cache(maxsize=None)
def make_points(family, n, seed=0):
    """(n, 3) float32, read-only.  Deterministic in (family, n, seed)."""
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + 7 * n + seed)
    if family == "uniform":
        p = rng.random((n, 3))
    elif family == "blob_outliers":   # a dense blob and a few points 1e4 times farther out
        p = rng.normal(0.0, 1.0, (n, 3))
        k = max(1, n // 16)
        d = rng.normal(0.0, 1.0, (k, 3))
        p[rng.choice(n, k, replace=False)] = 1e4 * d / np.linalg.norm(d, axis=1, keepdims=True)
    elif family == "identical":
        p = np.tile(np.array([[0.3, -1.2, 2.5]]), (n, 1))
    elif family == "duplicated":      # every point twice (n odd: one of them once), shuffled
        u = rng.random(((n + 1) // 2, 3))
        p = np.concatenate([u, u])[:n][rng.permutation(n)]
    elif family == "planar":
        p = rng.random((n, 3))
        p[:, 2] = 0.75
    elif family == "collinear":
        t = rng.random((n, 1)) * 10.0
        p = np.array([[0.5, -0.25, 1.0]]) + t * np.array([[0.6, 0.48, 0.64]])
    elif family == "lattice":         # integer coordinates: many exact ties
        m = int(np.ceil(n ** (1.0 / 3.0))) + 1
        g = np.stack(np.meshgrid(*([np.arange(m)] * 3), indexing="ij"), -1).reshape(-1, 3)
        p = g[rng.permutation(g.shape[0])[:n]].astype(np.float64)
    else:
        raise ValueError(family)
    p = np.ascontiguousarray(p, np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference(family, n, seed=0):
    """(dist2 fp32, scales float64 twin (n,3), isotropic float64 twin (n,1)) of make_points(family, n, seed): computed once,
    shared by the tests, read-only."""
    p = make_points(family, n, seed)
    d2 = dist2_three(p, np.float32)
    s64, _ = knn_ref64(p)
    out = (d2, s64, s64[:, :1].copy())
    for a in out:
        a.setflags(write=False)
    return out
