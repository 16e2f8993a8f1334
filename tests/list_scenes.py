"""One-tile scenes whose tile list has a CHOSEN length and a chosen last contributor.

A 16 x 16 image is one tile; in reference-list mode every visible Gaussian is exactly one instance of it, so the length of the
list is the number of Gaussians and the sorted position of a Gaussian is the rank of its depth.  The builders place lengths on
the edges at which the sort, the fused forward, the two backward kernels and the key bins change code path (BOUNDARIES), and
decide where the walk of the list ends: at its last entry (single_tile_scene) or at a chosen position (walled_scene).
Pure functions of (L, seed): numpy + the plain Camera dataclass, no oracle / product compute."""
import math
from dataclasses import dataclass

import numpy as np

from oracle.oracle import Camera

SH0 = 0.28209479177387814

# List lengths b at which a kernel changes path: position b - 1 is the last entry of one class, b the first of the next.
#   64 .. 1024        one-wave sort, 1 / 2 / 4 / 8 / 16 keys per lane (tile_sort_device.h wave_sort_ids_any); 64-entry batches of
#                     the one-wave backward; 256-entry LDS chunks of the fused forward (256, 512, 768, 1024); the fused launch's cut
#   2048 .. 8192      register runs of the LDS sorts, RUNS = 4 ((1024, 4096]: 2048, 3072, 4096) and RUNS = 8 ((4096, 8192]: 6144,
#                     8192); tile_last = 2048: 32 full segments of 64 of composite_bwd_long_kernel, which on a one-tile view takes every
#                     list beyond 1024 (split_len = 1024: gsr_policy_bwd_split cuts at the lowest tier while the tiles are few)
#   12288 .. 65536    8192-key chunks merged in 4096-key blocks: 1, 2, 3 merge passes from 8193, 16385, 32769 keys; 65536: the
#                     first length whose positions need more than 16 bits
BOUNDARIES = (64, 128, 256, 512, 768, 1024, 2048, 3072, 4096, 6144, 8192, 12288, 16384, 32768, 65536)

# The cases of tests/test_gpu_list_boundaries.py; tests/test_list_scenes_cpu.py holds the builders' conditions on the oracle for each.
FULL_WALK_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 2047, 2048,
                     2049, 3072, 3073, 4095, 4096, 4097, 6144, 6145, 8191, 8192, 8193, 12288, 12289, 16383, 16384, 16385, 32768,
                     32769, 65535, 65536, 65537)
MODE_LENGTHS = (64, 65, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16385)
# (L, stop): 2 500 and 9 000 entries are composite_bwd_long_kernel's on a default handle; 1 000 stay with the one-wave kernel
_STOPS = (2, 64, 65, 1024, 1025, 2048, 2049)
EARLY_STOPS = (tuple((1000, s) for s in (2, 64, 65, 512)) + tuple((2500, s) for s in _STOPS)
               + tuple((9000, s) for s in _STOPS + (4097,)))
# First views of L1 entries on a fresh handle and the bin capacity gsr_policy_begin_view estimates from them (8 N / T + 64, rounded
# up to 64): one tile, and two tiles with TWO_TILE_SECOND entries in the second.  The GPU test reads the capacity from gsr_stats.
BIN_FIRST_VIEWS = {100: 896, 1000: 8064}
TWO_TILE_SECOND = 10
TWO_TILE_FIRST_VIEWS = {100: 512, 1000: 4160}


@dataclass
class ListScene:
    means: np.ndarray
    shs: np.ndarray
    opac: np.ndarray
    scales: np.ndarray      # activated
    rots: np.ndarray
    cam: Camera
    deg: int
    order: np.ndarray       # order[p] = Gaussian id at sorted position p, by construction (list_positions reads it back from a run)
    walls: tuple = ()       # sorted positions of the full-tile splats (walled_scene)
    ties: int = 0           # adjacent list entries with equal depth bits (tied_tile_scene)
    lengths: tuple = ()     # list length per tile, row-major (many_tile_scene)

    @property
    def args(self):
        return self.means, self.shs, self.opac, self.scales, self.rots


def boundary_positions(L, stop=None, slack=0):
    """Sorted positions within 2 of a boundary <= L (and of `stop`), plus the first and the last of the list.
    slack = s: the positions that can END within 2 of a boundary, first or last once up to s entries of the list are dropped
    (an entry at p moves to p - s .. p): each window reaches s positions further back, the last entry's s further to the front."""
    edges = [b for b in BOUNDARIES if b <= L] + ([stop] if stop is not None else [])
    P = set(range(0, slack + 1)) | set(range(L - 1 - slack, L))
    for b in edges:
        P.update(range(b - 2, b + 3 + slack))
    return np.array(sorted(p for p in P if 0 <= p < L), np.int64)


def front_parameters(L):
    """(sigma in px, base opacity) of the faint front splats: the walk of the whole list, backdrop included, ends with
    final T >= 3e-4 at every pixel for every L <= 65537 (asserted on the oracle by tests/test_list_scenes_cpu.py; measured
    minimum 5.7e-3 at 4097, 2.0e-3 at 16385, 4.3e-4 at 65536).  Longer lists need a thinner front still."""
    if L <= 4097:
        return 1.5, 0.008
    if L <= 16385:
        return 1.1, 0.006
    return 1.05, 0.0042


def _camera(W=16, H=16):
    f = np.float32(8.0 / math.tan(math.radians(30.0)))
    return Camera(W, H, (f, f))


def _front(rng, n, depths, sigma_px, base_opacity, fx, pinned, deg, lo=(1.5, 1.5), hi=(14.5, 14.5), cx=8.0, cy=8.0):
    """n faint, near-isotropic splats at the given depths, projected centres uniform in [lo, hi] px.  `pinned` (bool, n): these get
    the top of the opacity range and a centre within 0.15 px of a pixel centre, so that they blend somewhere (alpha >= 1.4 / 255 at
    that pixel for every (sigma, opacity) of front_parameters) and their gradient rows carry signal."""
    u = rng.uniform(lo[0], hi[0], n)
    v = rng.uniform(lo[1], hi[1], n)
    ju, jv = rng.uniform(-0.15, 0.15, n), rng.uniform(-0.15, 0.15, n)
    # (lo, hi, cx, cy: scalars, or one value per splat — many_tile_scene)
    u = np.where(pinned, np.clip(np.round(u), np.ceil(lo[0]), np.floor(hi[0])) + ju, u)
    v = np.where(pinned, np.clip(np.round(v), np.ceil(lo[1]), np.floor(hi[1])) + jv, v)
    means = np.stack([(u - cx) * depths / fx, (v - cy) * depths / fx, depths], 1)
    scales = (sigma_px * depths / fx)[:, None] * rng.uniform(0.8, 1.25, (n, 3))
    rots = rng.standard_normal((n, 4))
    opac = base_opacity * np.where(pinned, 1.5, rng.uniform(1.0, 1.5, n))
    K = (deg + 1) ** 2
    shs = np.zeros((n, K, 3))
    shs[:, 0] = rng.normal(0.0, 0.5, (n, 3))
    if K > 1:
        shs[:, 1:] = rng.normal(0.0, 0.1, (n, K - 1, 3))
    return means, shs, opac, scales, rots


def _full_tile(depth, sigma_px, fx, colour, deg, centre=(7.5, 7.5), cx=8.0, cy=8.0):
    s = sigma_px * depth / fx
    mean = np.array([(centre[0] - cx) * depth / fx, (centre[1] - cy) * depth / fx, depth])
    shs = np.zeros(((deg + 1) ** 2, 3))
    shs[0] = (np.asarray(colour) - 0.5) / SH0
    # (not a sphere: an isotropic splat has an identically zero rotation gradient, and a list of one entry nothing else)
    return mean, shs, s * np.array([1.0, 0.9, 1.1]), np.array([0.9, 0.1, -0.2, 0.3])


def _unique_depths(rng, n, lo=2.0, hi=8.0):
    """n ascending depths in [lo, hi] that stay distinct in float32 (70 000 of them are 8.6e-5 apart; one ulp at 8 is 4.8e-7)."""
    step = (hi - lo) / max(n, 1)
    d = (lo + step * (np.arange(n) + rng.uniform(0.1, 0.9, n))).astype(np.float32)
    assert n < 2 or (np.diff(d) > 0).all()
    return d.astype(np.float64)


def _pack(parts, order, cam, deg, walls=()):
    """parts: per-position arrays (position-major).  Scatter them to Gaussian ids: Gaussian order[p] sits at position p."""
    out = []
    for a in parts:
        a = np.asarray(a, np.float32)
        b = np.empty_like(a)
        b[order] = a
        out.append(b)
    return ListScene(*out, cam, deg, order, tuple(walls))


def single_tile_scene(L, seed, deg=0):
    """A list of exactly L entries that every pixel walks to its END: L - 1 faint front splats at distinct depths in [2, 8] and one
    "backdrop" — the last id, depth 9, sigma 40 px, opacity 0.9 — which is the deepest key, sits at position L - 1 and blends at every
    pixel.  So n_rendered == n_visible == L, n_contrib == L at every pixel, and with front_parameters(L) the final transmittance
    stays >= 3e-4: no saturation decision is closer than a factor 3 to its threshold.  The Gaussians at boundary_positions(L)
    are pinned onto a pixel centre (see _front): one wrong visit there moves a gradient row that is not zero."""
    rng = np.random.default_rng([int(seed), int(L)])
    cam = _camera()
    fx = float(cam.focal[0])
    sigma_px, base = front_parameters(L)
    n = L - 1
    pinned = np.zeros(n, bool)
    P = boundary_positions(L)
    pinned[P[P < n]] = True
    means, shs, opac, scales, rots = _front(rng, n, _unique_depths(rng, n), sigma_px, base, fx, pinned, deg)
    bm, bs, bsc, br = _full_tile(9.0, 40.0, fx, (0.8, 0.3, 0.6), deg)
    parts = [np.concatenate([means, bm[None]]), np.concatenate([shs, bs[None]]), np.concatenate([opac, [0.9]]),
             np.concatenate([scales, bsc[None]]), np.concatenate([rots, br[None]])]
    order = np.concatenate([rng.permutation(n), [n]]).astype(np.int64)   # ids are not positions; the backdrop is the last id
    return _pack(parts, order, cam, deg)


def walled_scene(L, stop, seed, deg=0):
    """A list of L entries whose walk ends after exactly `stop` of them at every pixel.  Full-tile "walls" (opacity 0.97, sigma
    160 px: alpha >= 0.965 at every pixel centre, so each multiplies T by at most 0.035) sit at the sorted positions stop - 2,
    stop - 1 AND stop; everything else is a faint front splat.  With T_a >= 0.25 ahead of them, the second wall still blends
    (T_a · 0.03² >= 2.2e-4, a factor 2 above the 1e-4 threshold) and the third one is the next entry whose blend test is
    evaluated: it sees T_a · 0.035³ <= 4.3e-5, a factor 2 below — the walk stops there at every pixel, n_contrib == stop, and
    no entry at a position >= stop receives a gradient.  (Two walls alone leave T ≈ 9e-4 · T_a, which no faint splat behind
    them brings under 1e-4: the entry that ends the walk has to be opaque itself.)"""
    assert 2 <= stop < L
    rng = np.random.default_rng([int(seed), int(L), int(stop)])
    cam = _camera()
    fx = float(cam.focal[0])
    depths = _unique_depths(rng, L)
    walls = (stop - 2, stop - 1, stop)
    is_wall = np.zeros(L, bool)
    is_wall[list(walls)] = True
    front_pos = np.flatnonzero(~is_wall)
    pinned = np.isin(front_pos, boundary_positions(L, stop))
    # (the thinnest front of front_parameters: 4 100 entries ahead of the walls leave T_a ≈ 0.7)
    means, shs, opac = np.zeros((L, 3)), np.zeros((L, (deg + 1) ** 2, 3)), np.zeros(L)
    scales, rots = np.zeros((L, 3)), np.zeros((L, 4))
    fm, fs, fo, fsc, fr = _front(rng, front_pos.size, depths[front_pos], 1.05, 0.0042, fx, pinned, deg)
    means[front_pos], shs[front_pos], opac[front_pos], scales[front_pos], rots[front_pos] = fm, fs, fo, fsc, fr
    for k, p in enumerate(walls):
        means[p], shs[p], scales[p], rots[p] = _full_tile(depths[p], 160.0, fx, ((0.9, 0.2, 0.4), (0.1, 0.7, 0.5), (0.5, 0.5, 0.9))[k], deg)
        opac[p] = 0.97
    # the permutation depends on (seed, L) only: two scenes of one L put Gaussian order[p] at position p whatever `stop` is, so
    # the rows between two stops belong to the same Gaussians in both
    order = np.random.default_rng([int(seed), int(L), 0xA11]).permutation(L).astype(np.int64)
    return _pack([means, shs, opac, scales, rots], order, cam, deg, walls)


def two_tile_scene(L, n_second, seed, deg=0):
    """32 x 16, two tiles: L front splats in the first, n_second in the second, every 3-sigma square (radius 5 at sigma 1.05 px)
    inside its own tile — the lists have exactly L and n_second entries and the second tile's list starts at L."""
    rng = np.random.default_rng([int(seed), int(L), int(n_second)])
    cam = _camera(32, 16)
    fx = float(cam.focal[0])
    n = L + n_second
    depths = _unique_depths(rng, n)
    second = np.zeros(n, bool)
    second[rng.choice(n, n_second, replace=False)] = True
    parts = [None] * 5
    pin = np.zeros(L, bool)
    pin[boundary_positions(L)] = True     # positions within the FIRST list; the second's ten entries all blend (opacity 0.05)
    a = _front(rng, L, depths[~second], 1.05, 0.0042, fx, pin, deg, lo=(5.5, 5.5), hi=(10.5, 10.5), cx=16.0)
    b = _front(rng, n_second, depths[second], 1.05, 0.05, fx, np.ones(n_second, bool), deg, lo=(21.5, 5.5), hi=(26.5, 10.5), cx=16.0)
    for k in range(5):
        parts[k] = np.zeros((n,) + a[k].shape[1:])
        parts[k][~second], parts[k][second] = a[k], b[k]
    sc = _pack(parts, rng.permutation(n).astype(np.int64), cam, deg)
    sc.order = np.concatenate([sc.order[~second], sc.order[second]])   # the sorted ids: tile-major, then by depth
    return sc


# List lengths of tests/test_gpu_sort_ties.py (one tile, groups 1 and 5) and the key-path cases on top of them.
TIED_LENGTHS = (2, 64, 65, 129, 257, 513, 1024, 1025, 2049, 4096, 4097, 8192, 8193, 16385, 32769)
TIED_GROUPS = (1, 5)
TIED_MODE_LENGTHS = (1024, 4097, 8193)
# tied list length -> entries of the two first views that leave bins too small for it (estimate 8 L1 + 64: 896, 1664, 8064 keys)
TIED_BIN_FIRST_VIEWS = {1024: 100, 4097: 200, 8193: 1000}


def tied_tile_scene(L, groups, seed, deg=0):
    """single_tile_scene whose front shares its depths: every front Gaussian takes one of `groups` levels float32(2 + 6 (k + 0.5) /
    groups), the level drawn per Gaussian ID, so the list order is decided by the ids wherever the depth bits are equal —
    order = lexsort((id, depth)), the reference's "ties by ascending Gaussian id".  The camera has the identity pose: the depth
    bits of a key are the bits of means[:, 2].  With every level in use the list has L - 1 - groups adjacent tied pairs
    (`ties`); groups = 1 makes the whole front ONE tie, which the sort must return as ascending ids.  Backdrop, pinned
    positions and front_parameters as in single_tile_scene."""
    rng = np.random.default_rng([int(seed), int(L), int(groups), 0x71E])
    cam = _camera()
    fx = float(cam.focal[0])
    sigma_px, base = front_parameters(L)
    n = L - 1
    level = rng.integers(0, groups, n)
    depth_of_id = (2.0 + 6.0 * (level + 0.5) / groups).astype(np.float32)
    front_order = np.lexsort((np.arange(n), depth_of_id))      # the order first, then one splat per POSITION
    pinned = np.zeros(n, bool)
    P = boundary_positions(L)
    pinned[P[P < n]] = True
    means, shs, opac, scales, rots = _front(rng, n, depth_of_id[front_order].astype(np.float64), sigma_px, base, fx, pinned, deg)
    bm, bs, bsc, br = _full_tile(9.0, 40.0, fx, (0.8, 0.3, 0.6), deg)
    parts = [np.concatenate([means, bm[None]]), np.concatenate([shs, bs[None]]), np.concatenate([opac, [0.9]]),
             np.concatenate([scales, bsc[None]]), np.concatenate([rots, br[None]])]
    sc = _pack(parts, np.concatenate([front_order, [n]]).astype(np.int64), cam, deg)
    sc.ties = n - np.unique(level).size
    assert np.array_equal(sc.means[:n, 2], depth_of_id)        # the levels survive the float32 pack bit for bit
    return sc


MANY_FAINT_ABOVE = 64   # lists beyond this many entries get the faint front (opacity 0.0042), shorter ones 0.05


def many_tile_scene(gx, gy, lengths, seed, deg=0, slack=0):
    """A 16 gx x 16 gy image whose tile t (row-major) has a list of exactly lengths[t] entries: two_tile_scene on a grid.  Front
    splats of sigma 1.05 px, projected centres within [6, 10] px of their tile's origin in x and y — every 3-sigma square
    (radius 5) inside its own tile; distinct depths in [2, 8] whose ranks are dealt to the tiles at random; ids a random
    permutation; the entries at boundary_positions(lengths[t]) of every list pinned, the last one among them, so the deepest
    contributor of every tile is its last entry.  Opacity 0.0042 U(1, 1.5) in lists of more than MANY_FAINT_ABOVE entries, 0.05
    U(1, 1.5) in shorter ones (a 1024-entry list at 0.05 would saturate after some 300 entries; at 0.0042 its walk ends with
    T ~ 0.4).  Principal point in the image centre, focal length 2 W: at _camera()'s 13.9 px a splat 150 px off the axis is
    stretched over several tiles.  No per-tile Python loop over Gaussians: one pass per DISTINCT length.
    slack: pin boundary_positions(length, slack=slack) instead — for a caller that drops up to `slack` entries per list afterwards
    (tests/score_scenes.py) and needs the pinned ones at the boundaries of the lists that remain."""
    lengths = np.asarray(lengths, np.int64)
    assert lengths.shape == (gx * gy,) and (lengths >= 1).all()
    rng = np.random.default_rng([int(seed), gx, gy, int(lengths.sum()), 0x3A9])
    W, H = 16 * gx, 16 * gy
    f = np.float32(2.0 * W)
    cam = Camera(W, H, (f, f))
    fx = float(f)
    n = int(lengths.sum())
    depths = _unique_depths(rng, n)
    tile_of_rank = rng.permutation(np.repeat(np.arange(gx * gy), lengths))
    by_pos = np.argsort(tile_of_rank, kind="stable")           # position (tile-major, then depth) -> depth rank
    tile = tile_of_rank[by_pos]                                # == repeat(arange(T), lengths)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    pinned = np.zeros(n, bool)
    for Lk in np.unique(lengths):
        pinned[(starts[:-1][lengths == Lk][:, None] + boundary_positions(int(Lk), slack=slack)[None, :]).reshape(-1)] = True
    ox, oy = 16.0 * (tile % gx), 16.0 * (tile // gx)
    base = np.where(lengths[tile] > MANY_FAINT_ABOVE, 0.0042, 0.05)
    parts = _front(rng, n, depths[by_pos], 1.05, base, fx, pinned, deg, lo=(ox + 6.0, oy + 6.0), hi=(ox + 10.0, oy + 10.0),
                   cx=W / 2.0, cy=H / 2.0)
    sc = _pack(parts, rng.permutation(n).astype(np.int64), cam, deg)
    sc.lengths = tuple(int(x) for x in lengths)
    return sc


# Views with more than 256 tier tiles (tests/test_gpu_tier_routing.py): (tiles in (1024, 4096], in (4096, 8192], beyond 8192) on a
# 20 x 14 grid -> what gsr_policy_bwd_split must return for those counts on a default 320 x 224 configuration, as
# (n_mid4, n_mid8, n_big, split_len).  Listed in the order in which each case's NEIGHBOUR follows it (the last wraps around).
MANY_GRID = (20, 14)
NO_SPLIT = 0xFFFFFFFF
MANY_TILE_CASES = {(256, 0, 0): (256, 0, 0, 1024),     # the limit itself; the 1024-entry tile stays in the main launch
                   (257, 0, 0): (0, 0, 0, NO_SPLIT),   # default main kernel on lists beyond 1024
                   (256, 1, 0): (0, 1, 0, 4096),       # lists of 1025 .. 4096 in the main launch, 4096 included
                   (250, 6, 1): (0, 6, 1, 4096),       # long kernel over big, then mid8, with n_mid4 = 0
                   (0, 256, 1): (0, 0, 1, 8192),       # lists of 4097 .. 8192, 8192 included, in the main launch
                   (0, 257, 0): (0, 0, 0, NO_SPLIT)}   # default main kernel on lists beyond 4096
MANY_CLASSES = ("mid4", "mid8", "big", "1024", "ten")


def many_tile_lengths(case, seed=5):
    """(lengths, classes) of a MANY_TILE_CASES key: tier tiles at random places of the grid — the first two of a tier ON its upper
    edge (4096, 8192), the others one past its lower edge (1025, 4097); lists beyond 8192 hold 8193 — one ordinary tile of exactly
    1024 entries and ten entries everywhere else.  classes: MANY_CLASSES name -> tile indices."""
    gx, gy = MANY_GRID
    tiles = np.random.default_rng([int(seed), *case]).permutation(gx * gy)
    lengths = np.full(gx * gy, 10, np.int64)
    classes, k = {}, 0
    for name, count, low, edge in (("1024", 1, 1024, 1024), ("mid4", case[0], 1025, 4096), ("mid8", case[1], 4097, 8192),
                                   ("big", case[2], 8193, 8193)):
        classes[name] = np.sort(tiles[k:k + count])
        lengths[tiles[k:k + count]] = low
        lengths[tiles[k:k + min(count, 2)]] = edge
        k += count
    classes["ten"] = np.sort(tiles[k:])
    return lengths, classes


def tile_rows(sc, tiles):
    """Gaussian ids of the pinned entries (boundary_positions) of the given tiles' lists of a many_tile_scene."""
    lengths = np.asarray(sc.lengths, np.int64)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    pos = [starts[t] + boundary_positions(int(lengths[t])) for t in tiles]
    return sc.order[np.concatenate(pos)] if pos else np.zeros(0, np.int64)


def list_positions(st):
    """Sorted position -> Gaussian id of the first tile's list of the oracle state `st` (one-tile scenes: of THE list)."""
    a, b = (int(x) for x in np.asarray(st.ranges)[0])
    return np.asarray(st.values_sorted[a:b]).astype(np.int64)
