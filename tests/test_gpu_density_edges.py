"""-m gpu: adaptive density control on the MI355X — csrc/densify.hip and the findall / gather passes of csrc/trainer.hip through
the C ABI (pkg._lib) — held to the float64 definition tests/densify_ref.py at every threshold, workgroup edge and special value.

Every comparison is array_equal on integers or float bits, with two exceptions that tests/test_densify_ref_cpu.py prepares
without a GPU, on the inputs of this file (densify_ref.py holds them):

  masks            the definition reports a row as undecided when its float64 exp / sigmoid lies within 2^-19 (16 to 32 fp32 ulps)
                   of the threshold; such rows are left out, and may be at most 1 % of a case.  Measured: 0 of 4096 rows, for
                   every kind, gamma in {0.05, 0.5, e^-1} and min_opacity in {0.005, 0.3}.  The hand rows are all decided.
  split children,  within TOL_FACTOR = 4 times the largest error that the fp32 restatement (oracle/densify.py on glibc) has
  reset opacity    against the definition on these rows (densify_ref.RESTATEMENT_ERR, measured on 2 x 257 rows x 4 cases x 2
                   seeds, and 1040 opacities):
                     normals         1.3e-7 · max(1, r)      r: the Box-Muller radius of the component      (measured 1.21e-7)
                     point step      1.2e-5 · |sigma .* xi|  3-vector norms; the rounding onto the parent's position
                                                             dominates it                                   (measured 1.10e-5)
                     new scales      2.8e-7  absolute                                                       (measured 2.78e-7)
                     reset opacity   2.4e-7  absolute, rows with sigmoid(o) < 0.1 and |o| < 8               (measured 2.38e-7)
                   The factor is there because the device's expf / logf / sinf / cosf are allowed one to two ulps where glibc
                   is below one; nothing here was tuned on the kernels' output.

The workgroup of compose_rows_kernel composes 2048 / row_words whole rows (one from 2048 words on); the block-edge cases put the
end of the rows, and the first appended row, on the last row of a workgroup, on the first of the next and in the middle.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import densify_ref as R
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TOL = {k: R.TOL_FACTOR * v for k, v in R.RESTATEMENT_ERR.items()}
FILL = -1            # every destination is pre-filled with 0xFF bytes and is SLACK elements longer than the call may write
SLACK = 8


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _addr(t):
    return None if t is None else t.data_ptr()


def devf(a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()


def devi(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def filled(n, dtype):
    """n + SLACK elements of 0xFF bytes."""
    item = torch.empty(0, dtype=dtype).element_size()
    return torch.full(((n + SLACK) * item,), 0xFF, dtype=torch.uint8, device="cuda").view(dtype)


def host(t, n):
    """The first n elements on the host, after asserting that the fill behind them survived."""
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert (a[n:].view(np.uint8) == 0xFF).all(), "a store behind the last element"
    return a[:n]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def check(lib, rc):
    assert rc == 0, (rc, lib.gsr_last_error_string().decode())


# ---------------------------------------------------------------------------------------------------------------------
# gsr_densify_grad_mean
def _grad_mean_inputs():
    rng = np.random.default_rng(11)
    n = 257
    d = rng.integers(1, 4, n).astype(f32)
    a = (rng.gamma(2.0, 2e-4, n) * d).astype(f32)
    nan, inf = np.nan, np.inf
    special = [(0, 0), (2, 0), (-2, 0), (1e-30, 1e10), (-1e-30, 1e10), (nan, 1), (inf, inf), (1e-45, 3), (3e-39, 7), (1, inf),
               (-0.0, 1), (3.4e38, 1e-3)]
    for k, (x, y) in enumerate(special):
        a[k], d[k] = x, y
    a[254:257], d[254:257] = [0, 2, -2], 0                      # the last row of a workgroup, the first of the next
    return a, d, len(special)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_grad_mean_bits(pkg, n):
    lib = pkg._lib.load()
    a, d, n_special = _grad_mean_inputs()
    want = R.grad_mean(a, d)
    assert want[0] == 0 and want[1] == np.inf and want[2] == -np.inf and 0 < want[3] < np.finfo(f32).tiny and want[5] == 0
    assert want[254] == 0 and want[255] == np.inf and want[256] == -np.inf
    ad, dd = devf(a), devf(d)
    out = filled(n, torch.float32)
    check(lib, lib.gsr_densify_grad_mean(n, _ptr(ad), _ptr(dd), _ptr(out), _stream()))
    assert np.array_equal(bits(host(out, n)), bits(want[:n]))
    if n == 1:                                                  # every special row as the only row of a call
        for k in range(n_special):
            out = filled(1, torch.float32)
            check(lib, lib.gsr_densify_grad_mean(1, _ptr(ad[k:]), _ptr(dd[k:]), _ptr(out), _stream()))
            assert np.array_equal(bits(host(out, 1)), bits(want[k:k + 1])), k


# ---------------------------------------------------------------------------------------------------------------------
# gsr_densify_mask
def gpu_mask(lib, c, sd):
    n = c["n"]
    g, s, o = (None if c[k] is None else devf(c[k]) for k in ("grad", "scales", "opacities"))
    r = devi(c["max_radii"])
    m = filled(n, torch.uint8)
    check(lib, lib.gsr_densify_mask(c["kind"], n, c["n_grad"], _ptr(g), _ptr(s), sd, _ptr(o), _ptr(r), c["thr"], c["gamma"],
                                    c["min_opacity"], c["max_screen_size"], _ptr(m), _stream()))
    return host(m, n)


def definition_mask(c):
    return R.masks(c["kind"], c["grad"], c["n_grad"], c["scales"], c["opacities"], c["max_radii"], c["thr"], c["gamma"],
                   c["min_opacity"], c["max_screen_size"])


@pytest.mark.parametrize("sd", [1, 3])
@pytest.mark.parametrize("n", R.MASK_N)
def test_mask_random_rows(pkg, n, sd):
    lib = pkg._lib.load()
    scales, opac, grad, radii = (a[:n] for a in R.mask_case(sd))
    n_grad = n - 5 if n > 5 else n
    for kind in (R.CLONE, R.SPLIT, R.PRUNE):
        for gamma in R.GAMMAS:
            for mo in (R.MIN_OPACITIES if kind == R.PRUNE else R.MIN_OPACITIES[:1]):
                c = dict(kind=kind, n=n, n_grad=0 if kind == R.PRUNE else n_grad, grad=None if kind == R.PRUNE else grad[:n_grad],
                         scales=scales, opacities=opac, max_radii=radii, thr=R.MASK_THR, gamma=gamma, min_opacity=mo,
                         max_screen_size=R.MASK_SCREEN)
                want, decided = definition_mask(c)
                assert (~decided).sum() <= n // 100, (kind, gamma, mo)
                got = gpu_mask(lib, c, sd)
                assert set(np.unique(got)) <= {0, 1}
                bad = np.flatnonzero((got != want) & decided)
                assert bad.size == 0, (kind, gamma, mo, bad[:8])
                if kind != R.PRUNE and n > n_grad:              # rows beyond n_grad count as 0, whatever lies behind grad
                    assert not got[n_grad:].any()


@pytest.mark.parametrize("sd", [1, 3])
def test_mask_hand_rows(pkg, sd):
    """grad == thr and one ulp either side, NaN, rows at and beyond n_grad under thr > 0, = 0 and < 0, a NULL grad, exp(0) == gamma,
    the largest scale and a NaN on each axis, max_radii at the bound, max_screen_size = 0 over poisoned scales and a NULL max_radii,
    opacity +-100 and NaN: the mask written down by hand, which the definition and the restatement reproduce on the CPU."""
    lib = pkg._lib.load()
    for c in R.hand_mask_calls(sd):
        want, decided = definition_mask(c)
        assert decided.all() and np.array_equal(want.astype(np.uint8), c["expect"]), c["name"]
        got = gpu_mask(lib, c, sd)
        assert np.array_equal(got, c["expect"]), (c["name"], got, c["expect"])


# ---------------------------------------------------------------------------------------------------------------------
# gsr_compose_rows
def gpu_compose(pkg, groups, keep, n_keep, sel, n_sel, reps, expect_rc=0):
    """groups: (src array or None, row_words, new_zero, wants a destination).  Returns the destinations' rows (None for a group
    without one)."""
    L, lib = pkg._lib, pkg._lib.load()
    rows = n_keep + n_sel * max(reps, 0)
    srcs = [devi(s) for s, _, _, _ in groups]
    dsts = [filled(rows * rw, torch.int32) if has else None for _, rw, _, has in groups]
    cg = (L.ComposeGroup * len(groups))(*[L.ComposeGroup(_addr(s), _addr(d), rw, z) for s, d, (_, rw, z, _) in zip(srcs, dsts, groups)])
    kd, sd_ = devi(keep), devi(sel)
    rc = lib.gsr_compose_rows(cg, len(groups), _ptr(kd), n_keep, _ptr(sd_), n_sel, reps, _stream())
    assert rc == expect_rc, (rc, lib.gsr_last_error_string().decode())
    return [None if d is None else host(d, rows * rw).reshape(rows, rw) for d, (_, rw, _, _) in zip(dsts, groups)]


def check_compose(pkg, srcs, zero, keep, n_keep, sel, n_sel, reps, what, null_src=()):
    groups = [(None if g in null_src else s, s.shape[1], z, True) for g, (s, z) in enumerate(zip(srcs, zero))]
    got = gpu_compose(pkg, groups, keep, n_keep, sel, n_sel, reps)
    for g, (s, z) in enumerate(zip(srcs, zero)):
        want = R.compose(s, keep, n_keep, sel, n_sel, reps, z)
        assert got[g].shape == want.shape, (what, g)
        if not np.array_equal(got[g], want):
            r = np.flatnonzero((got[g] != want).any(axis=1))
            raise AssertionError(f"{what}: group {g} (row_words {s.shape[1]}, new_zero {z}): {r.size} rows differ, first {r[:6]}")


@pytest.mark.parametrize("rw", [1, 3, 4, 45, 48, 2047, 2048, 2049])
def test_compose_block_edges(pkg, rw):
    """Total rows and the keep/new boundary on every side of a workgroup edge, for every form densification uses.  Two groups a
    launch — a copied one and a new_zero one — so the second group's first workgroup is never workgroup 0."""
    rng = np.random.default_rng(rw)
    rpb = 1 if rw >= R.COMPOSE_WORDS else R.COMPOSE_WORDS // rw
    totals = sorted({t for t in (rpb - 1, rpb, rpb + 1, rpb + 3, 2 * rpb + 1) if t > 0})   # (rpb + 3: four new rows behind rpb - 1)
    n_src = max(totals) + 3
    srcs = [rng.integers(1, 2 ** 31, (n_src, rw)).astype(np.int32) for _ in range(2)]
    zero = (0, 1)
    split_one = split_wrap = 0
    for T in totals:
        for n_keep in sorted({rpb - 1, rpb, rpb // 2}):          # first appended row: last of a workgroup, first of the next, inside
            m = T - n_keep
            if m <= 0:
                continue
            sel = rng.integers(0, n_src, m)
            check_compose(pkg, srcs, zero, None, n_keep, sel, m, 1, f"clone T={T} n_keep={n_keep}")
            reps = 2 if m % 2 == 0 else 3 if m % 3 == 0 else 1
            split_one += reps == 2 and m == 2
            split_wrap += reps >= 2 and m > reps
            keep = rng.permutation(n_src)[:n_keep] if n_keep else None
            check_compose(pkg, srcs, zero, keep, n_keep, sel[:m // reps], m // reps, reps, f"split T={T} n_keep={n_keep} reps={reps}")
        # only new rows; the new_zero group has no source at all
        sel = rng.integers(0, n_src, T)
        check_compose(pkg, srcs, zero, None, 0, sel, T, 1, f"new only T={T}", null_src=(1,))
        # prune: n_sel = 0, and reps = 0 with a selection that must not be used
        keep = np.sort(rng.permutation(n_src)[:T])
        check_compose(pkg, srcs, zero, keep, T, None, 0, 1, f"prune T={T}")
        check_compose(pkg, srcs, zero, keep, T, sel[:3], min(3, T), 0, f"prune by reps=0 T={T}")
        # the spatial re-sort: a permutation
        check_compose(pkg, srcs, zero, rng.permutation(T), T, None, 0, 1, f"permutation T={T}")
    assert split_one >= 1 and split_wrap >= 1, "reps = 2 with n_sel = 1 and with a wrapping n_sel both ran"


@pytest.mark.parametrize("empty", [(), (11, 12)])
def test_compose_24_groups(pkg, empty):
    """GSR_COMPOSE_MAX_GROUPS groups of mixed widths in one launch, new_zero alternating (the last group's is set); `empty`
    groups have row_words = 0 and no arrays: the host drops them before the launch."""
    rng = np.random.default_rng(24)
    widths = [1, 3, 4, 45, 48, 2047, 2048, 2049] * 3
    assert len(widths) == pkg._lib.COMPOSE_MAX_GROUPS
    n_src, n_keep, n_sel, reps = 40, 23, 11, 2
    keep, sel = rng.integers(0, n_src, n_keep), rng.integers(0, n_src, n_sel)
    srcs = [rng.integers(1, 2 ** 31, (n_src, w)).astype(np.int32) for w in widths]
    groups = [(None, 0, g % 2, False) if g in empty else (s, w, g % 2, True) for g, (s, w) in enumerate(zip(srcs, widths))]
    got = gpu_compose(pkg, groups, keep, n_keep, sel, n_sel, reps)
    for g, s in enumerate(srcs):
        if g in empty:
            continue
        assert np.array_equal(got[g], R.compose(s, keep, n_keep, sel, n_sel, reps, g % 2)), (g, widths[g])


def test_compose_error_codes(pkg):
    """More than GSR_COMPOSE_MAX_GROUPS groups, a negative row_words, a NULL sel_idx that would be read: GSR_E_INVALID_ARG and
    nothing written."""
    L, lib = pkg._lib, pkg._lib.load()
    s = np.arange(1, 9, dtype=np.int32).reshape(4, 2)
    src, dst, idx = devi(s), filled(6, torch.int32), devi([3])

    def call(n_groups, rw, sel):
        cg = (L.ComposeGroup * n_groups)(*[L.ComposeGroup(_addr(src), _addr(dst), rw, 0)] * n_groups)
        return lib.gsr_compose_rows(cg, n_groups, None, 2, _ptr(sel), 1, 1, _stream())

    assert call(L.COMPOSE_MAX_GROUPS + 1, 2, idx) == L.GSR_E_INVALID_ARG
    assert call(1, -1, idx) == L.GSR_E_INVALID_ARG
    assert call(1, 2, None) == L.GSR_E_INVALID_ARG
    host(dst, 0)
    assert call(1, 2, idx) == 0
    assert np.array_equal(host(dst, 6).reshape(3, 2), s[[0, 1, 3]])


# ---------------------------------------------------------------------------------------------------------------------
# gsr_gather_rows, gsr_mask_findall
@pytest.mark.parametrize("count", [85, 64, 255, 256, 257])
def test_gather_rows(pkg, count):
    """8 groups; count x row_words is 255 (85 x 3, 255 x 1), 256 (64 x 4, 256 x 1) or 257 for one of them: the last word of a
    workgroup, the first of the next.  Descending indices with repeats, then random ones."""
    L, lib = pkg._lib, pkg._lib.load()
    widths = (1, 3, 4, 45, 48, 1, 3, 4)
    assert len(widths) == L.ADAM_MAX_GROUPS
    rng = np.random.default_rng(count)
    n_src = 300
    srcs = [rng.integers(1, 2 ** 31, (n_src, w)).astype(np.int32) for w in widths]
    sdev = [devi(s) for s in srcs]
    for idx in ((n_src - 1 - np.arange(count) // 2), rng.integers(0, n_src, count)):
        dsts = [filled(count * w, torch.int32) for w in widths]
        gg = (L.GatherGroup * len(widths))(*[L.GatherGroup(_addr(s), _addr(d), w) for s, d, w in zip(sdev, dsts, widths)])
        idev = devi(idx)
        check(lib, lib.gsr_gather_rows(gg, len(widths), _ptr(idev), count, _stream()))
        for s, d, w in zip(srcs, dsts, widths):
            assert np.array_equal(host(d, count * w).reshape(count, w), R.gather(s, idx)), w


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2048, 2049])
def test_mask_findall(pkg, n):
    lib = pkg._lib.load()
    rng = np.random.default_rng(n)
    last = np.zeros(n, np.uint8); last[-1] = 1
    edges = np.zeros(n, np.uint8); edges[[i for i in (63, 64, 255, 256, 1023, 1024) if i < n]] = 1
    high = rng.choice(np.uint8([0, 0, 0x80, 1, 0xFF]), n)       # any non-zero byte counts as set
    nb = int(lib.gsr_mask_findall_scratch_bytes(n))
    for name, mask in (("last", last), ("edges", edges), ("all", np.full(n, 1, np.uint8)), ("0x80", high), ("none", np.zeros(n, np.uint8))):
        md = torch.from_numpy(mask).cuda()
        idx, cnt = filled(n, torch.int32), filled(1, torch.int32)
        scr = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
        check(lib, lib.gsr_mask_findall(_ptr(md), n, _ptr(idx), _ptr(cnt), _ptr(scr), _stream()))
        want = np.flatnonzero(mask)
        assert int(host(cnt, 1)[0]) == want.size, name
        got = host(idx, n)
        assert np.array_equal(got[:want.size], want), name
        assert (got[want.size:] == FILL).all(), name            # nothing written past the count


# ---------------------------------------------------------------------------------------------------------------------
# gsr_split_transform
def gpu_split(pkg, p, q, s, sd, seed, n):
    lib = pkg._lib.load()
    pd, sc = filled(3 * n, torch.float32), filled(sd * n, torch.float32)
    pd[:3 * n] = devf(p[:n]).reshape(-1); sc[:sd * n] = devf(s[:n]).reshape(-1)
    qd = devf(q[:n])
    check(lib, lib.gsr_split_transform(n, sd, _ptr(pd), _ptr(qd), _ptr(sc), seed, _stream()))
    return host(pd, 3 * n).reshape(n, 3).copy(), host(sc, sd * n).reshape(n, sd).copy()


def assert_children(got_p, got_s, p, q, s, sd, seed, what):
    n = got_p.shape[0]
    p64, s64, sx = R.split_children(p[:n], q[:n], s[:n], seed, sd)
    err = np.linalg.norm(got_p.astype(f64) - p64, axis=1) / np.linalg.norm(sx, axis=1)
    assert err.max() <= TOL["step"], (what, "point step", float(err.max()), int(err.argmax()))
    es = np.abs(got_s.astype(f64) - s64)
    assert es.max() <= TOL["scale"], (what, "scale", float(es.max()))


@pytest.mark.parametrize("sd", [1, 3])
@pytest.mark.parametrize("n", R.SPLIT_N)
def test_split_identity_frame_gives_the_normals(pkg, n, sd):
    """Identity quaternion, scale 0, parent on the origin: the child's position IS the normal triple of its row — the generator
    itself against the definition, in the normals' own tolerance."""
    p, q, s = R.split_cases(sd)["identity"]
    for seed in R.SPLIT_SEEDS:
        got_p, got_s = gpu_split(pkg, p, q, s, sd, seed, n)
        xi, r = R.normals(seed, n)
        err = np.abs(got_p.astype(f64) - xi) / np.maximum(1.0, r)
        assert err.max() <= TOL["normal"], (seed, float(err.max()), np.unravel_index(err.argmax(), err.shape))
        assert np.abs(got_s.astype(f64) - np.log(1.0 / f64(f32(0.8) * f32(2)))).max() <= TOL["scale"]


@pytest.mark.parametrize("sd", [1, 3])
@pytest.mark.parametrize("n", R.SPLIT_N)
def test_split_random_rows_and_scaled_quaternions(pkg, n, sd):
    cases = R.split_cases(sd)
    p, q, s = cases["random"]
    seed = R.SPLIT_SEEDS[0]
    for name in ("random", "q*1e-3", "q*1e3"):
        _, qs, _ = cases[name]
        got_p, got_s = gpu_split(pkg, p, qs, s, sd, seed, n)
        assert_children(got_p, got_s, p, qs, s, sd, seed, name)
        assert_children(got_p, got_s, p, q, s, sd, seed, name + " against the unit quaternion's children")


@pytest.mark.parametrize("sd", [1, 3])
def test_split_keying_seeds_and_zero_quaternion(pkg, sd):
    p, q, s = R.split_cases(sd)["random"]
    a, b = R.SPLIT_SEEDS
    pa, sa = gpu_split(pkg, p, q, s, sd, a, 257)
    # row i does not depend on n; one seed twice is identical; two seeds differ in every row, and only in the points
    p5, s5 = gpu_split(pkg, p, q, s, sd, a, 5)
    assert np.array_equal(bits(p5), bits(pa[:5])) and np.array_equal(bits(s5), bits(sa[:5]))
    pa2, sa2 = gpu_split(pkg, p, q, s, sd, a, 257)
    assert np.array_equal(bits(pa2), bits(pa)) and np.array_equal(bits(sa2), bits(sa))
    pb, sb = gpu_split(pkg, p, q, s, sd, b, 257)
    assert (pa != pb).any(axis=1).all()
    assert np.array_equal(bits(sb), bits(sa)), "the new scales do not depend on the noise"
    # a zero quaternion: 1 / |q| is Inf, Inf * 0 is NaN in every entry of R — NaN points, as the definition gives; scales as ever
    q0 = q.copy(); q0[1::2] = 0
    pz, sz = gpu_split(pkg, p, q0, s, sd, a, 257)
    p64, _, _ = R.split_children(p, q0, s, a, sd)
    assert np.isnan(p64[1::2]).all() and np.array_equal(np.isnan(pz), np.isnan(p64))
    assert np.array_equal(bits(pz[0::2]), bits(pa[0::2])) and np.array_equal(bits(sz), bits(sa))


# ---------------------------------------------------------------------------------------------------------------------
# gsr_reset_opacity
def test_reset_opacity(pkg):
    lib = pkg._lib.load()
    o, above = R.reset_case()
    o, above = np.concatenate([o, f32([np.nan])]), np.concatenate([above, [False]])
    n = o.shape[0]
    want = R.reset_opacity(o)
    od = filled(n, torch.float32)
    od[:n] = devf(o)
    check(lib, lib.gsr_reset_opacity(n, _ptr(od), _stream()))
    got = host(od, n)
    assert np.isnan(got[-1]) and np.isnan(want[-1]), "a NaN opacity stays a NaN"
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and got[o == -100][0] == -np.inf
    assert np.unique(bits(got[above])).size == 1, "every row above the cut gets one value"
    assert above[[2, 3]].tolist() == [False, True] and above[o == 100][0] and above[np.isposinf(o)][0]
    fin = np.isfinite(want)
    assert fin.sum() == n - 2
    err = np.abs(got[fin].astype(f64) - want[fin])
    assert err.max() <= TOL["reset"], (float(err.max()), o[fin][err.argmax()])


# ---------------------------------------------------------------------------------------------------------------------
# gsr_morton_codes
def test_morton_codes(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    nan, inf = np.nan, np.inf
    rng = np.random.default_rng(21)
    x_all = sum(np.uint64(1) << np.uint64(3 * b) for b in range(21))   # cell 2^21 - 1 on the x axis
    hand = f32([[-1, -2, 0.5], [1, 2, 4.5], [-9, -9, -9], [9, 9, 9], [nan, 0, 1], [0, nan, 1], [0, 0, nan], [inf, -inf, nan],
                [np.nextafter(f32(1), f32(0)), 0, 1]])
    pts = np.concatenate([hand, rng.uniform(-1.5, 5.0, (300, 3)).astype(f32)])
    n = pts.shape[0]
    pd = devf(pts)
    for lo, hi in ((f32([-1, -2, 0.5]), f32([1, 2, 4.5])),                   # power-of-two extents: the point at hi is t == 1 exactly
                   (f32([-1, -2, 0.5]), f32([1, 2, 0.5])),                   # a degenerate axis: cell 0
                   (f32([-0.7, 0.1, -1.3]), f32([4.9, 3.3, 2.2]))):
        codes = filled(n, torch.int64)
        check(lib, lib.gsr_morton_codes(n, _ptr(pd), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), _ptr(codes), _stream()))
        got = host(codes, n).view(np.uint64)
        want = R.morton(pts, lo, hi)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        flat = hi[2] == lo[2]
        assert got[2] == 0 and got[7] == x_all
        if lo[0] == -1:
            assert got[0] == 0
            full = x_all | (x_all << np.uint64(1)) | (np.uint64(0) if flat else x_all << np.uint64(2))
            assert got[1] == full and got[3] == full
    codes = filled(n, torch.int64)
    rc = lib.gsr_morton_codes(n, _ptr(pd), (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, -1, 1), _ptr(codes), _stream())
    assert rc == L.GSR_E_INVALID_ARG
    host(codes, 0)


# ---------------------------------------------------------------------------------------------------------------------
# gsr_count_nonfinite
def test_count_nonfinite(pkg):
    lib = pkg._lib.load()
    n, widths = 257, (1, 3, 4, 45, 48, 1, 3, 4)
    rng = np.random.default_rng(31)
    nan, inf, big = np.nan, np.inf, np.finfo(f32).max
    arrays = [rng.normal(size=(n, w)).astype(f32) for w in widths]
    arrays[0][63, 0] = nan; arrays[0][64, 0] = nan                    # the last lane of a wave, the first of the next
    arrays[1][255, 2] = inf; arrays[1][256, 0] = nan                  # the last row of a workgroup, the first of the next
    arrays[2][70, 1] = nan; arrays[2][100, 3] = inf                   # two rows of one wave: counted twice, the lower one first
    arrays[3][10, 0] = nan; arrays[3][10, 44] = inf                   # two entries of one row: counted once
    arrays[4][200, 47] = -inf
    arrays[5][5, 0] = big; arrays[5][6, 0] = -big; arrays[5][7, 0] = 1e-45   # FLT_MAX and a subnormal are finite
    arrays[7][256, 3] = inf; arrays[7][0, 0] = nan
    want_c, want_f = R.nonfinite(arrays)
    assert want_c.tolist() == [2, 2, 2, 1, 1, 0, 0, 2] and want_f.tolist() == [63, 255, 70, 10, 200, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    dev_ = [devf(a) for a in arrays]
    k = len(widths)
    arr, rw = (C.c_void_p * k)(*[a.data_ptr() for a in dev_]), (C.c_int32 * k)(*widths)
    counts, first = filled(k, torch.int32), filled(k, torch.int32)
    counts[:k] = 12345                                                # the call clears its counters itself
    check(lib, lib.gsr_count_nonfinite(arr, rw, k, n, _ptr(counts), _ptr(first), _stream()))
    assert np.array_equal(host(counts, k).view(np.uint32), want_c)
    assert np.array_equal(host(first, k).view(np.uint32), want_f)
