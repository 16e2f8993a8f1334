"""The 3-D smoothing filter without a GPU: what pins tests/filter3d_ref.py — the restatement
tests/test_gpu_filter3d.py holds the kernels to — and the host side of smoothing_filter (the camera table's fp32 fields, the
argument errors that need no device)."""
import math

import numpy as np
import pytest
import torch

import filter3d_ref as fr

f32 = np.float32


@pytest.fixture(scope="module")
def sf(pkg):
    return pkg.smoothing_filter


# ---- the sweep ----
@pytest.mark.parametrize("V", [1, 3, 33])
def test_fp32_sweep_against_the_twin(V):
    """N = 4096 random points: where the validity sets of the two evaluations agree for every camera, the filters differ by
    at most sweep_bound; the points where they disagree are at most 1 %."""
    table = fr.camera_table(fr.make_rig(V))
    pts = fr.make_points(4096)
    a, b = fr.sweep(pts, table, dtype=f32), fr.sweep(pts, table, dtype=np.float64)
    agree = (a.valid == b.valid).all(0)
    assert (~agree).mean() <= 0.01
    assert np.array_equal(a.seen[agree], b.seen[agree]) and b.seen.any() and not b.seen.all()
    m = agree & b.seen
    err = np.abs(a.filter.astype(np.float64) - b.filter)
    bound = fr.sweep_bound(b, table)
    print(f"V = {V}: {int((~agree).sum())} disagreeing points, {int(m.sum())} seen, worst err / bound {(err[m] / bound[m]).max():.3f}, "
          f"worst relative error {(err[m] / b.filter[m]).max():.2e}")
    assert (err[m] <= bound[m]).all()
    # the unseen points carry the maximum of the seen ones, in both
    assert (a.filter[~a.seen] == a.filter[a.seen].max()).all() and (b.filter[~b.seen] == b.filter[b.seen].max()).all()


def test_hand_rows_sit_where_they_say():
    """Against camera 0 in fp32: z == near is not valid and the next float is; the four image-edge rows are valid WITH equality
    (one ulp further out they are not); the point behind the rig and the NaN point are seen by nobody."""
    table = fr.camera_table(fr.make_rig(33))
    hand = fr.hand_rows(table)
    assert len(fr.HAND) == hand.shape[0]
    s = fr.sweep(hand, table, dtype=f32)
    assert list(s.valid[0]) == [False, True, True, True, True, True, False, False]
    assert not s.valid[:, 6].any() and not s.valid[:, 7].any() and not s.seen[6] and not s.seen[7]
    c = table[0]
    for row, (j, edge, away) in zip(range(2, 6), ((0, 18, 1), (0, 16, -1), (1, 18, 1), (1, 16, -1))):
        x, z = hand[row, j], hand[row, 2]
        assert c[12 + j] * x + c[14 + j] * z == c[edge + j] * z, fr.HAND[row]
        out = hand[row:row + 1].copy()
        out[0, j] = np.nextafter(x, f32(away * np.inf))
        assert not fr.sweep(out, table[:1], dtype=f32).valid[0, 0], fr.HAND[row]
    # a NaN point changes nobody else's filter
    clean = fr.sweep(hand[:7], table, dtype=f32)
    assert np.array_equal(clean.filter.view(np.int32), s.filter[:7].view(np.int32)) and np.isfinite(s.filter).all()


def test_no_point_seen_is_all_zeros():
    table = fr.camera_table(fr.make_rig(3))
    s = fr.sweep(fr.unseen_points(65), table, dtype=f32)
    assert s.count == 0 and not s.filter.any() and not s.seen.any()


# (n, workgroup) -> (seen points, seen points of the workgroup that holds the maximum)
FOLD_FIGURES = {(65537, 64): (14474, 1), (263169, 257): (58201, 1), (263169, 200): (58200, 257)}


@pytest.mark.parametrize("n,wg", fr.FOLD_CASES)
def test_fold_points_put_the_maximum_where_they_say(n, wg):
    """The inputs of the final fold's GPU cases: ceil(n / 1024) partials (65: wave 1 of the final holds one; 258: a second trip
    for threads 0 and 1), some points seen by no camera — the fill is written — and the largest filter among the seen points on
    ONE point, in workgroup `wg`: the last one, or number 200."""
    table, pts, at, s = fr.fold_case(n, wg)
    n_wg = (n + fr.WG_POINTS - 1) // fr.WG_POINTS
    assert n_wg in (65, 258) and at // fr.WG_POINTS == wg < n_wg and (wg == n_wg - 1) == (at == n - 1)
    assert table.shape[0] == 2 and pts.shape == (n, 3)
    assert s.seen[at] and 0 < s.count < n and s.count == int(s.seen.sum())
    top = np.flatnonzero(s.seen & (s.filter == s.filter[at]))
    assert list(top) == [at] and s.filter[at] == s.filter[s.seen].max(), "one point holds the maximum"
    assert (s.filter[~s.seen].view(np.int32) == s.filter[at].view(np.int32)).all() and (~s.seen).sum() > 1000, "the fill is that point's filter"
    per_wg = np.bincount(np.arange(n) // fr.WG_POINTS, weights=s.seen, minlength=n_wg).astype(int)
    assert (per_wg[:-1] > 0).all(), "every partial count matters"
    print(n, wg, s.count, int(per_wg[wg]))
    assert (s.count, int(per_wg[wg])) == FOLD_FIGURES[n, wg]
    # and the hand rows are still in front
    assert not s.seen[6] and not s.seen[7] and np.isfinite(s.filter).all()


# ---- apply and its pullback ----
def test_analytic_backward_is_autograd_of_the_forward():
    o, s, f, g_o, g_s = fr.apply_rows(2000)
    to, ts = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (o, s))
    tf = torch.tensor(f.astype(np.float64))
    se = torch.sqrt(ts * ts + (tf * tf)[:, None])
    oe = to * (ts / se).prod(1)
    (oe * torch.tensor(g_o.astype(np.float64))).sum().backward(retain_graph=True)
    (se * torch.tensor(g_s.astype(np.float64))).sum().backward()
    vo, vs, first, second = fr.apply_backward(o, s, f, g_o, g_s, np.float64, terms=True)
    assert np.allclose(to.grad.numpy(), vo, rtol=1e-12, atol=0)
    assert (np.abs(ts.grad.numpy() - vs) <= 1e-12 * (np.abs(first) + np.abs(second))).all()
    oe64, se64 = fr.apply(o, s, f, np.float64)
    assert np.allclose(oe.detach().numpy(), oe64, rtol=1e-14) and np.allclose(se.detach().numpy(), se64, rtol=1e-14)


@pytest.mark.parametrize("rows", ["apply", "edge"])
def test_apply_properties(rows):
    """Mass preservation o_eff · Π se == o · Π s, se >= f, and the fp32 evaluation within the bounds the GPU test uses."""
    o, s, f, g_o, g_s = fr.apply_rows(200_000) if rows == "apply" else fr.edge_rows()
    oe64, se64 = fr.apply(o, s, f, np.float64)
    mass = o.astype(np.float64) * s.astype(np.float64).prod(1)
    assert (fr.rel(oe64 * se64.prod(1), mass) <= 1e-14).all()
    oe32, se32 = fr.apply(o, s, f, f32)
    assert oe32.dtype == f32 and se32.dtype == f32
    assert (se32 >= f[:, None]).all() and (se32 >= s).all() and (se64 >= f[:, None]).all()
    assert (fr.rel(oe32.astype(np.float64) * se32.astype(np.float64).prod(1), mass) <= 2e-6).all()
    assert fr.rel(se32, se64).max() <= 2.4e-7 and fr.rel(oe32, oe64).max() <= 1e-6
    vo32, vs32 = fr.apply_backward(o, s, f, g_o, g_s, f32)
    vo64, vs64, first, second = fr.apply_backward(o, s, f, g_o, g_s, np.float64, terms=True)
    assert fr.rel(vo32, vo64).max() <= 1e-6
    assert (np.abs(vs32 - vs64) <= 2e-6 * (np.abs(first) + np.abs(second))).all()
    ro32, rs32 = fr.apply_raw(o, s, f, f32)
    ro64, rs64 = fr.apply_raw(o, s, f, np.float64)
    assert (np.abs(ro32 - ro64) <= 1e-6 * np.maximum(1.0, np.abs(ro64))).all()
    assert (np.abs(rs32 - rs64) <= 1e-6 * np.maximum(1.0, np.abs(rs64))).all()
    # the raw values ARE logit / log of the effective ones
    assert np.allclose(ro64, np.log(oe64 / (1.0 - oe64)), rtol=0, atol=1e-9) and np.array_equal(rs64, np.log(se64))


def test_a_zero_filter_passes_through_bit_for_bit():
    o, s, f, g_o, g_s = fr.edge_rows()
    z = f == 0
    assert z.sum() > 50 and z[-1]
    oe, se = fr.apply(o, s, f, f32)
    vo, vs = fr.apply_backward(o, s, f, g_o, g_s, f32)
    for got, want in ((oe, o), (se, s), (vo, g_o), (vs, g_s)):
        assert np.array_equal(got[z].view(np.int32), want[z].view(np.int32))
    # ... and the tiny-scale rows neither underflow nor overflow: c = 1e-18
    t = (s[:, 0] == f32(1e-6)) & (f == 1)
    assert t.sum() > 20 and (oe[t] > 0).all() and np.isfinite(vs[t]).all() and (se[t] == 1).all()


# ---- the host side ----
def test_camera_table_fields(sf):
    cams = fr.make_rig(5)
    got = sf.camera_table(cams)
    assert got.dtype == f32 and got.shape == (5, sf.CAMERA_FLOATS) and sf.CAMERA_FLOATS == fr.CAMERA_FLOATS == 22
    assert np.array_equal(got.view(np.int32), fr.camera_table(cams).view(np.int32))
    for row, cam in zip(got, cams):
        res = (cam.width, cam.height)
        for j in range(2):
            assert row[14 + j] == f32(cam.principal[j]) * f32(res[j])
            assert row[16 + j] == f32(-0.15) * f32(res[j]) and row[18 + j] == f32(1.15) * f32(res[j])
        assert row[20] == f32(1) / max(f32(cam.focal[0]), f32(cam.focal[1])) and row[21] == 0
        assert np.array_equal(row[:9].reshape(3, 3).T, np.asarray(cam.R, f32)) and np.array_equal(row[9:12], np.asarray(cam.t, f32))
    wide = sf.camera_table(cams, margin=0.5)
    assert wide[1, 16] == f32(-0.5) * f32(33) and wide[1, 19] == f32(1.5) * f32(17)
    assert sf.filter_scale() == f32(math.sqrt(0.2)) == fr.K and sf.filter_scale(0.0) == 0
    # the package's own Camera is such an object
    import gsr_pkg
    cam = gsr_pkg.load().Camera(64, 48, (60.0, 61.0))
    row = sf.camera_table([cam])[0]
    assert np.array_equal(row[:12], np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)) and tuple(row[14:16]) == (32.0, 24.0)


def test_argument_errors_without_a_device(sf):
    with pytest.raises(ValueError, match="no cameras"):
        sf.camera_table([])
    cams = fr.make_rig(2)
    for bad in (-0.1, float("nan"), None):
        with pytest.raises(ValueError, match="margin"):
            sf.camera_table(cams, margin=bad)
    for bad in (-1.0, float("inf"), "0.2"):
        with pytest.raises(ValueError, match="variance"):
            sf.filter_scale(bad)
    with pytest.raises(ValueError, match="focal"):
        sf.camera_table([fr.Cam(64, 48, (0.0, 50.0), (0.5, 0.5), np.eye(3), np.zeros(3))])
    with pytest.raises(ValueError, match="HIP"):
        sf.compute_filter_3d(torch.zeros(5, 3), cams)
    with pytest.raises(ValueError, match="HIP"):
        sf.compute_filter_3d(np.zeros((5, 3), f32), cams)
    z1, z3 = torch.zeros(5, 1), torch.zeros(5, 3)
    with pytest.raises(ValueError):
        sf.apply_filter_3d(z1, z3, torch.zeros(5))
    with pytest.raises(ValueError):
        sf.merged_raw(z1, z3, torch.zeros(5))
    with pytest.raises(ValueError):
        sf.apply_filter_3d_backward_(z1, z3, torch.zeros(5), z1.clone(), z3.clone())
