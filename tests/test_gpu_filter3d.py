"""-m gpu: the 3-D smoothing filter on the MI355X (csrc/filter3d.hip through smoothing_filter).
  1. the camera sweep against the fp32 restatement of tests/filter3d_ref.py, bit for bit — filter, seen flags and count as
     integers, every N x V of the restatement's cases, the hand-placed rows, a scene nobody sees, two runs; 65 and 258
     partials into the final fold;
  2. the sweep against the float64 twin;
  3. apply, its pullback and the raw (export) values against the float64 twin, the zero-filter pass-through, in place ==
     out of place;
  4. through the rasterizer on cell-101: the autograd chain, the raw-parameter gradients, every row of ∇scales / ∇opacities
     against the oracle composed with the restated pullback and against float64 autograd, the filter term's share;
  5. the four entry points on guarded arenas, and their error codes.
Every test fails on a build without the feature: the package has no smoothing_filter, the library no gsr_filter3d_*."""
import ctypes as C

import numpy as np
import pytest
import torch

import filter3d_ref as fr
import gradient_rows as gr
from guarded import Arena, placements
from hip_helpers import blend_boundary_pixels, dev
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, f32).view(np.int32)


def _same_sweep(got, want, tag):
    filt, seen, count = got
    assert filt.dtype == torch.float32 and seen.dtype == torch.uint8 and tuple(count.shape) == (1,)
    assert int(count.item()) == want.count, (tag, int(count.item()), want.count)
    assert np.array_equal(seen.cpu().numpy(), want.seen.astype(np.uint8)), tag
    bad = np.flatnonzero(bits(filt) != bits(want.filter))
    assert bad.size == 0, (tag, bad[:8], filt.cpu().numpy()[bad[:8]], want.filter[bad[:8]])


# ---- 1. the sweep, bit for bit ----
@pytest.mark.parametrize("V", fr.V_CASES)
@pytest.mark.parametrize("n", fr.N_CASES)
def test_sweep_is_the_fp32_restatement_bit_for_bit(pkg, n, V):
    SF = pkg.smoothing_filter
    cams = fr.make_rig(V)
    table = fr.camera_table(cams)
    pts_h = fr.make_points(n, table)
    want = fr.sweep(pts_h, table, dtype=f32)
    pts = dev(pts_h)
    got = SF.compute_filter_3d(pts, table, return_seen=True)
    _same_sweep(got, want, (n, V))
    again = SF.compute_filter_3d(pts, table, return_seen=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs"
    # without the seen flags (they live in the scratch then), from a camera list, from a table on the device
    for cameras in (table, cams, dev(table)):
        assert np.array_equal(bits(SF.compute_filter_3d(pts, cameras)), bits(want.filter))
    if n >= len(fr.HAND):   # the hand rows: unseen ones carry the fill, the NaN row among them
        assert np.isfinite(got[0].cpu().numpy()).all()
        assert not got[1][6] and not got[1][7]
        if V == 1:
            assert not got[1][0] and bool(got[1][1:6].all())


@pytest.mark.parametrize("n,wg", fr.FOLD_CASES)
def test_final_fold_past_one_wave_and_one_trip(pkg, n, wg):
    """65 and 258 partial maxima and counts into filter3d_final_kernel — the earlier cases stop at 2, which threads 0 and 1 of
    wave 0 hold after one trip of the loop.  The largest filter sits on ONE seen point of workgroup `wg` of the sweep (the
    last, which is wave 1's only partial of 65 and thread 1's second trip of 258; or number 200, in wave 3), and every unseen
    point carries it as the fill: a fold that loses a wave or a trip shows in thousands of rows and in the count
    (tests/test_filter3d_cpu.py holds the inputs to this)."""
    SF = pkg.smoothing_filter
    table, pts_h, at, want = fr.fold_case(n, wg)
    assert want.seen[at] and want.filter[at] == want.filter[want.seen].max() and (~want.seen).sum() > 1000
    pts = dev(pts_h)
    got = SF.compute_filter_3d(pts, table, return_seen=True)
    _same_sweep(got, want, (n, wg))
    assert int(got[2].item()) == int(want.seen.sum())
    again = SF.compute_filter_3d(pts, table, return_seen=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs"
    assert np.array_equal(bits(SF.compute_filter_3d(pts, table)), bits(want.filter)), "the seen flags in the scratch"


@pytest.mark.parametrize("n", [1, 257, 1025])
def test_a_scene_nobody_sees(pkg, n):
    table = fr.camera_table(fr.make_rig(3))
    filt, seen, count = pkg.smoothing_filter.compute_filter_3d(dev(fr.unseen_points(n)), table, return_seen=True)
    assert int(count.item()) == 0 and not bool(seen.any()) and not bits(filt).any()


def test_near_variance_and_margin_reach_the_kernel(pkg):
    SF = pkg.smoothing_filter
    cams = fr.make_rig(3)
    pts_h = fr.make_points(257, fr.camera_table(cams))
    pts = dev(pts_h)
    for near, variance, margin in ((1.0, 0.2, 0.15), (0.2, 0.5, 0.15), (0.2, 0.2, 0.0), (0.0, 0.0, 0.4)):
        table = fr.camera_table(cams, margin)
        want = fr.sweep(pts_h, table, near=near, k=f32(np.sqrt(variance)), dtype=f32)
        got = SF.compute_filter_3d(pts, cams, near=near, variance=variance, margin=margin, return_seen=True)
        _same_sweep(got, want, (near, variance, margin))
    e = SF.compute_filter_3d(torch.zeros(0, 3, device="cuda"), cams, return_seen=True)
    assert e[0].shape == (0,) and e[1].shape == (0,) and int(e[2].item()) == 0
    with pytest.raises(ValueError, match="no cameras"):
        SF.compute_filter_3d(pts, [])
    with pytest.raises(ValueError, match="no cameras"):
        SF.compute_filter_3d(pts, torch.zeros(0, SF.CAMERA_FLOATS, device="cuda"))
    with pytest.raises(ValueError):
        SF.compute_filter_3d(pts, np.zeros((3, 20), f32))
    with pytest.raises(ValueError, match="near"):
        SF.compute_filter_3d(pts, cams, near=-1.0)


# ---- 2. the sweep against the float64 twin ----
@pytest.mark.parametrize("V", [1, 3, 33])
def test_sweep_against_the_float64_twin(pkg, V):
    """|Δfilter| <= 3e-7 · k · inv_f · (Σ_j |R[2+3j]·p_j| + |t[2]|) wherever the device's validity sets — the restatement's,
    by test 1 — agree with the twin's for every camera; at most 1 % of the points may disagree."""
    table = fr.camera_table(fr.make_rig(V))
    pts_h = fr.make_points(4096)
    a, b = fr.sweep(pts_h, table, dtype=f32), fr.sweep(pts_h, table, dtype=np.float64)
    filt, seen, _ = pkg.smoothing_filter.compute_filter_3d(dev(pts_h), table, return_seen=True)
    assert np.array_equal(seen.cpu().numpy().astype(bool), a.seen)
    agree = (a.valid == b.valid).all(0)
    m = agree & b.seen
    err = np.abs(filt.cpu().numpy().astype(np.float64) - b.filter)
    bound = fr.sweep_bound(b, table)
    print(f"V = {V}: {int((~agree).sum())} of 4096 points disagree, {int(m.sum())} compared, worst err / bound {(err[m] / bound[m]).max():.3f}")
    assert (~agree).mean() <= 0.01 and m.sum() > 400
    assert (err[m] <= bound[m]).all()


# ---- 3. apply, pullback, raw ----
def _check_apply(pkg, rows, tag):
    SF = pkg.smoothing_filter
    o, s, f, g_o, g_s = rows
    n = o.shape[0]
    od, sd, fd, god, gsd = dev(o.reshape(n, 1)), dev(s), dev(f), dev(g_o.reshape(n, 1)), dev(g_s)
    oe, se = SF.apply_filter_3d_forward(od, sd, fd)
    assert oe.shape == (n, 1) and se.shape == (n, 3)
    oe64, se64 = fr.apply(o, s, f, np.float64)
    e_se, e_oe = fr.rel(se.cpu().numpy(), se64).max(), fr.rel(oe.cpu().numpy().reshape(-1), oe64).max()
    vo, vs = SF.apply_filter_3d_backward(od, sd, fd, god, gsd)
    vo64, vs64, first, second = fr.apply_backward(o, s, f, g_o, g_s, np.float64, terms=True)
    e_vo = fr.rel(vo.cpu().numpy().reshape(-1), vo64).max()
    e_vs = (np.abs(vs.cpu().numpy() - vs64) / (np.abs(first) + np.abs(second))).max()
    ro, rs = SF.merged_raw(od, sd, fd)
    ro64, rs64 = fr.apply_raw(o, s, f, np.float64)
    e_ro = (np.abs(ro.cpu().numpy().reshape(-1) - ro64) / np.maximum(1.0, np.abs(ro64))).max()
    e_rs = (np.abs(rs.cpu().numpy() - rs64) / np.maximum(1.0, np.abs(rs64))).max()
    print(f"{tag}: se {e_se:.2e}, o_eff {e_oe:.2e}, vo {e_vo:.2e}, vs {e_vs:.2e} of the terms, raw opacity {e_ro:.2e}, raw scale {e_rs:.2e}")
    assert e_se <= 2.4e-7 and e_oe <= 1e-6 and e_vo <= 1e-6 and e_vs <= 2e-6 and e_ro <= 1e-6 and e_rs <= 1e-6
    # in place == out of place, bit for bit; the inputs are left alone
    go2, gs2 = god.clone(), gsd.clone()
    r = SF.apply_filter_3d_backward_(od, sd, fd, go2, gs2)
    assert r[0].data_ptr() == go2.data_ptr() and r[1].data_ptr() == gs2.data_ptr()
    assert torch.equal(go2.view(torch.int32), vo.view(torch.int32)) and torch.equal(gs2.view(torch.int32), vs.view(torch.int32))
    assert np.array_equal(bits(od).reshape(-1), bits(o)) and np.array_equal(bits(sd), bits(s)) and np.array_equal(bits(fd), bits(f))
    return oe, se, vo, vs


def test_apply_and_pullback_against_the_float64_twin(pkg):
    """200 000 rows: se 2.4e-7 (1.5 roundings), o_eff and vo 1e-6 (10.5), vs 2e-6 of |g_s·r| + |filter term| (18.5 per term),
    raw 1e-6 · max(1, |x|); numpy fp32 shows 1.1e-7, 3.7e-7, 3.6e-7, 5.6e-7, 3.8e-7 / 1.7e-7 (tests/test_filter3d_cpu.py)."""
    _check_apply(pkg, fr.apply_rows(200_000), "200 000 rows")


def test_apply_edge_rows(pkg):
    """N = 257: f == 0 passes through bit for bit (the lone thread of the second workgroup is such a row); s = 1e-6 under
    f = 1 gives c = 1e-18 without an underflow."""
    rows = fr.edge_rows()
    o, s, f, g_o, g_s = rows
    oe, se, vo, vs = _check_apply(pkg, rows, "edge rows")
    z = f == 0
    assert z[-1] and z.sum() > 50
    for got, want in ((oe, o), (se, s), (vo, g_o), (vs, g_s)):
        assert np.array_equal(bits(got).reshape(want.shape)[z], bits(want)[z])
    t = (s[:, 0] == f32(1e-6)) & (f == 1)
    assert t.sum() > 20 and bool((oe.cpu().numpy().reshape(-1)[t] > 0).all()) and bool(torch.isfinite(vs).all())
    # and the restatement in fp32 is what the device computes, to the last bit where no logf is involved
    oe32, se32 = fr.apply(o, s, f, f32)
    vo32, vs32 = fr.apply_backward(o, s, f, g_o, g_s, f32)
    for got, want in ((oe, oe32), (se, se32), (vo, vo32), (vs, vs32)):
        assert np.array_equal(bits(got).reshape(want.shape), bits(want))


# ---- 4. through the rasterizer ----
NAME = "cell-101"
_chain = {}


def chain(pkg, orc):
    """cell-101 with its eight views (synthetic.view_pose) as the training cameras: the device's filter, effective parameters
    and gradients by hand, and the reference columns on the oracle state of the effective parameters.  Once."""
    if _chain:
        return _chain
    import f64_model as fm
    R, SF = pkg.rasterizer, pkg.smoothing_filter
    mode, deg, W, H, n = gr.CELLS[101]
    s = pkg.synthetic.make_scene(n, W, H, deg, 101, sigma_px=4.0)
    sc = gr.build_scene(pkg, NAME)
    assert np.array_equal(sc.arrays[0], s.means)
    ocam = sc.cam
    cam = pkg.Camera(W, H, tuple(ocam.focal), tuple(ocam.principal), np.asarray(ocam.R), np.asarray(ocam.t))
    views = [pkg.Camera(W, H, tuple(ocam.focal), tuple(ocam.principal), *pkg.synthetic.view_pose(j)) for j in range(8)]
    raw = dict(means=s.means, opac=s.opacities_raw.reshape(-1, 1), scales=s.scales_raw, rots=s.rotations, dc=s.shs[:, :1].copy(),
               rest=s.shs[:, 1:].copy())
    d = {k: dev(np.ascontiguousarray(v)) for k, v in raw.items()}
    filt = SF.compute_filter_3d(d["means"], views)
    shs, oa, sa = R.prologue_forward(d["dc"], d["rest"], d["opac"], d["scales"])
    oe, se = SF.apply_filter_3d_forward(oa, sa, filt)
    rast = R.GaussianRasterizer(W, H, mode=mode)
    img = rast.forward_raw(d["means"], shs, oe, se, d["rots"], cam, deg, sc.bg).clone()
    vp = dev(sc.vp)
    vm, vsh, vo, vsc, vr, _, _ = rast.backward_raw(vp, d["means"], shs, oe, se, d["rots"], cam, deg, sc.bg)
    g_eff = (vo.clone(), vsc.clone())
    SF.apply_filter_3d_backward_(oa, sa, filt, vo, vsc)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in dict(filt=filt, oa=oa, sa=sa, oe=oe, se=se, shs=shs, vo=vo, vsc=vsc).items()}
    # the references: oracle at the device's effective parameters, its gradients through the restated pullback; float64
    # autograd through effective parameters formed in float64
    args = (s.means, h["shs"], h["oe"].reshape(-1), h["se"], s.rotations)
    st = orc.forward(*args, ocam, deg, background=sc.bg, mode=mode)
    g = orc.backward(st, sc.vp, *args, ocam, deg, background=sc.bg)
    o_vo, o_vs, first, second = fr.apply_backward(h["oa"], h["sa"], h["filt"], g.vopacities, g.vscales, f32, terms=True)
    tt = lambda a, grad=False: torch.tensor(np.asarray(a, np.float64), dtype=fm.DT, requires_grad=grad)  # noqa: E731
    o64, s64, f64 = tt(h["oa"].reshape(-1), True), tt(h["sa"], True), tt(h["filt"])
    se64 = torch.sqrt(s64 * s64 + (f64 * f64)[:, None])
    oe64 = o64 * (s64 / se64).prod(1)
    img64 = fm.render_dense(tt(s.means), tt(h["shs"]), oe64, se64, tt(s.rotations), ocam, deg, np.asarray(sc.bg, f32), mode,
                            st.values_sorted, st.ranges, st.radii)
    (img64 * tt(sc.vp)).sum().backward()
    bmask, _, ids = blend_boundary_pixels(st, h["oe"].reshape(-1), W, H, with_ids=True)
    touched = np.zeros(n, bool)
    touched[list(ids)] = True
    ill = h["se"].max(1) / np.maximum(h["se"].min(1), 1e-30) > gr.ILL_RATIO
    _chain.update(sc=sc, s=s, cam=cam, deg=deg, mode=mode, d=d, filt=filt, shs=shs, oa=oa, sa=sa, oe=oe, se=se, img=img, vp=vp,
                  grads=dict(vm=vm, vsh=vsh, vo=vo, vsc=vsc, vr=vr), g_eff=g_eff, h=h, st=st, vis=st.radii > 0, touched=touched, ill=ill,
                  bmask=bmask, orc=dict(vopacities=o_vo.reshape(n, 1), vscales=o_vs), first=first, second=second,
                  f64=dict(vopacities=o64.grad.numpy().reshape(n, 1), vscales=s64.grad.numpy()), radii=rast.radii.cpu().numpy())
    return _chain


def test_autograd_chain_is_the_by_hand_chain_bit_for_bit(pkg, orc):
    """_Prologue -> apply_filter_3d -> rasterize: the image of `rasterize` fed the separately computed effective tensors, and
    the raw-parameter gradients of prologue_backward(apply_filter_3d_backward_(backward_raw))."""
    c = chain(pkg, orc)
    R, SF = pkg.rasterizer, pkg.smoothing_filter
    sc, d = c["sc"], c["d"]
    leaves = {k: v.clone().requires_grad_(True) for k, v in d.items()}
    rast = R.GaussianRasterizer(sc.cam.width, sc.cam.height, mode=c["mode"])
    shs, oa, sa = R._Prologue.apply(leaves["dc"], leaves["rest"], leaves["opac"], leaves["scales"])
    oe, se = SF.apply_filter_3d(oa, sa, c["filt"])
    img = R.rasterize(leaves["means"], shs, oe, se, leaves["rots"], rast=rast, camera=c["cam"], sh_degree=c["deg"], background=sc.bg)
    assert torch.equal(oe.detach(), c["oe"]) and torch.equal(se.detach(), c["se"])
    assert torch.equal(img.detach(), c["img"])
    assert not torch.equal(c["oe"], c["oa"]) and not torch.equal(c["se"], c["sa"]), "the filter does something"
    order = ("means", "opac", "scales", "rots", "dc", "rest")
    got = torch.autograd.grad((img * c["vp"]).sum(), [leaves[k] for k in order])
    g = c["grads"]
    vdc, vrest, vor, vsr = R.prologue_backward(c["oa"], c["sa"], g["vsh"], g["vo"], g["vsc"], 3)
    want = dict(means=g["vm"], opac=vor, scales=vsr, rots=g["vr"], dc=vdc, rest=vrest)
    for k, x in zip(order, got):
        assert torch.isfinite(x).all() and x.abs().sum() > 0, k
        assert torch.equal(x, want[k].reshape(x.shape)), k
    # the device's effective cotangents went through the restated pullback: the same bits
    vo32, vs32 = fr.apply_backward(c["h"]["oa"], c["h"]["sa"], c["h"]["filt"], c["g_eff"][0].cpu().numpy(), c["g_eff"][1].cpu().numpy(), f32)
    assert np.array_equal(bits(g["vo"]).reshape(-1), bits(vo32)) and np.array_equal(bits(g["vsc"]), bits(vs32))


def test_filtered_gradient_rows(pkg, orc):
    """∇scales and ∇opacities w.r.t. the activated values, row by row (gradient_rows.check_rows, its 2 % cap of exempt rows),
    and the share of the filter's own term: a pullback without it fails here."""
    c = chain(pkg, orc)
    assert np.array_equal(c["radii"], c["st"].radii) and gr.boundary_pixels_ok(c["bmask"])
    vis = c["vis"]
    hip = dict(vopacities=c["h"]["vo"].reshape(-1, 1), vscales=c["h"]["vsc"])
    for nm in ("vopacities", "vscales"):
        rep = gr.check_rows(f"{NAME} [3-D filter] {nm}", hip[nm], c["orc"][nm], c["f64"][nm], vis, c["touched"], c["ill"])
        print(f"rows {rep.name}: checked {rep.checked}, z {rep.z}, a {rep.a}, f {rep.f}, b {rep.b}, exempt {rep.exempt}, "
              f"worst |hip - orc| / T = {rep.worst:.3f}")
        assert rep.checked == int(vis.sum()) > 200
    T, _ = gr.row_tolerance(np.asarray(c["orc"]["vscales"], np.float64), vis)
    share = (np.linalg.norm(c["second"], axis=1)[vis] > T[vis]).mean()
    carried = (np.linalg.norm(hip["vscales"].astype(np.float64) - c["first"], axis=1)[vis] > T[vis]).mean()
    print(f"{NAME}: the filter term of ∇scales exceeds the row tolerance on {share:.1%} of the visible rows; the device's rows carry it on {carried:.1%}")
    assert share > 0.5, "the scene cannot see the filter's term"
    assert carried > 0.5


# ---- 5. guarded arenas ----
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _guarded_calls(lib, P, n, V, tag):
    U8 = torch.uint8
    table_h = fr.camera_table(fr.make_rig(V))
    pts_h = fr.make_points(n, table_h)
    o, s, _, g_o, g_s = fr.edge_rows(n)
    nb = int(lib.gsr_filter3d_scratch_bytes(n))
    assert nb == n + 8 * ((n + 1023) // 1024) + 8
    pts, table = P.place("points", pts_h), P.place("table", table_h)
    filt, seen, count = P.place("filter", (n,)), P.place("seen", (n,), U8), P.place("count", (1,), torch.int32)
    scr = P.place("scratch", (nb,), U8, align=8, role="scratch")
    filt2, scr2 = P.place("filter, no seen, no count", (n,)), P.place("scratch2", (nb,), U8, align=8, role="scratch")
    od, sd, god, gsd = P.place("opacities", o), P.place("scales", s), P.place("g_o", g_o), P.place("g_s", g_s)
    oe, se, ro, rs = P.place("o_eff", (n,)), P.place("s_eff", (n, 3)), P.place("o_raw", (n,)), P.place("s_raw", (n, 3))
    vo, vs = P.place("vo", (n,)), P.place("vs", (n, 3))
    io, is_ = P.place("in-place g_o", g_o, role="inout"), P.place("in-place g_s", g_s, role="inout")
    if P.skew == "worst":
        assert pts.data_ptr() % 16 == 4 and table.data_ptr() % 16 == 4 and scr.data_ptr() % 16 == 8 and seen.data_ptr() % 2 == 1
    for t in (filt, seen, count, scr, filt2, scr2, oe, se, ro, rs, vo, vs):
        t.view(-1).view(U8).fill_(0xFF)
    st = _stream()
    rcs = [lib.gsr_filter3d_compute(n, _ptr(pts), V, _ptr(table), fr.NEAR, float(fr.K), _ptr(filt), _ptr(seen), _ptr(count), _ptr(scr), nb, st),
           lib.gsr_filter3d_compute(n, _ptr(pts), V, _ptr(table), fr.NEAR, float(fr.K), _ptr(filt2), None, None, _ptr(scr2), nb, st),
           lib.gsr_filter3d_apply(n, _ptr(od), _ptr(sd), _ptr(filt), 0, _ptr(oe), _ptr(se), st),
           lib.gsr_filter3d_apply(n, _ptr(od), _ptr(sd), _ptr(filt), 1, _ptr(ro), _ptr(rs), st),
           lib.gsr_filter3d_apply_backward(n, _ptr(od), _ptr(sd), _ptr(filt), _ptr(god), _ptr(gsd), _ptr(vo), _ptr(vs), st),
           lib.gsr_filter3d_apply_backward(n, _ptr(od), _ptr(sd), _ptr(filt), _ptr(io), _ptr(is_), _ptr(io), _ptr(is_), st)]
    assert rcs == [0] * 6, (tag, rcs, lib.gsr_last_error_string().decode())
    torch.cuda.synchronize()
    assert P.check() == [], (tag, P.check())
    P.assert_inputs_unchanged()
    want = fr.sweep(pts_h, table_h, dtype=f32)
    _same_sweep((filt, seen, count), want, tag)
    assert torch.equal(filt2.view(torch.int32), filt.view(torch.int32)), tag
    assert torch.equal(io.view(torch.int32), vo.view(torch.int32)) and torch.equal(is_.view(torch.int32), vs.view(torch.int32)), tag
    return {k: v.clone() for k, v in dict(filt=filt, seen=seen, count=count, oe=oe, se=se, ro=ro, rs=rs, vo=vo, vs=vs).items()}


def test_entry_points_on_guarded_buffers(pkg):
    """N = 257, V = 3 on the five placements: no guard word changes, the inputs are unchanged, poisoned outputs and scratch do
    not reach a result, the same bits everywhere.  Under skew "worst" points and table start at 4 mod 16, the scratch at 8 mod
    16 and the seen flags at an odd address: the entry points may not ask for more."""
    lib = pkg._lib.load()
    ref = None
    for P in placements(1 << 18, "cuda"):
        tag = f"{P.skew}/{P.fill}"
        got = _guarded_calls(lib, P, 257, 3, tag)
        if ref is None:
            ref = got
            continue
        for k in got:
            assert torch.equal(got[k].contiguous().view(-1).view(torch.uint8), ref[k].contiguous().view(-1).view(torch.uint8)), (tag, k)


def test_error_codes(pkg):
    L = pkg._lib
    lib = L.load()
    n, V = 257, 3
    bad = L.GSR_E_INVALID_ARG
    nb = int(lib.gsr_filter3d_scratch_bytes(n))
    assert lib.gsr_filter3d_scratch_bytes(0) == 0 and lib.gsr_filter3d_scratch_bytes(-1) == 0
    P = Arena(1 << 16, "cuda", "aligned", 0)
    pts, table = P.place("points", fr.make_points(n)), P.place("table", fr.camera_table(fr.make_rig(V)))
    filt, scr = P.place("filter", (n,)), P.place("scratch", (nb,), torch.uint8, align=8, role="scratch")
    o, s, g_s = P.place("o", (n,)), P.place("s", (n, 3)), P.place("g_s", (n, 3))
    before = filt.clone()
    st = _stream()
    k, near = float(fr.K), fr.NEAR

    def compute(n=n, pts=pts, V=V, table=table, near=near, k=k, filt=filt, scr=scr, nb=nb):
        return lib.gsr_filter3d_compute(n, _ptr(pts), V, _ptr(table), near, k, _ptr(filt), None, None, _ptr(scr), nb, st)

    for kw, word in ((dict(pts=None), b"null"), (dict(table=None), b"null"), (dict(filt=None), b"null"), (dict(scr=None), b"null"),
                     (dict(V=0), b"camera"), (dict(V=-1), b"camera"), (dict(n=-1), b"negative"), (dict(nb=nb - 1), b"scratch"),
                     (dict(near=-0.5), b"near_plane"), (dict(k=float("nan")), b"near_plane"), (dict(n=1 << 31), b"31 bits")):
        assert compute(**kw) == bad and word in lib.gsr_last_error_string(), kw
    assert compute(n=0) == 0 and compute(n=0, pts=None, table=None, filt=None, scr=None, nb=0) == 0
    odd = scr[4:]
    assert lib.gsr_filter3d_compute(4, _ptr(pts), V, _ptr(table), near, k, _ptr(filt), None, None, _ptr(odd), nb - 4, st) == bad
    assert b"aligned" in lib.gsr_last_error_string()
    for a in ((None, s, filt, o, s), (o, None, filt, o, s), (o, s, None, o, s)):
        assert lib.gsr_filter3d_apply(n, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), 0, _ptr(g_s[:, 0]), _ptr(g_s), st) == bad
    assert lib.gsr_filter3d_apply(n, _ptr(o), _ptr(s), _ptr(filt), 0, None, _ptr(g_s), st) == bad
    assert lib.gsr_filter3d_apply(n, _ptr(o), _ptr(s), _ptr(filt), 0, _ptr(o), _ptr(g_s), st) == bad and b"inputs" in lib.gsr_last_error_string()
    assert lib.gsr_filter3d_apply(-1, _ptr(o), _ptr(s), _ptr(filt), 0, _ptr(filt), _ptr(g_s), st) == bad
    assert lib.gsr_filter3d_apply(0, None, None, None, 0, None, None, st) == 0
    assert lib.gsr_filter3d_apply_backward(n, _ptr(o), _ptr(s), _ptr(filt), None, _ptr(g_s), _ptr(o), _ptr(g_s), st) == bad
    assert lib.gsr_filter3d_apply_backward(n, _ptr(o), _ptr(s), _ptr(filt), _ptr(o), _ptr(g_s), _ptr(o), None, st) == bad
    assert lib.gsr_filter3d_apply_backward(-5, _ptr(o), _ptr(s), _ptr(filt), _ptr(o), _ptr(g_s), _ptr(o), _ptr(g_s), st) == bad
    assert lib.gsr_filter3d_apply_backward(0, None, None, None, None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert P.check() == [] and torch.equal(filt, before), "a refused call touches nothing"
