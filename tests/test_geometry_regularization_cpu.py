"""Geometry regularisation (src/geometry_regularization.jl) without a GPU: the numpy restatement in geometry_ref.py against
an independent torch float64 autograd formulation and central differences, the reference's own tests
(test/runtests.jl:613-695) re-expressed, the "too little evidence" gate, and the argument checks of the
gsr_normal_loss_* / gsr_flatten_loss entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_ref as gr
import geometry_torch as gt


@pytest.mark.parametrize("W,H,f", [(97, 61, 100.0), (64, 48, 100.0), (40, 33, 350.0)])
def test_restatement_vs_torch_float64_autograd(W, H, f):
    img = gt.noisy_frame(W, H, f, seed=W * 3 + H)
    r = gr.depth_normal(img, (f, f), weight=0.05)
    loss, grad, ok, sum_w, count = gt.gradient(img, (f, f))
    assert np.array_equal(ok, r["valid"]) and count == r["count"] and 0.3 <= ok.mean() <= 0.7
    assert abs(sum_w - r["sum_w"]) <= 1e-12 * sum_w
    assert abs(r["loss"] - 0.05 * loss) <= 1e-12 * abs(loss)
    for ch in (3, 4, slice(5, 8)):
        assert np.abs(grad[..., ch]).max() > 0
        assert gt.rel_l2(r["vimage"][..., ch], 0.05 * grad[..., ch]) <= 1e-12
    assert not r["vimage"][..., :3].any() and not grad[..., :3].any()
    # the same masks in float32: the family sits away from the thresholds
    assert np.array_equal(gt.depth_normal(img, (f, f), dtype=torch.float32)[2], ok)


def test_restatement_vs_central_differences():
    """A few pixels well inside valid neighbourhoods; steps small enough that no mask decision moves."""
    W, H, f = 48, 36, 100.0
    img = gt.noisy_frame(W, H, f, seed=5).astype(np.float64)
    base = gr.depth_normal(img, (f, f))
    ok = base["valid"]
    picked = 0
    for y, x in zip(*np.nonzero(ok)):
        if picked == 6:
            break
        if not (2 <= y < H - 4 and 2 <= x < W - 4 and ok[y - 1:y + 2, x - 1:x + 2].all()):
            continue
        picked += 1
        py, px = y + 1, x + 1   # the centre's pixel
        for ch, h in ((3, 1e-5), (4, 1e-6), (5, 1e-5), (6, 1e-5), (7, 1e-5)):
            lo, hi = img.copy(), img.copy()
            lo[py, px, ch] -= h
            hi[py, px, ch] += h
            rl, rh = gr.depth_normal(lo, (f, f)), gr.depth_normal(hi, (f, f))
            assert np.array_equal(rl["valid"], ok) and np.array_equal(rh["valid"], ok)
            # (the normaliser Σw is detached: hold it where α moves)
            fd = (rh["loss"] * max(rh["sum_w"], 1.0) - rl["loss"] * max(rl["sum_w"], 1.0)) / (2 * h) / max(base["sum_w"], 1.0)
            if ch == 4:
                # ... and so is the weight w = α_c of the centre itself: take its term out of the difference
                dw = (float(rh["weights"][py, px]) - float(rl["weights"][py, px])) / (2 * h)
                fd -= dw * base["one_minus_cos"][py - 1, px - 1] / max(base["sum_w"], 1.0)
            g = base["vimage"][py, px, ch]
            assert abs(fd - g) <= 1e-5 * max(abs(g), 1e-3), (py, px, ch, fd, g)
    assert picked == 6


# ---- the reference's own tests (test/runtests.jl:613-695) ----

def test_flatten_reference_cases():
    # columns of the reference's (3, N) matrix are Gaussians: minima 0, 1, 3
    s = np.array([[1, 0, 2], [2, 5, 1], [3, 4, 6]], np.float32)
    loss, g_raw, g_act = gr.flatten(s)
    assert abs(loss - np.mean(np.exp([0.0, 1.0, 3.0]))) <= 1e-12
    assert np.count_nonzero(g_raw) == 3
    assert abs(g_raw[0, 1] - np.exp(0.0) / 3) <= 1e-12 and abs(g_raw[1, 2] - np.exp(1.0) / 3) <= 1e-12
    assert abs(g_raw[2, 0] - np.exp(3.0) / 3) <= 1e-12
    assert np.count_nonzero(g_act) == 3 and np.allclose(g_act[g_act != 0], 1 / 3)
    # all axes tied (the initialisation): exactly one axis per Gaussian wins, the first
    tied = np.ones((4, 3), np.float32)
    loss, g_raw, _ = gr.flatten(tied)
    assert abs(loss - np.e) <= 1e-12 and np.count_nonzero(g_raw) == 4 and np.count_nonzero(g_raw[:, 0]) == 4
    assert gr.flatten(np.zeros((0, 3), np.float32))[0] == 0.0
    # isotropic (N, 1): the single axis wins
    loss, g_raw, g_act = gr.flatten(np.array([[0.5], [-1.0]], np.float32), weight=2.0)
    assert abs(loss - 2.0 * (np.exp(0.5) + np.exp(-1.0)) / 2) <= 1e-12 and np.allclose(g_act, 1.0)
    # against autograd
    r = np.random.default_rng(1).normal(size=(50, 3))
    t = torch.tensor(r, requires_grad=True)
    (torch.exp(t.min(dim=1).values).mean() * 0.3).backward()
    loss, g_raw, _ = gr.flatten(r, 0.3)
    assert np.abs(g_raw - t.grad.numpy()).max() <= 1e-15


def test_depth_normal_reference_cases():
    W, H, f = 64, 48, 100.0
    plane = gt.plane_frame(W, H, f)
    assert (plane[..., 3] > 0).all()
    assert abs(gr.depth_normal(plane, (f, f))["loss"]) < 1e-4
    flat = gt.plane_frame(W, H, f, normals=(0.0, 0.0, -1.0))
    r = gr.depth_normal(flat, (f, f))
    expect = 1.0 - float(gt.PLANE_N @ np.array([0.0, 0.0, -1.0]))
    assert abs(r["loss"] - expect) <= 1e-3 * expect
    assert r["count"] == (W - 2) * (H - 2)
    # transparent views carry no geometry
    r04 = gr.depth_normal(gt.plane_frame(W, H, f, alpha=0.4), (f, f))
    assert r04["loss"] == 0.0 and r04["count"] == 0 and not r04["vimage"].any()
    # finite non-zero gradients on all three inputs, and the quotient rule vα = -(D/α)·vD
    v = r["vimage"]
    for ch in (3, 4, slice(5, 8)):
        assert np.isfinite(v[..., ch]).all() and np.abs(v[..., ch]).max() > 0
    D, A = flat[..., 3].astype(np.float64), flat[..., 4].astype(np.float64)
    assert np.allclose(v[..., 4], -(D / A) * v[..., 3], rtol=1e-4, atol=0.0)
    # the same through the torch formulation, in float32 as the reference runs it
    loss32, g32, _, _, _ = gt.gradient(flat, (f, f), dtype=torch.float32)
    assert abs(loss32 - expect) <= 1e-3 * expect
    assert np.allclose(g32[..., 4], -(D / A) * g32[..., 3], rtol=1e-4, atol=1e-12)


# ---- the gate ----

def _opaque_block(W, H, f, bw, bh):
    """The plane, opaque on a bw x bh block of pixels and α = 0.4 elsewhere: (bw-2)·(bh-2) valid centres."""
    a = np.full((H, W), 0.4)
    a[5:5 + bh, 7:7 + bw] = 1.0
    return gt.plane_frame(W, H, f, normals=(0.0, 0.0, -1.0), alpha=a)


def test_gate_on_the_number_of_valid_centres():
    W, H, f = 40, 30, 100.0
    r63 = gr.depth_normal(_opaque_block(W, H, f, 9, 11), (f, f))    # 7 x 9
    r64 = gr.depth_normal(_opaque_block(W, H, f, 10, 10), (f, f))   # 8 x 8
    assert r63["count"] == 63 and r63["loss"] == 0.0 and not r63["vimage"].any()
    assert r64["count"] == 64 and r64["loss"] > 0.0 and r64["vimage"].any()
    assert r63["sum_w"] == 63.0 and r64["sum_w"] == 64.0    # the counts are reported also where the gate closes
    for img, n in ((_opaque_block(W, H, f, 9, 11), 63), (_opaque_block(W, H, f, 10, 10), 64)):
        loss, grad, ok, _, count = gt.gradient(img, (f, f))
        assert count == n and (loss > 0) == (n >= 64) and grad.any() == (n >= 64)


def test_gate_on_the_weight_sum_cannot_bind_alone():
    """Σw >= 16 (geometry_regularization.jl:180): a valid centre has w = α_c >= 0.5, so count >= 64 implies Σw >= 32 —
    no input puts Σw "just under 16" behind an open count gate.  What inputs CAN do is checked: the smallest Σw of an open
    gate, and Σw straddling 16 (31 and 33 centres of α = 0.5: 15.5 and 16.5) behind a closed one."""
    W, H, f = 40, 30, 100.0

    def half_opaque(n_centres_w, n_centres_h):
        a = np.full((H, W), 0.4)
        a[5:5 + n_centres_h + 2, 7:7 + n_centres_w + 2] = 0.5
        return gt.plane_frame(W, H, f, normals=(0.0, 0.0, -1.0), alpha=a)
    r = gr.depth_normal(half_opaque(8, 8), (f, f))
    assert r["count"] == 64 and r["sum_w"] == 32.0 and r["loss"] > 0.0
    under, over = gr.depth_normal(half_opaque(31, 1), (f, f)), gr.depth_normal(half_opaque(11, 3), (f, f))
    assert (under["count"], under["sum_w"]) == (31, 15.5) and (over["count"], over["sum_w"]) == (33, 16.5)
    assert under["loss"] == 0.0 and over["loss"] == 0.0 and not under["vimage"].any() and not over["vimage"].any()


@pytest.mark.parametrize("W,H", [(2, 5), (5, 2), (1, 1), (2, 2), (3, 3)])
def test_frames_without_enough_interior(W, H):
    img = gt.plane_frame(W, H, 100.0)
    r = gr.depth_normal(img, (100.0, 100.0))
    assert r["loss"] == 0.0 and not r["vimage"].any() and r["weights"].shape == (H, W)
    # (3, 3) has one interior pixel, a valid centre: it is counted and weighted, and the gate closes on it
    assert r["count"] == int(r["weights"].sum()) == (1 if (W, H) == (3, 3) else 0)


def test_invalid_centres_with_nonfinite_values_cost_nothing():
    """The intended deviation: NaN / Inf at centres that are invalid anyway leave loss and gradients finite, and equal to
    those of the frame with these values replaced by harmless finite ones."""
    W, H, f = 48, 36, 100.0
    img = gt.noisy_frame(W, H, f, seed=11)
    clean = img.copy()
    clean[10:14, 10:14, 4] = 0.2            # a transparent patch: its centres and their neighbours are invalid
    clean[20:23, 30:33, 4] = 0.1
    bad = clean.copy()
    bad[11:13, 11:13, 3] = np.nan           # ... with non-finite depth, alpha (still not opaque) and normals inside
    bad[11, 11, 4] = np.nan
    bad[12, 12, 5:8] = np.inf
    bad[21, 31, 3] = np.inf
    bad[21, 31, 5] = -np.inf
    a, b = gr.depth_normal(clean, (f, f), weight=0.05), gr.depth_normal(bad, (f, f), weight=0.05)
    assert np.array_equal(a["valid"], b["valid"]) and np.array_equal(a["weights"], b["weights"])
    assert np.isfinite(b["loss"]) and np.isfinite(b["vimage"]).all()
    assert a["loss"] == b["loss"] and np.array_equal(a["vimage"], b["vimage"])


# ---- argument checks: every one fails with GSR_E_INVALID_ARG before any HIP call (no device here) ----

def test_scratch_bytes_and_invalid_arguments(pkg):
    L = pkg._lib
    lib = L.load()
    E = L.GSR_E_INVALID_ARG
    assert lib.gsr_normal_loss_scratch_bytes(1920, 1080) == (4 + 30 * 68 * 3) * 4    # header + 3 floats per 64x16 tile
    assert lib.gsr_normal_loss_scratch_bytes(3, 3) == (4 + 3) * 4
    assert lib.gsr_normal_loss_scratch_bytes(0, 10) == 0 and lib.gsr_normal_loss_scratch_bytes(10, -1) == 0
    assert lib.gsr_flatten_loss_scratch_bytes(0) == 0 and lib.gsr_flatten_loss_scratch_bytes(-5) == 0
    assert lib.gsr_flatten_loss_scratch_bytes(1) == 4 and lib.gsr_flatten_loss_scratch_bytes(2048) == 4
    assert lib.gsr_flatten_loss_scratch_bytes(2049) == 8 and lib.gsr_flatten_loss_scratch_bytes(1_000_003) == 489 * 4
    p = C.c_void_p(16)    # non-null dummies stand in for device pointers: never dereferenced when the call is refused
    cam = L.CameraS()
    cam.focal[0] = cam.focal[1] = 100.0
    cam.principal[0] = cam.principal[1] = 0.5
    nocam = L.CameraS()
    nb = lib.gsr_normal_loss_scratch_bytes(64, 48)

    def fwd(W=64, H=48, Cc=8, im=p, cm=cam, loss=p, st=p, wm=None, sc=p, nsc=nb):
        return lib.gsr_normal_loss_forward(W, H, Cc, im, None if cm is None else C.byref(cm), 0.05, loss, st, wm, sc, nsc, None)
    for kw in (dict(W=0), dict(H=-3), dict(Cc=3), dict(Cc=5), dict(Cc=9), dict(im=None), dict(cm=None), dict(cm=nocam),
               dict(loss=None), dict(st=None), dict(sc=None), dict(nsc=nb - 1), dict(nsc=0)):
        assert fwd(**kw) == E, kw
    assert b"8 channels" in (fwd(Cc=5), lib.gsr_last_error_string())[1]

    def bwd(W=64, H=48, Cc=8, im=p, cm=cam, vp=C.c_void_p(32), sc=p, nsc=nb):
        return lib.gsr_normal_loss_backward(W, H, Cc, im, None if cm is None else C.byref(cm), 0.05, vp, sc, nsc, None)
    for kw in (dict(W=0), dict(H=0), dict(Cc=5), dict(im=None), dict(cm=None), dict(cm=nocam), dict(vp=None), dict(vp=p),
               dict(sc=None), dict(nsc=nb - 4)):
        assert bwd(**kw) == E, kw
    assert b"must not be the image" in (bwd(vp=p), lib.gsr_last_error_string())[1]

    nf = lib.gsr_flatten_loss_scratch_bytes(5000)

    def flat(n=5000, sd=3, s=p, loss=p, vs=None, sc=p, nsc=nf):
        return lib.gsr_flatten_loss(n, sd, s, 0.005, loss, vs, sc, nsc, None)
    for kw in (dict(n=-1), dict(sd=2), dict(sd=0), dict(sd=4), dict(s=None), dict(loss=None), dict(sc=None), dict(nsc=nf - 1),
               dict(n=0, loss=None)):
        assert flat(**kw) == E, kw


def test_host_mirror_refuses_before_any_launch(pkg):
    """Shape and device checks of the Python entry points are ValueErrors (CPU tensors here: nothing can be launched)."""
    G = pkg.geometry_regularization
    cam = pkg.Camera(64, 48, (100.0, 100.0))
    img = torch.zeros((48, 64, 8))
    with pytest.raises(ValueError, match="HIP tensor"):
        G.depth_normal_loss(img, cam)
    with pytest.raises(ValueError, match="HIP tensor"):
        G.depth_normal_loss_backward_(img, cam, torch.zeros_like(img), 0.05)
    with pytest.raises(ValueError, match="HIP tensor"):
        G.flatten_loss(torch.zeros((10, 3)))
    with pytest.raises(ValueError, match="HIP tensor"):
        G.l1_ssim_normal_loss(None, img, torch.zeros((3, 48, 64)), cam, None)
