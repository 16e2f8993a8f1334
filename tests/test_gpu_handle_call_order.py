"""-m gpu: the ORDER in which a caller may issue a handle's entry points.  The parity, gradient-row, list-boundary, sort-tie,
poisoned- and guarded-buffer tests hold what each entry point computes; this file holds what happens between them — above all
around gsr_reserve, which frees and reallocates grow-only scratch WITHOUT copying: a reserve that reallocates anything ends the
live forward (include/gsr.h), one that reallocates nothing leaves it live, bit for bit.

The handle's call-order table.  F = forward, B = backward, U = update_stats, R(...) = reserve; n Gaussians, D = the view's
n_rendered; "grow" = R(4n, 4D), asserted to raise memory_usage() (a reallocation happened: no row passes vacuously); "= ref" =
torch.equal with a fresh handle's F + B on the same inputs and cotangent (five gradient tensors, grad_means_2d, radii).

  order                                         outcome                                              held by
  --------------------------------------------  ---------------------------------------------------  ---------------------------
  B                                             GSR_E_STATE                                          test_gpu_parity.py::test_state_errors
  F(forward-only) B                             GSR_E_STATE                                          test_gpu_forward_only.py
  F B(tail) B                                   GSR_E_STATE (inputs consumed)                        test_gpu_trainer.py::test_fused_step_checks_its_contract
  F F B(generation of the first)                GSR_E_STATE (superseded)                             test_gpu_parity.py::test_state_errors
  F release B                                   GSR_E_STATE; F after it works                        test_gpu_parity.py::test_state_errors
  1  F R(0, 0) B                                = ref; memory_usage unchanged                        test_reserve_of_nothing_...
  2  grow F grow R(n, D) B                      = ref; the two later reserves reallocate nothing     test_reserve_within_capacity_...
  3  F grow | B, U                              GSR_E_STATE; gstate empty; per-forward buffers null  test_grow_after_the_forward_...
     ... F B                                    = ref; no scratch regrowth in that forward
  4  F B grow | U                               GSR_E_STATE; GRAD_MEANS2D null                       test_grow_after_the_backward_...
  5  F B U grow F B                             = ref; U's statistics those of a handle that never   test_post_train_step_order_...
                                                reserved (the order of densification.post_train_step)
  6  F loss grow | fused backward + tail        GSR_E_STATE; no counter, θ, μ, ν moves               test_grow_before_the_fused_step_...
  7  3 through the C ABI, handle-owned radii /  GSR_BUF_RADII null; gsr_update_stats, gsr_backward   test_grow_with_handle_owned_state_arrays_...
     ∇means_2d (gsr_aux.radii = NULL)           GSR_E_STATE
  8  R(4n, 4D) in the library only, F,          memory_usage unchanged (the library reallocates      test_grow_of_the_mirror_alone_...
     rast.reserve(4n, 4D)                       nothing), gstate replaced its arrays: as 3
  9  rows 1 and 3 with F = gsr_forward_scored,  as 1 and 3: a scored forward is a forward; its score   test_scored_forward_in_the_orders_...
     and F(scored) drop | B                     set keeps what it got, the pair after it = ref

Every refusal is reached through a host-side check that returns before any launch — named at each assertion: the rows 3, 4, 6,
7, 8 never put a backward kernel over the fresh allocations of a reserve.  Sequences 3 and 5 also run once with GSR_DEBUG_GUARD=1
(test_gpu_guarded_handle.py's switch: the guards of the buffers a reserve frees are compared at the free)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from hip_helpers import dev
from test_gpu_guarded_handle import debug_guard, guards_ok

pytestmark = pytest.mark.gpu

W, H, N, DEG, BG = 64, 48, 300, 1, (0.1, 0.2, 0.3)
MODES = ("rgb", "rgbdn")          # :rgbdn has the gnormal and s3 buffers :rgb lacks
GROW = 4                          # well past the forward's own slack (25 % per Gaussian, at most 50 % per instance)
NAMES = ("vmeans", "vshs", "vopacities", "vscales", "vrotations", "grad_means_2d", "radii")
_CASES = {}


def _pair(rast, c, scores=None):
    """forward (scored into `scores` if given) + backward on the case's inputs and cotangent: clones of what `ref` holds."""
    rast.forward_raw(*c.t, c.cam, DEG, BG, scores=scores)
    out = rast.backward_raw(c.vp, *c.t, c.cam, DEG, BG)
    return [o.clone() for o in out[:5]] + [rast.gstate.grad_means_2d.clone(), rast.gstate.radii.clone()]


def _stats(rast):
    """update_stats into fresh (zero) densification statistics."""
    mr = torch.zeros(N, dtype=torch.int32, device="cuda")
    acc, den = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    rast.update_stats(mr, acc, den)
    return [mr, acc, den]


def case(pkg, orc, mode):
    """Scene, device inputs, cotangent and `ref` of one mode: computed once, shared by every sequence, never written."""
    if mode in _CASES:
        return _CASES[mode]
    seed = 31 + len(mode)
    s = pkg.synthetic.make_scene(N, W, H, DEG, seed, sigma_px=4.0)
    s.means[::7, 2] = -1.0        # behind the camera: culled, radii 0, zero gradient rows
    c = types.SimpleNamespace(mode=mode, s=s, cam=pkg.Camera(W, H, tuple(s.focal)), ch=pkg._lib.MODES[mode])
    c.t = [dev(s.means), dev(s.shs), dev(s.opacities.reshape(-1, 1)), dev(s.scales), dev(s.rotations)]
    c.vp = dev(np.random.default_rng(seed).standard_normal((H, W, c.ch)).astype(np.float32))
    rast = pkg.rasterizer.GaussianRasterizer(W, H, mode=mode)
    try:
        c.ref = _pair(rast, c)
        c.ref_stats = _stats(rast)            # a handle that never reserved
        c.D = int(rast.stats.n_rendered)
    finally:
        rast.close()
    torch.cuda.synchronize()
    st = orc.forward(s.means, s.shs, s.opacities, s.scales, s.rotations, orc.Camera(W, H, s.focal), DEG)
    radii = c.ref[6].cpu().numpy()
    assert np.array_equal(radii, st.radii) and (radii > 0).any() and not radii[::7].any()
    assert 500 <= c.D <= st.n_rendered < 5000, (c.D, st.n_rendered)   # exact culling: at most the oracle's ~1 400 instances
    assert all(bool(g.abs().sum() > 0) for g in c.ref[:6]) and bool(c.ref_stats[2].sum() > 0)
    _CASES[mode] = c
    return c


def same(got, ref, names=NAMES):
    for name, a, b in zip(names, got, ref):
        assert a.shape == b.shape and torch.equal(a, b), name


def new(pkg, c):
    return pkg.rasterizer.GaussianRasterizer(W, H, mode=c.mode)


def grow(rast, c):
    """reserve(4n, 4D), and the proof that it reallocated: the handle's memory rose."""
    before = rast.memory_usage()
    rast.reserve(GROW * N, GROW * c.D)
    assert rast.memory_usage() > before


def refused(pkg, call, *args, **kw):
    """GsrError(GSR_E_STATE) whose text names the reserve as the reason."""
    with pytest.raises(pkg._lib.GsrError) as e:
        call(*args, **kw)
    assert e.value.code == pkg._lib.GSR_E_STATE and "gsr_reserve" in str(e.value), str(e.value)


def buffer(pkg, rast, which):
    p, sz = C.c_void_p(), C.c_size_t()
    pkg._lib.check(pkg._lib.load().gsr_buffer(rast._h, which, C.byref(p), C.byref(sz)))
    return p.value, sz.value


def forward_is_dropped(pkg, rast, c):
    """The outcomes of row 3 after `forward, grow`.  Nothing here launches a kernel: gsr_backward stops at
    check_backward_state (fwd_valid is false), gsr_update_stats at its own fwd_valid / bwd_valid test, gsr_buffer /
    gsr_copy_buffer at buffer_lookup's sizes (last_n = last_D = 0)."""
    L = pkg._lib
    refused(pkg, rast.backward_raw, c.vp, *c.t, c.cam, DEG, BG)
    mr = torch.zeros(N, dtype=torch.int32, device="cuda")
    acc, den = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    refused(pkg, rast.update_stats, mr, acc, den)
    assert not mr.any() and not acc.any() and not den.any()
    assert rast.gstate.radii.numel() == 0 and tuple(rast.gstate.grad_means_2d.shape) == (0, 2)
    for which in (L.BUF_RADII, L.BUF_GRAD_MEANS2D, L.BUF_VALUES_SORTED, L.BUF_GEOM, L.BUF_NORMALS, L.BUF_GRAD_ROWS, L.BUF_INSTANCE_AUX):
        assert buffer(pkg, rast, which) == (None, 0), which
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.load().gsr_copy_buffer(rast._h, L.BUF_GEOM, word.data_ptr(), 4, L.stream()) == L.GSR_E_STATE
    assert L.load().gsr_copy_buffer(rast._h, L.BUF_GEOM, word.data_ptr(), 0, L.stream()) == 0   # (nothing asked: nothing refused)


def fresh_pair_equals_ref(rast, c, scores=None):
    """... and the handle is as good as new: forward + backward = ref, and that forward regrows no scratch."""
    regrowths = int(rast.stats.scratch_regrowths)
    got = _pair(rast, c, scores)
    assert int(rast.stats.scratch_regrowths) == regrowths and int(rast.stats.n_rendered) == c.D
    same(got, c.ref)


# ---- 1, 2: reserves that reallocate nothing ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_reserve_of_nothing_between_forward_and_backward(pkg, orc, mode):
    c = case(pkg, orc, mode)
    rast = new(pkg, c)
    try:
        rast.forward_raw(*c.t, c.cam, DEG, BG)
        before = rast.memory_usage()
        rast.reserve(0, 0)
        assert rast.memory_usage() == before and rast.gstate.radii.numel() == N
        out = rast.backward_raw(c.vp, *c.t, c.cam, DEG, BG)
        same(list(out[:5]) + [rast.gstate.grad_means_2d, rast.gstate.radii], c.ref)
        same(_stats(rast), c.ref_stats, ("max_radii", "accum", "denom"))
    finally:
        rast.close()


@pytest.mark.parametrize("mode", MODES)
def test_reserve_within_capacity_between_forward_and_backward(pkg, orc, mode):
    c = case(pkg, orc, mode)
    rast = new(pkg, c)
    try:
        rast.reserve(GROW * N, GROW * c.D)      # first allocations: nothing to drop
        rast.forward_raw(*c.t, c.cam, DEG, BG)
        assert int(rast.stats.scratch_regrowths) == 0
        before, p0 = rast.memory_usage(), rast.gstate.radii.data_ptr()
        rast.reserve(GROW * N, GROW * c.D)      # a repeat
        rast.reserve(N, c.D)                    # smaller
        assert rast.memory_usage() == before and rast.gstate.radii.data_ptr() == p0 and rast.gstate.radii.numel() == N
        out = rast.backward_raw(c.vp, *c.t, c.cam, DEG, BG)
        same(list(out[:5]) + [rast.gstate.grad_means_2d, rast.gstate.radii], c.ref)
    finally:
        rast.close()


# ---- 3, 4, 5: a reserve that reallocates --------------------------------------------------------------------------------------
def sequence_3(pkg, c, check=None, scores=None):
    rast = new(pkg, c)
    try:
        rast.forward_raw(*c.t, c.cam, DEG, BG, scores=scores)
        grow(rast, c)
        forward_is_dropped(pkg, rast, c)
        fresh_pair_equals_ref(rast, c, scores)
        if check:
            check(pkg, rast)
    finally:
        rast.close()


def sequence_5(pkg, c, check=None):
    rast = new(pkg, c)
    try:
        same(_pair(rast, c), c.ref)
        stats = _stats(rast)
        grow(rast, c)
        assert rast.gstate.radii.numel() == 0
        fresh_pair_equals_ref(rast, c)
        same(stats, c.ref_stats, ("max_radii", "accum", "denom"))   # written before the reserve: those of a handle that never reserved
        if check:
            check(pkg, rast)
    finally:
        rast.close()


@pytest.mark.parametrize("mode", MODES)
def test_grow_after_the_forward_drops_it(pkg, orc, mode):
    sequence_3(pkg, case(pkg, orc, mode))


@pytest.mark.parametrize("mode", MODES)
def test_grow_after_the_backward_drops_the_pair(pkg, orc, mode):
    c = case(pkg, orc, mode)
    rast = new(pkg, c)
    try:
        same(_pair(rast, c), c.ref)
        assert buffer(pkg, rast, pkg._lib.BUF_GRAD_MEANS2D) == (rast.gstate.grad_means_2d.data_ptr(), N * 8)
        grow(rast, c)
        mr = torch.zeros(N, dtype=torch.int32, device="cuda")
        acc, den = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        refused(pkg, rast.update_stats, mr, acc, den)       # gsr_update_stats' fwd_valid / bwd_valid test, before its launch
        assert not mr.any() and not acc.any() and not den.any()
        assert buffer(pkg, rast, pkg._lib.BUF_GRAD_MEANS2D) == (None, 0)
        assert tuple(rast.gstate.grad_means_2d.shape) == (0, 2)
    finally:
        rast.close()


@pytest.mark.parametrize("mode", MODES)
def test_post_train_step_order_is_untouched(pkg, orc, mode):
    sequence_5(pkg, case(pkg, orc, mode))


@pytest.mark.parametrize("mode", MODES)
def test_sequences_3_and_5_on_a_guarded_handle(pkg, orc, mode):
    """GSR_DEBUG_GUARD=1: every buffer the reserve frees has its guard compared at the free, the new ones at the end."""
    c = case(pkg, orc, mode)
    with debug_guard(True):
        sequence_3(pkg, c, check=guards_ok)
        sequence_5(pkg, c, check=guards_ok)


# ---- 9: the scored forward in the orders above --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_scored_forward_in_the_orders_of_rows_1_and_3(pkg, orc, mode):
    """gsr_forward_scored where rows 1 and 3 have gsr_forward, and gsr_drop_forward behind it.  The score set of one view, taken
    on a handle nothing happened to, is what every scored forward here adds: a dropped forward's scores are not taken back."""
    c = case(pkg, orc, mode)
    K = pkg.contribution
    one = K.ContributionScores(N, "cuda")
    rast = new(pkg, c)
    try:
        # row 1: F(scored) R(0, 0) B = ref
        rast.forward_raw(*c.t, c.cam, DEG, BG, scores=one)
        before = rast.memory_usage()
        rast.reserve(0, 0)
        assert rast.memory_usage() == before and rast.gstate.radii.numel() == N
        out = rast.backward_raw(c.vp, *c.t, c.cam, DEG, BG)
        same(list(out[:5]) + [rast.gstate.grad_means_2d, rast.gstate.radii], c.ref)
        same(_stats(rast), c.ref_stats, ("max_radii", "accum", "denom"))
        assert int(one.hits.sum()) > 0 and not one.hits[::7].any()
        # F(scored) drop | B: refused before any launch (check_backward_state), then a scored pair = ref
        two = K.ContributionScores(N, "cuda")
        rast.forward_raw(*c.t, c.cam, DEG, BG, scores=two)
        pkg._lib.check(pkg._lib.load().gsr_drop_forward(rast._h))
        refused(pkg, rast.backward_raw, c.vp, *c.t, c.cam, DEG, BG)
        same(_pair(rast, c, two), c.ref)
        assert two.n_views == 2 and torch.equal(two.hits, 2 * one.hits) and torch.equal(two.q, 2 * one.q) and torch.equal(two.bits, one.bits)
    finally:
        rast.close()
    # row 3: F(scored) grow | B, U refused; F(scored) B = ref
    three = K.ContributionScores(N, "cuda")
    sequence_3(pkg, c, scores=three)
    assert three.n_views == 2 and torch.equal(three.hits, 2 * one.hits) and torch.equal(three.q, 2 * one.q)
    assert torch.equal(three.bits, one.bits)


# ---- 6: the fused backward + trainer tail ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_grow_before_the_fused_step_moves_no_counter_and_no_parameter(pkg, orc, mode):
    c = case(pkg, orc, mode)
    R, O, s = pkg.rasterizer, pkg.optim, c.s
    raw = dict(points=dev(s.means), features_dc=dev(s.shs[:, :1].copy()), features_rest=dev(s.shs[:, 1:].copy()),
               opacities=dev(s.opacities_raw.reshape(-1, 1)), scales=dev(s.scales_raw), rotations=dev(s.rotations))
    opts = {k: O.Adam(raw[k], 1e-3, eps=1e-15) for k in O.GROUPS}
    for k in O.GROUPS:                                    # moments that a stray update would visibly decay
        opts[k].mu.fill_(0.25); opts[k].nu.fill_(0.5)
    act = list(R.prologue_forward(raw["features_dc"], raw["features_rest"], raw["opacities"], raw["scales"]))
    target = dev(np.random.default_rng(3).uniform(0, 1, (3, H, W)).astype(np.float32))
    rast = new(pkg, c)
    try:
        img = rast.forward_raw(raw["points"], *act, raw["rotations"], c.cam, DEG, BG)
        _, vp = pkg.fused_ssim.l1_ssim_loss(rast, img, target)
        grow(rast, c)
        was = [(raw[k].clone(), opts[k].mu.clone(), opts[k].nu.clone()) for k in O.GROUPS] + [tuple(a.clone() for a in act)]
        # gsr_backward_trainer_tail stops at check_backward_state, before tail_lr_t and before any launch
        refused(pkg, O.fused_backward_tail_step, rast, vp, opts, raw, *act, c.cam, DEG, BG,
                forward_generation=rast.stats.generation, color_cotangent=True)
        torch.cuda.synchronize()
        assert all(o.current_step == 0 for o in opts.values())
        for k, (theta, mu, nu) in zip(O.GROUPS, was):
            assert torch.equal(raw[k], theta) and torch.equal(opts[k].mu, mu) and torch.equal(opts[k].nu, nu), k
        assert all(torch.equal(a, b) for a, b in zip(act, was[-1]))
    finally:
        rast.close()


# ---- 7: the C ABI with handle-owned radii / ∇means_2d -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_grow_with_handle_owned_state_arrays_through_the_c_abi(pkg, orc, mode):
    """gsr_aux.radii = NULL, gsr_grads.vmeans2d = NULL: the handle owns both arrays, and after the forward its radii pointer
    aims INTO a buffer the reserve frees."""
    c = case(pkg, orc, mode)
    L, lib = pkg._lib, pkg._lib.load()
    rast = new(pkg, c)
    try:
        h = rast._h
        K = int(c.t[1].shape[1])
        inp = L.Inputs(N, K, DEG, *[x.data_ptr() for x in c.t], (C.c_float * 3)(*BG))
        cs = rast._camera(c.cam, None, None)
        img = torch.zeros(H, W, c.ch, device="cuda")
        aux, stats = L.Aux(None, None, None, 0, 0), L.Stats()
        g = [torch.zeros(N, 3, device="cuda"), torch.zeros(N, K, 3, device="cuda"), torch.zeros(N, 1, device="cuda"),
             torch.zeros(N, 3, device="cuda"), torch.zeros(N, 4, device="cuda")]
        mr = torch.zeros(N, dtype=torch.int32, device="cuda")
        acc, den = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")

        def forward():
            L.check(lib.gsr_forward(h, C.byref(inp), C.byref(cs), img.data_ptr(), C.byref(aux), L.stream(), C.byref(stats)))

        def backward():
            gs = L.Grads(*[x.data_ptr() for x in g], None, None, None, None, int(stats.generation), 0, 0)
            return lib.gsr_backward(h, C.byref(inp), C.byref(cs), c.vp.data_ptr(), C.byref(gs), L.stream())

        def owned(which, dtype, shape):
            out = torch.zeros(shape, dtype=dtype, device="cuda")
            L.check(lib.gsr_copy_buffer(h, which, out.data_ptr(), out.numel() * out.element_size(), L.stream()))
            return out

        forward()
        assert int(stats.n_rendered) == c.D
        p, nbytes = buffer(pkg, rast, L.BUF_RADII)
        assert p and nbytes == N * 4
        before = int(lib.gsr_memory_usage(h))
        L.check(lib.gsr_reserve(h, GROW * N, GROW * c.D))
        assert int(lib.gsr_memory_usage(h)) > before
        assert buffer(pkg, rast, L.BUF_RADII) == (None, 0)
        # gsr_update_stats: its fwd_valid / bwd_valid test; gsr_backward: check_backward_state — both before any launch
        assert lib.gsr_update_stats(h, mr.data_ptr(), acc.data_ptr(), den.data_ptr(), L.stream()) == L.GSR_E_STATE
        assert b"gsr_reserve" in lib.gsr_last_error_string()
        assert backward() == L.GSR_E_STATE and b"gsr_reserve" in lib.gsr_last_error_string()
        torch.cuda.synchronize()
        assert not den.any() and not any(bool(x.any()) for x in g)
        # the handle is as good as new, with both arrays its own
        forward()
        assert backward() == 0, lib.gsr_last_error_string()
        same(g + [owned(L.BUF_GRAD_MEANS2D, torch.float32, (N, 2)), owned(L.BUF_RADII, torch.int32, (N,))], c.ref)
        L.check(lib.gsr_update_stats(h, mr.data_ptr(), acc.data_ptr(), den.data_ptr(), L.stream()))
        same([mr, acc, den], c.ref_stats, ("max_radii", "accum", "denom"))
    finally:
        rast.close()


# ---- 8: only the mirror's arrays grow ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_grow_of_the_mirror_alone_drops_the_forward(pkg, orc, mode):
    """The library's buffers are already large, `gstate` is small: rast.reserve replaces gstate's arrays, whose addresses the
    handle holds since the forward (gsr_aux.radii) — the mirror ends the forward in the library (gsr_drop_forward)."""
    c = case(pkg, orc, mode)
    L = pkg._lib
    rast = new(pkg, c)
    try:
        L.check(L.load().gsr_reserve(rast._h, GROW * N, GROW * c.D))
        rast.forward_raw(*c.t, c.cam, DEG, BG)
        assert len(rast.gstate) == N and buffer(pkg, rast, L.BUF_RADII) == (rast.gstate.radii.data_ptr(), N * 4)
        before = rast.memory_usage()
        rast.reserve(GROW * N, GROW * c.D)
        assert rast.memory_usage() == before          # the library reallocated nothing
        assert len(rast.gstate) == GROW * N           # gstate did
        forward_is_dropped(pkg, rast, c)
        fresh_pair_equals_ref(rast, c)
    finally:
        rast.close()
