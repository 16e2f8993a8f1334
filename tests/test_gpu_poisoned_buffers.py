"""-m gpu: every HIP path run three times — clean (GSR_DEBUG_FILL unset, caller outputs zeroed), and with the handle's float
scratch and every caller output pre-filled with a NaN word (0xFFFFFFFF) or a huge finite word (0x7F7F7F7F, 3.4e38: NaN hides
behind comparisons).  A kernel that reads a float it never wrote passes the parity tests as long as the memory holds zeros;
here the poisoned runs must be BIT-identical to the clean one and still meet the oracle criteria of test_gpu_parity.py.

GSR_DEBUG_FILL (gsr.h) fills only the handle buffers that hold nothing but float data (rows, vmean2d, final_T, gnormal, d0-d2,
partial, long_state); the index / key / count buffers are covered by the stale-state sequences at the end instead (a view A,
then B on the same handle == B on a fresh handle, clean runs only).

a. the path matrix and the additional scenes: clean + two poisoned runs, bit-identical; the oracle criteria on the poisoned
   runs wherever the oracle has the quantity (not: compact_binning 2, the trainer tail, the empty scene; the factored form is
   held to the unfactored vshs instead).
b. stateless entry points (SSIM, loss head, prologue, sh_grad_from_views and its tail, PLY rows, gather / compose rows,
   bilateral slice / TV / Adam tail with caller-owned scratch): every output pre-filled, bit-identical to the clean run.
c. stale state.

Routing (composite.hip gsr_launch_* and gsr_api.cpp launch_composite_bwd), which every cell below asserts from gsr_stats /
the stage profile:
  composite_bwd_kernel<C, BG0, VC, ACC>   one wave per tile, every tile not split off:
      ACC = grad_precision != default                    (accurate: never BG0, never a split)
      VC  = 3 if C == 3 or GSR_GRADS_COLOR_COTANGENT, else C
      BG0 = background == 0 and C > 3 and not ACC and VC == C
  composite_bwd_long_kernel<C, BG0>        default precision, tiles of the tier lists (gsr_stats.tier_tiles, > 1024
      instances) split off by gsr_policy_bwd_split; BG0 = background == 0 (also for C == 3); C is the mode's even when VC = 3
  sort_composite_fwd_kernel<C, AUX, KEEP>  the fused sort + forward: runs when the bins are used (compact_binning != 1) and
      the per-instance buffers already hold D (gsr_reserve, an earlier view, or GSR_FORWARD_ONLY = KEEP false);
      AUX = covisibilities or uncertainties given
  composite_fwd_strip_kernel<C, AUX>       every tile when the fused launch did not run (a fresh handle's first training
      view, compact mode), else the tiles of the tier lists
"""
import contextlib
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from hip_helpers import compare_backward, compare_forward, dev, frac_bad, rel_l2
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu

WORDS = {"nan": -1, "big": 0x7F7F7F7F}  # int32 views of 0xFFFFFFFF and 0x7F7F7F7F
POISON = ("nan", "big")
MODES = ("rgb", "rgbd", "rgbdn")
CH = {"rgb": 3, "rgbd": 5, "rgbdn": 8}


def _b(x):
    return "true" if x else "false"


def main_bwd(c, bg0, prec, color):
    acc = prec is not None
    vc = 3 if (c == 3 or color) else c
    return f"composite_bwd_kernel<{c}, {_b(bg0 and c > 3 and not acc and vc == c)}, {vc}, {_b(acc)}>"


def long_bwd(c, bg0):
    return f"composite_bwd_long_kernel<{c}, {_b(bg0)}>"


def fused_fwd(c, aux, keep):
    return f"sort_composite_fwd_kernel<{c}, {_b(aux)}, {_b(keep)}>"


def strip_fwd(c, aux):
    return f"composite_fwd_strip_kernel<{c}, {_b(aux)}>"


COMPOSITE_KERNELS = ("composite_bwd_kernel", "composite_bwd_long_kernel", "sort_composite_fwd_kernel", "composite_fwd_strip_kernel")


def compiled_kernels(lib_path):
    """Every instantiation of the four compositing kernels in the BUILT library, read from the mangled kernel names the host
    side registers (`_ZN..20composite_bwd_kernelILi3ELb0ELi3ELb0EEEv..`), in the notation of main_bwd / long_bwd / ...
    (the long kernel's PASS 1 / 2 pair is one entry: both launch together)."""
    import re
    blob = open(lib_path, "rb").read()
    pat = re.compile(rb"(" + b"|".join(k.encode() for k in COMPOSITE_KERNELS) + rb")I((?:L[ib]\d+E)+)E")
    out = set()
    for m in pat.finditer(blob):
        name = m.group(1).decode()
        args = [int(v) if k == b"i" else bool(int(v)) for k, v in re.findall(rb"L([ib])(\d+)E", m.group(2))]
        if name == "composite_bwd_long_kernel":
            args = args[:2]
        out.add(f"{name}<{', '.join(str(a) if isinstance(a, int) and not isinstance(a, bool) else _b(a) for a in args)}>")
    return out


NAMED = set()  # filled at collection time by the cells' route declarations below (each cell asserts its route when it runs)


@contextlib.contextmanager
def debug_fill(fill):
    """GSR_DEBUG_FILL for the handles created (and grown) inside the block; read by the library at every allocation."""
    old = os.environ.pop("GSR_DEBUG_FILL", None)
    if fill:
        os.environ["GSR_DEBUG_FILL"] = fill
    try:
        yield
    finally:
        os.environ.pop("GSR_DEBUG_FILL", None)
        if old is not None:
            os.environ["GSR_DEBUG_FILL"] = old


def poison(t, fill):
    """A caller output as the run finds it: zeros (clean run) or every 32-bit word the fill word."""
    if t is not None and t.numel():
        if fill is None:
            t.zero_()
        else:
            t.view(torch.int32).fill_(WORDS[fill])
    return t


def empty(*shape, fill):
    return poison(torch.empty(*shape, device="cuda", dtype=torch.float32), fill)


def same_bits(a, b, what):
    assert a.shape == b.shape, what
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    if not torch.equal(a, b):
        d = (a != b).reshape(-1).nonzero()
        raise AssertionError(f"{what}: {d.numel()} of {a.numel()} words differ from the clean run (first at {int(d[0])})")


def assert_same(clean, other, fill):
    assert clean.keys() == other.keys()
    for k, v in clean.items():
        if isinstance(v, torch.Tensor):
            same_bits(v, other[k], f"{k} [{fill}]")
        elif isinstance(v, (list, tuple)) and v and isinstance(v[0], torch.Tensor):
            for i, (x, y) in enumerate(zip(v, other[k])):
                same_bits(x, y, f"{k}[{i}] [{fill}]")
        else:
            assert v == other[k], (k, fill)


class Scene(types.SimpleNamespace):
    pass


def make(pkg, orc, mode, n, W, H, deg, seed, bg, sigma_px=4.0, view=3, K=None):
    s = pkg.synthetic.make_scene(n, W, H, deg, seed, sigma_px=sigma_px, K=K)
    R, t = pkg.synthetic.view_pose(view)
    cam = orc.Camera(W, H, s.focal, R=R, t=t)
    return Scene(means=s.means, shs=s.shs, opac=s.opacities, scales=s.scales, rots=s.rotations, cam=cam, deg=deg,
                 bg=tuple(float(b) for b in bg), mode=mode, W=W, H=H, seed=seed)


def pcam(pkg, cam):
    return pkg.Camera(cam.width, cam.height, tuple(cam.focal), tuple(cam.principal), np.asarray(cam.R), np.asarray(cam.t))


def oracle(orc, sc, vp=None, pose=False, aux=False):
    st = orc.forward(sc.means, sc.shs, sc.opac, sc.scales, sc.rots, sc.cam, sc.deg, background=sc.bg, mode=sc.mode,
                     want_covis=aux, want_uncert=aux)
    g = None if vp is None else orc.backward(st, vp, sc.means, sc.shs, sc.opac, sc.scales, sc.rots, sc.cam, sc.deg,
                                             background=sc.bg, pose_grad=pose)
    return st, g


def backward_into(pk, rast, vp, t, camera, deg, bg, Rd, td, arena, vR, vt, factored, color):
    """backward_raw with the caller's own vR / vt (backward_raw allocates those itself); `pk`: the binding module."""
    L = rast._lib
    inp = rast._inputs(*t, deg, bg)
    cs = rast._camera(camera, Rd, td)
    n, K = inp.n, inp.n_coeffs
    sizes = [4 * n, 3 * n, n, 3 * n, 3 * n] if factored else [4 * n, 3 * n, 3 * K * n, n, 3 * n]
    o = np.cumsum([0] + sizes)
    parts = [arena[o[i]:o[i + 1]] for i in range(5)]
    if factored:
        vrot, vmeans, vopac, vscales, vsh = parts
    else:
        vrot, vmeans, vsh, vopac, vscales = parts
    g = pk.Grads(vmeans.data_ptr(), None if factored else vsh.data_ptr(), vopac.data_ptr(), vscales.data_ptr(), vrot.data_ptr(),
                 None if vR is None else vR.data_ptr(), None if vt is None else vt.data_ptr(),
                 vsh.data_ptr() if factored else None, rast.gstate._grad_means_2d.data_ptr() if n else None,
                 int(rast.stats.generation), pk.GRADS_COLOR_COTANGENT if color else 0, 0)
    pk.check(L.gsr_backward(rast._h, C.byref(inp), C.byref(cs), vp.data_ptr(), C.byref(g), _stream()))
    return [vmeans.view(n, 3), vsh.view(n, 3) if factored else vsh.view(n, K, 3), vopac.view(n, 1), vscales.view(n, 3),
            vrot.view(n, 4)]


def run_view(pkg, sc, fill, *, prec=None, exact=False, budget=0, warm=0, vp=None, loss=False, aux_prior=None,
             forward_only=False, pose=False, factored=False, views=1, check=None):
    """One handle, `views` forwards of the scene (the last one followed by the backward unless forward_only); every buffer the
    call writes is a poisoned (or, clean: zeroed) caller buffer.  Returns the outputs of the last view, cloned."""
    W, H, L = sc.W, sc.H, pkg._lib
    n = sc.means.shape[0]
    t = [dev(sc.means), dev(sc.shs), dev(np.asarray(sc.opac).reshape(-1, 1)), dev(sc.scales), dev(sc.rots)]
    camera = pcam(pkg, sc.cam)
    with debug_fill(fill):
        rast = pkg.rasterizer.GaussianRasterizer(W, H, mode=sc.mode, near_plane=sc.cam.near_plane, far_plane=sc.cam.far_plane,
                                                 exact_tile_cull=exact, bins_budget_bytes=budget, grad_precision=prec,
                                                 form_tuner=False)
        try:
            Cn = rast.channels
            if warm:
                rast.reserve(n, warm)
            rast.gstate.reserve(n)
            poison(rast.gstate._grad_means_2d, fill)
            Rd = td = None
            if pose:
                Rd, td = dev(np.asarray(sc.cam.R, np.float32).T), dev(np.asarray(sc.cam.t, np.float32))
            covis = unc = None
            for v in range(views):
                if v == views - 1:
                    rast.profile(True)
                img = empty(H, W, Cn, fill=fill)
                if aux_prior is not None:
                    covis = dev(aux_prior, torch.uint8)
                    unc = empty(H, W, fill=fill)
                rast.forward_raw(*t, camera, sc.deg, sc.bg, Rd, td, covis, unc, image_out=img, forward_only=forward_only)
            torch.cuda.synchronize()
            s = rast.stats
            out = dict(image=img.clone(), final_T=rast.accum_alpha, n_contrib=rast.n_contrib,
                       stats=(int(s.n_rendered), int(s.compact_binning), tuple(int(x) for x in s.tier_tiles)))
            if aux_prior is not None:
                out["covis"], out["unc"] = covis.clone(), unc.clone()
            if not forward_only:
                if loss:
                    tgt = dev(pkg.synthetic.make_target(W, H, sc.seed))
                    lo, vpx = empty(1, fill=fill), empty(H, W, Cn, fill=fill)
                    L.check(L.load().gsr_loss_l1_ssim(rast._h, img.data_ptr(), tgt.data_ptr(), 0.2, lo.data_ptr(),
                                                      vpx.data_ptr(), _stream()))
                    vpd = vpx
                else:
                    vpd = dev(vp)
                K = sc.shs.shape[1]
                arena = empty((14 if factored else 11 + 3 * K) * n, fill=fill)
                vR = vt = None
                if pose:
                    vR, vt = empty(3, 3, fill=fill), empty(3, fill=fill)
                gr = backward_into(L, rast, vpd, t, camera, sc.deg, sc.bg, Rd, td, arena, vR, vt, factored, loss)
                torch.cuda.synchronize()
                out["grads"] = [x.clone() for x in gr]
                out["vmeans2d"] = rast.gstate.grad_means_2d.clone()
                if loss:
                    out["loss"], out["vpix"] = lo.clone(), vpx.clone()
                if pose:
                    out["vR"], out["vt"] = vR.clone(), vt.clone()
            prof = rast.profile_read()
            rast.profile(False)
            out["route"] = (prof["sort_composite_fwd"][1] > 0, prof["composite_fwd"][1] > 0)
            if check is not None:
                check(rast, out)
            return out
        finally:
            rast.close()


def poisoned_runs(pkg, sc, check=None, **kw):
    """clean, then the two poisoned runs: bit-identical to the clean one, each checked by `check` (the oracle criteria)."""
    clean = run_view(pkg, sc, None, **kw)
    for fill in POISON:
        assert_same(clean, run_view(pkg, sc, fill, check=check, **kw), fill)
    return clean


def oracle_check(st, g, sc, lists=True, vis=None):
    def check(rast, out):
        if lists:
            compare_forward(st, types.SimpleNamespace(rast=rast), out["image"], sc.opac)
        else:
            assert frac_bad(out["image"].cpu().numpy(), st.image, 0.0, 1e-4) <= 1e-4
        if g is not None and "grads" in out:
            compare_backward(g, [x for x in out["grads"]] + [None, None], st.radii > 0)
            assert rel_l2(out["vmeans2d"].cpu().numpy(), g.vmeans2d) <= 1e-4
    return check


# ---------------------------------------------------------------------------------------------------------------------
# a. the path matrix
MATRIX = [(m, z, p, cot) for m in MODES for z in (True, False) for p in (None, "accurate") for cot in ("random", "loss")]
for _m, _z, _p, _cot in MATRIX:
    NAMED |= {main_bwd(CH[_m], _z, _p, _cot == "loss"), fused_fwd(CH[_m], False, True)}


@pytest.mark.parametrize("mode,bg0,prec,cot", MATRIX)
def test_path_matrix(pkg, orc, mode, bg0, prec, cot):
    """Ragged 101x70 view; warm handle (gsr_reserve + a first view: the fused forward); zero / non-zero background; both gradient
    arithmetics; a random cotangent on every channel or the loss head's own (GSR_GRADS_COLOR_COTANGENT)."""
    sc = make(pkg, orc, mode, 2500, 101, 70, 2, 301, (0, 0, 0) if bg0 else (0.3, 0.1, 0.6))
    vp = np.random.default_rng(7).standard_normal((sc.H, sc.W, CH[mode])).astype(np.float32)
    st, _ = oracle(orc, sc)
    # (a fresh handle's first view is binned compactly — its bins start from an estimate — and rendered by the strip kernel:
    #  the second view of a reserved handle is the steady state of a training run)
    kw = dict(prec=prec, warm=2 * st.n_rendered + 64, vp=vp, loss=cot == "loss", views=2)
    clean = run_view(pkg, sc, None, **kw)
    # routing: the main backward only (no tier tile), the fused forward for every tile
    assert clean["stats"][1:] == (0, (0, 0, 0)) and clean["route"] == (True, False), (clean["stats"], clean["route"])
    assert (sc.bg == (0.0, 0.0, 0.0)) == bg0
    vpo = clean["vpix"].cpu().numpy() if cot == "loss" else vp
    if cot == "loss":
        assert mode == "rgb" or not clean["vpix"][:, :, 3:].view(torch.int32).any()
    _, g = oracle(orc, sc, vpo)
    for fill in POISON:
        assert_same(clean, run_view(pkg, sc, fill, check=oracle_check(st, g, sc), **kw), fill)


def _hot_scene(pkg, orc, mode, bg0):
    """Three hot tiles, one per tier list: (1024, 4096], (4096, 8192] and > 8192 instances (test_gpu_parity.py's
    test_backward_of_long_lists_... construction, once per tile), next to ordinary tiles."""
    W, H, deg, n = 96, 64, 1, 600
    base = pkg.synthetic.make_scene(n, W, H, deg, 55, sigma_px=3.0)
    rng = np.random.default_rng(56)
    parts = [base]
    opac, scales = [base.opacities], [base.scales]
    for k, (n_hot, x0, y0) in enumerate(((1500, 0, 0), (5000, 32, 16), (16000, 64, 32))):
        hot = pkg.synthetic.make_scene(n_hot, W, H, deg, 57 + k, sigma_px=2.0)
        z = rng.uniform(2.0, 9.0, n_hot)
        u = rng.uniform(x0 + 1.0, x0 + 14.0, n_hot) - W / 2.0
        v = rng.uniform(y0 + 1.0, y0 + 14.0, n_hot) - H / 2.0
        hot.means[:] = np.stack([u * z / base.focal[0], v * z / base.focal[1], z], 1).astype(np.float32)
        scales.append(hot.scales * 0.5)
        parts.append(hot)
        opac.append(np.full(n_hot, 0.004 + 40.0 / n_hot, np.float32))
    cat = lambda f: np.concatenate([getattr(p, f) for p in parts])  # noqa: E731
    cam = orc.Camera(W, H, base.focal)
    return Scene(means=cat("means"), shs=cat("shs"), opac=np.concatenate(opac), scales=np.concatenate(scales), rots=cat("rotations"),
                 cam=cam, deg=deg, bg=(0.0, 0.0, 0.0) if bg0 else (0.2, 0.4, 0.1), mode=mode, W=W, H=H, seed=58)


_HOT_ORACLE = {}
HOT = [(m, z, p) for m in MODES for z in (True, False) for p in (None, "accurate")]
for _m, _z, _p in HOT:
    NAMED |= {long_bwd(CH[_m], _z) if _p is None else main_bwd(CH[_m], _z, _p, False), strip_fwd(CH[_m], False)}


@pytest.mark.parametrize("mode,bg0,prec", HOT)
def test_hot_tiles_in_all_three_tiers(pkg, orc, mode, bg0, prec):
    """Default precision: the tier tiles go to composite_bwd_long_kernel (PASS 2 zeroes their rows behind the last
    contributor); accurate: the same lists through the main kernel."""
    sc = _hot_scene(pkg, orc, mode, bg0)
    vp = np.random.default_rng(58).standard_normal((sc.H, sc.W, CH[mode])).astype(np.float32)
    key = (mode, bg0)
    if key not in _HOT_ORACLE:
        _HOT_ORACLE[key] = oracle(orc, sc, vp)
    st, g = _HOT_ORACLE[key]
    clean = run_view(pkg, sc, None, prec=prec, vp=vp)
    assert all(x > 0 for x in clean["stats"][2]), clean["stats"]  # a tile in each tier list
    # ... and the backward splits them off to the long kernel (default precision; accurate handles split nothing): the
    # policy function launch_composite_bwd calls, on the handle's default configuration and this view's tier counts
    L = pkg._lib
    cfg, sp = L.PolicyConfig(), L.BwdSplit()
    L.load().gsr_policy_config_init(C.byref(cfg), sc.W, sc.H, 0, -1)
    L.load().gsr_policy_bwd_split(C.byref(cfg), *clean["stats"][2], C.byref(sp))
    assert (sp.n_mid4, sp.n_mid8, sp.n_big) == clean["stats"][2], (sp.n_mid4, sp.n_mid8, sp.n_big)
    assert clean["route"][1]  # the strip forward (cold handle: every tile)
    for fill in POISON:
        assert_same(clean, run_view(pkg, sc, fill, prec=prec, vp=vp, check=oracle_check(st, g, sc)), fill)


NAMED |= {main_bwd(3, False, None, False)}


@pytest.mark.parametrize("prec", [None, "accurate"])
def test_large_rects_under_exact_cull(pkg, orc, prec):
    """Footprints of more than GSR_DENSE_RECT (32) tiles under exact culling: one row slot per tile of the rect, the culled
    tiles' slots never written nor read (preprocess.hip, pergauss.hip)."""
    sc = make(pkg, orc, "rgb", 1500, 320, 208, 1, 61, (0.1, 0.2, 0.3), sigma_px=45.0, view=0)
    vp = np.random.default_rng(3).standard_normal((sc.H, sc.W, 3)).astype(np.float32)
    st, g = oracle(orc, sc, vp)
    tiles = st.tiles_touched
    assert (tiles > 32).sum() > 100

    def check(rast, out):
        rect = rast.geometry()["rect"].cpu().numpy().astype(np.int64)
        area = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
        assert ((area > 32) & (st.radii > 0)).sum() > 100
        assert out["stats"][0] < st.n_rendered  # exact culling dropped instances of those rects
        oracle_check(st, g, sc, lists=False)(rast, out)

    poisoned_runs(pkg, sc, check=check, exact=True, prec=prec, vp=vp)


NAMED |= {strip_fwd(3, False)}


def test_compact_binning_1(pkg, orc):
    sc = make(pkg, orc, "rgb", 2500, 101, 70, 2, 303, (0.3, 0.1, 0.6))
    vp = np.random.default_rng(5).standard_normal((sc.H, sc.W, 3)).astype(np.float32)
    st, g = oracle(orc, sc, vp)
    clean = poisoned_runs(pkg, sc, check=oracle_check(st, g, sc), budget=1, vp=vp, warm=2 * st.n_rendered)
    assert clean["stats"][1] == 1 and clean["route"] == (False, True)


def test_compact_binning_2(pkg):
    """Bins of 1536 keys, lists far longer: the second view stays in its bins, the overflow lists are scattered again."""
    W, H, n, deg = 640, 416, 30000, 1
    s = pkg.synthetic.make_scene(n, W, H, deg, 67)
    for i, k in enumerate(("dense:0.01:70", "dense:0.005:190", "hot:9000")):
        s = pkg.synthetic.add_skew(s, k, seed=68 + i)
    from oracle import oracle as orc
    sc = Scene(means=s.means, shs=s.shs, opac=s.opacities, scales=s.scales, rots=s.rotations, cam=orc.Camera(W, H, s.focal),
               deg=deg, bg=(0.0, 0.0, 0.0), mode="rgb", W=W, H=H, seed=69)
    vp = np.random.default_rng(5).standard_normal((H, W, 3)).astype(np.float32)
    clean = poisoned_runs(pkg, sc, budget=(40 * 26 + 1) * 8 * 1536, vp=vp, views=2)
    assert clean["stats"][1] == 2 and sum(clean["stats"][2]) > 0, clean["stats"]


AUXC = [(m, w) for m in MODES for w in (False, True)]
for _m, _w in AUXC:
    NAMED |= {fused_fwd(CH[_m], True, True) if _w else strip_fwd(CH[_m], True)}


@pytest.mark.parametrize("mode,warm", AUXC)
def test_covisibilities_and_uncertainties(pkg, orc, mode, warm):
    """gsr_aux: uncertainties are fully overwritten (gsr.h); covisibilities are only ever SET (prior | this view)."""
    sc = make(pkg, orc, mode, 2000, 101, 70, 0, 305, (0.2, 0.2, 0.2))
    vp = np.random.default_rng(6).standard_normal((sc.H, sc.W, CH[mode])).astype(np.float32)
    n = sc.means.shape[0]
    st, g = oracle(orc, sc, vp, aux=True)
    kw = dict(vp=vp, warm=(2 * st.n_rendered if warm else 0), views=2 if warm else 1)
    clean = run_view(pkg, sc, None, aux_prior=np.zeros(n, np.uint8), **kw)
    assert clean["route"] == (warm, not warm)
    assert (clean["covis"].cpu().numpy() != st.covisibilities).mean() <= 5e-3
    assert frac_bad(clean["unc"].cpu().numpy(), st.uncertainties, 0, 1e-4) <= 1e-4
    prior = np.random.default_rng(8).integers(0, 2, n).astype(np.uint8)
    for fill in POISON:
        p = run_view(pkg, sc, fill, aux_prior=prior, check=oracle_check(st, g, sc), **kw)
        assert torch.equal(p.pop("covis"), clean["covis"] | dev(prior, torch.uint8))
        assert_same({k: v for k, v in clean.items() if k != "covis"}, p, fill)


FWDONLY = [(m, a) for m in MODES for a in (False, True)]
for _m, _a in FWDONLY:
    NAMED |= {fused_fwd(CH[_m], _a, False)}


@pytest.mark.parametrize("mode,aux", FWDONLY)
def test_forward_only(pkg, orc, mode, aux):
    sc = make(pkg, orc, mode, 2000, 101, 70, 1, 307, (0.0, 0.0, 0.0))
    n = sc.means.shape[0]
    st, _ = oracle(orc, sc, aux=aux)
    kw = dict(forward_only=True, aux_prior=np.zeros(n, np.uint8) if aux else None, views=2)
    clean = poisoned_runs(pkg, sc, check=oracle_check(st, None, sc, lists=False), **kw)
    assert clean["route"] == (True, False)
    train = run_view(pkg, sc, "nan", vp=np.zeros((sc.H, sc.W, CH[mode]), np.float32), aux_prior=kw["aux_prior"])
    same_bits(clean["image"], train["image"], "forward-only image == training image")


def test_pose_gradients(pkg, orc):
    sc = make(pkg, orc, "rgbd", 2000, 101, 70, 2, 309, (0.0, 0.0, 0.0), view=1)
    vp = np.random.default_rng(3).standard_normal((sc.H, sc.W, 5)).astype(np.float32)
    st, g = oracle(orc, sc, vp, pose=True)

    def check(rast, out):
        oracle_check(st, g, sc)(rast, out)
        assert rel_l2(out["vR"].cpu().numpy().reshape(-1), g.vR) <= 1e-4
        assert rel_l2(out["vt"].cpu().numpy(), g.vt) <= 1e-4

    # vR / vt are float atomics over the Gaussians (pergauss.hip): their last bits follow the arrival order, so they are held
    # to the clean run within reassociation (relative L2 over the 9 / 3 values, robust to an element that cancels to ~0) and
    # must be finite; everything else is bit-identical
    kw = dict(vp=vp, pose=True)
    clean = run_view(pkg, sc, None, **kw)
    pose_clean = {k: clean.pop(k) for k in ("vR", "vt")}
    for fill in POISON:
        p = run_view(pkg, sc, fill, check=check, **kw)
        for k, a in pose_clean.items():
            b = p.pop(k)
            assert torch.isfinite(b).all() and rel_l2(b.cpu().numpy(), a.cpu().numpy()) <= 1e-5, (k, fill)
        assert_same(clean, p, fill)


def test_factored_sh_and_sh_grad_from_views(pkg, orc):
    """gsr_grads.vcolors (vshs not written), and gsr_sh_grad_from_views into a poisoned (N,K,3): V = 1 == the unfactored vshs."""
    sc = make(pkg, orc, "rgb", 2000, 101, 70, 3, 311, (0.1, 0.1, 0.1))
    vp = np.random.default_rng(4).standard_normal((sc.H, sc.W, 3)).astype(np.float32)
    full = run_view(pkg, sc, None, vp=vp)
    clean = poisoned_runs(pkg, sc, vp=vp, factored=True)
    n, K = sc.shs.shape[0], sc.shs.shape[1]
    cc = dev(np.asarray(pcam(pkg, sc.cam).camera_center, np.float32).reshape(1, 3))
    for fill in (None,) + POISON:
        out = empty(n, K, 3, fill=fill)
        pkg.rasterizer.sh_grad_from_views(dev(sc.means), clean["grads"][1][None].contiguous(), cc, K, sc.deg, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, full["grads"][1]), fill  # (== as in test_gpu_parity: a culled Gaussian's zero may carry a sign)
        if fill is None:
            ref = out
        else:
            same_bits(out, ref, f"sh_grad_from_views [{fill}]")


def test_k_padded_sh_bands_come_back_as_zeros(pkg, orc):
    sc = make(pkg, orc, "rgb", 1500, 101, 70, 1, 313, (0.0, 0.0, 0.0), K=16)
    vp = np.random.default_rng(5).standard_normal((sc.H, sc.W, 3)).astype(np.float32)
    st, g = oracle(orc, sc, vp)
    clean = poisoned_runs(pkg, sc, check=oracle_check(st, g, sc), vp=vp)
    assert not clean["grads"][1][:, 4:, :].view(torch.int32).any()


def test_nothing_visible_and_empty_scene(pkg, orc):
    """D = 0: all-zero image, T, n_contrib, uncertainties (gsr.h) and zero gradients, whatever the buffers held."""
    sc = make(pkg, orc, "rgbdn", 300, 101, 70, 1, 315, (1.0, 1.0, 1.0))
    sc.means = sc.means.copy()
    sc.means[:, 2] = -3.0
    vp = np.ones((sc.H, sc.W, 8), np.float32)
    n = sc.means.shape[0]
    clean = poisoned_runs(pkg, sc, vp=vp, aux_prior=np.ones(n, np.uint8))
    assert clean["stats"][0] == 0
    for k in ("image", "final_T", "unc"):
        assert not clean[k].view(torch.int32).any(), k
    assert all(not x.view(torch.int32).any() for x in clean["grads"] + [clean["vmeans2d"]])
    e = np.zeros((0, 3), np.float32)
    sc0 = Scene(means=e, shs=np.zeros((0, 4, 3), np.float32), opac=np.zeros(0, np.float32), scales=e,
                rots=np.zeros((0, 4), np.float32), cam=sc.cam, deg=1, bg=(1.0, 0.0, 0.0), mode="rgb", W=sc.W, H=sc.H, seed=1)
    clean0 = poisoned_runs(pkg, sc0, vp=np.ones((sc.H, sc.W, 3), np.float32))
    assert not clean0["image"].view(torch.int32).any()


TAIL = [("rgb", False), ("rgbd", True), ("rgbdn", False)]


@pytest.mark.parametrize("mode,color", TAIL)
def test_backward_trainer_tail(pkg, mode, color):
    """gsr_backward_trainer_tail (pergauss_bwd_kernel's FUSED instantiations): parameters, moments, activated copies and
    gstate.∇means_2d after two steps are the clean run's, bit for bit; culled Gaussians included."""
    W, H, n, deg = 101, 70, 1500, 2
    s = pkg.synthetic.make_scene(n, W, H, deg, 77, sigma_px=5.0)
    s.means[::7, 2] = -1.0
    cam = pkg.Camera(W, H, tuple(s.focal))
    R, O = pkg.rasterizer, pkg.optim
    Cn = CH[mode]
    target = dev(np.random.default_rng(3).uniform(0, 1, (3, H, W)).astype(np.float32))

    def run(fill):
        with debug_fill(fill):
            raw = dict(points=dev(s.means), features_dc=dev(s.shs[:, :1].copy()), features_rest=dev(s.shs[:, 1:].copy()),
                       opacities=dev(s.opacities_raw.reshape(-1, 1)), scales=dev(s.scales_raw), rotations=dev(s.rotations))
            opts = {k: O.Adam(raw[k], 1e-3, eps=1e-15) for k in O.GROUPS}
            act = list(R.prologue_forward(raw["features_dc"], raw["features_rest"], raw["opacities"], raw["scales"]))
            rast = R.GaussianRasterizer(W, H, mode=mode, form_tuner=False)
            rast.gstate.reserve(n)
            poison(rast.gstate._grad_means_2d, fill)
            losses = []
            for _ in range(2):
                img = rast.forward_raw(raw["points"], *act, raw["rotations"], cam, deg, (0.0, 0.0, 0.0),
                                       image_out=empty(H, W, Cn, fill=fill))
                # the loss head into pre-filled loss / cotangent buffers (the fused_ssim wrapper allocates its own)
                lo, vp = empty(1, fill=fill), empty(H, W, Cn, fill=fill)
                pkg._lib.check(pkg._lib.load().gsr_loss_l1_ssim(rast._h, img.data_ptr(), target.data_ptr(), 0.2, lo.data_ptr(),
                                                                vp.data_ptr(), _stream()))
                losses.append(lo.clone())
                O.fused_backward_tail_step(rast, vp, opts, raw, *act, cam, deg, (0.0, 0.0, 0.0),
                                           forward_generation=rast.stats.generation, color_cotangent=color)
            torch.cuda.synchronize()
            out = dict(raw=[raw[k].clone() for k in O.GROUPS], mu=[opts[k].mu.clone() for k in O.GROUPS],
                       nu=[opts[k].nu.clone() for k in O.GROUPS], act=[a.clone() for a in act],
                       vmeans2d=rast.gstate.grad_means_2d.clone(), loss=losses, vpix=vp.clone())
            rast.close()
            return out

    clean = run(None)
    assert not torch.equal(clean["raw"][0], dev(s.means))
    for fill in POISON:
        assert_same(clean, run(fill), fill)


def test_every_instantiation_is_named_by_a_cell(pkg):
    built = compiled_kernels(pkg._lib.LIB_PATH)
    assert len(built) >= 36, sorted(built)  # 12 main + 6 long backward, 12 fused + 6 strip forward today
    assert built <= NAMED, sorted(built - NAMED)  # an instantiation added to composite.hip needs a cell that routes to it
    assert NAMED <= built, sorted(NAMED - built)


# ---------------------------------------------------------------------------------------------------------------------
# b. stateless entry points: outputs the same whatever they held before
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 5, 7), (2, 3, 17, 33), (1, 3, 1, 40)])
def test_ssim_planar_forward_and_backward(pkg, shape, exact):
    lib = pkg._lib.load()
    rng = np.random.default_rng(sum(shape))
    B, CHn, H, W = shape
    img, ref, dmap = (dev(rng.uniform(0, 1, shape).astype(np.float32)) for _ in range(3))
    res = {}
    with pkg.fused_ssim.exact_arithmetic(exact):
        for fill in (None,) + POISON:
            m, d0, d1, d2, gi = (empty(*shape, fill=fill) for _ in range(5))
            pkg._lib.check(lib.gsr_ssim_forward(W, H, CHn, B, img.data_ptr(), ref.data_ptr(), 0.01 ** 2, 0.03 ** 2, 1,
                                                m.data_ptr(), d0.data_ptr(), d1.data_ptr(), d2.data_ptr(), _stream()))
            pkg._lib.check(lib.gsr_ssim_backward(W, H, CHn, B, img.data_ptr(), ref.data_ptr(), dmap.data_ptr(), d0.data_ptr(),
                                                 d1.data_ptr(), d2.data_ptr(), gi.data_ptr(), _stream()))
            torch.cuda.synchronize()
            res[fill] = dict(m=m, d0=d0, d1=d1, d2=d2, grad=gi)
    assert torch.isfinite(res[None]["m"]).all() and torch.isfinite(res[None]["grad"]).all()
    for fill in POISON:
        assert_same(res[None], res[fill], fill)


@pytest.mark.parametrize("prec", ["fast", "exact"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", [(17, 9), (33, 1)])
def test_loss_head(pkg, orc, W, H, mode, prec):
    """gsr_loss_l1_ssim: fewer tiles than the XCD-aware grid's 8 lanes (padding workgroups write zero partials, the finisher
    sums them); channels >= 3 of vpixels are exact zeros."""
    rng = np.random.default_rng(W * H)
    Cn = CH[mode]
    img = rng.uniform(0, 1, (H, W, Cn)).astype(np.float32)
    tgt = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    L = pkg._lib
    res = {}
    for fill in (None,) + POISON:
        with debug_fill(fill):
            rast = pkg.rasterizer.GaussianRasterizer(W, H, mode=mode, ssim_precision=prec)
            lo, vpx = empty(1, fill=fill), empty(H, W, Cn, fill=fill)
            di, dt = dev(img), dev(tgt)
            L.check(L.load().gsr_loss_l1_ssim(rast._h, di.data_ptr(), dt.data_ptr(), 0.2, lo.data_ptr(), vpx.data_ptr(),
                                              _stream()))
            torch.cuda.synchronize()
            res[fill] = dict(loss=lo.clone(), vpix=vpx.clone())
            rast.close()
    assert not res[None]["vpix"][:, :, 3:].view(torch.int32).any()
    loss_o, vp_o = orc.loss_head(np.ascontiguousarray(img[:, :, :3]), tgt)
    assert abs(float(res[None]["loss"]) - float(loss_o)) < 1e-5
    assert rel_l2(res[None]["vpix"][:, :, :3].cpu().numpy(), vp_o) <= 1e-4
    for fill in POISON:
        assert_same(res[None], res[fill], fill)


def test_prologue_forward_and_backward(pkg):
    L = pkg._lib
    lib = L.load()
    n, kr = 1000, 15
    rng = np.random.default_rng(9)
    dc, rest = dev(rng.standard_normal((n, 1, 3)).astype(np.float32)), dev(rng.standard_normal((n, kr, 3)).astype(np.float32))
    op, sc = dev(rng.standard_normal((n, 1)).astype(np.float32)), dev(rng.standard_normal((n, 3)).astype(np.float32) - 3)
    vshs, vo, vs = (dev(rng.standard_normal(s).astype(np.float32)) for s in ((n, kr + 1, 3), (n, 1), (n, 3)))
    res = {}
    for fill in (None,) + POISON:
        shs, oa, sa = empty(n, kr + 1, 3, fill=fill), empty(n, 1, fill=fill), empty(n, 3, fill=fill)
        L.check(lib.gsr_prologue_forward(n, kr, 3, dc.data_ptr(), rest.data_ptr(), op.data_ptr(), sc.data_ptr(),
                                         shs.data_ptr(), oa.data_ptr(), sa.data_ptr(), _stream()))
        vdc, vrest, vop, vsc = empty(n, 1, 3, fill=fill), empty(n, kr, 3, fill=fill), empty(n, 1, fill=fill), empty(n, 3, fill=fill)
        L.check(lib.gsr_prologue_backward(n, kr, 3, oa.data_ptr(), sa.data_ptr(), vshs.data_ptr(), vo.data_ptr(), vs.data_ptr(),
                                          vdc.data_ptr(), vrest.data_ptr(), vop.data_ptr(), vsc.data_ptr(), _stream()))
        torch.cuda.synchronize()
        res[fill] = dict(shs=shs, oa=oa, sa=sa, vdc=vdc, vrest=vrest, vo=vop, vs=vsc)
    for fill in POISON:
        assert_same(res[None], res[fill], fill)


def _same_whatever_the_fill(run):
    """run(fill) -> dict of outputs written into buffers pre-filled with `fill` (None: zeros); all three must agree."""
    res = {fill: run(fill) for fill in (None,) + POISON}
    for fill in POISON:
        assert_same(res[None], res[fill], fill)
    return res[None]


def _scratch_bytes(nbytes, fill):
    """A caller-owned scratch buffer of at least nbytes, as uint8 (the bindings' type), pre-filled word by word."""
    return empty((int(nbytes) + 7) // 4, fill=fill).view(torch.uint8)


def test_sh_grad_from_views_tail(pkg):
    """gsr_sh_grad_from_views_tail: θ, μ, ν are updated from themselves and the activated opacities / scales are read (the
    prologue pullback), so what can hold garbage beforehand is the activated SH copy (written, never read) and small->vshs
    (documented unread).  Both are pre-filled; θ, μ, ν and the activated copies must be the clean run's, bit for bit."""
    r = np.random.default_rng(43)
    n, kr, V, deg = 1031, 15, 3, 3
    O, R, L = pkg.optim, pkg.rasterizer, pkg._lib
    shapes = dict(points=(n, 3), features_dc=(n, 1, 3), features_rest=(n, kr, 3), opacities=(n, 1), scales=(n, 3), rotations=(n, 4))
    host = {k: r.normal(size=sh).astype(np.float32) for k, sh in shapes.items()}
    host["points"][:, 2] += 6.0
    centers = dev(r.normal(size=(V, 3)).astype(np.float32))
    vc = r.normal(size=(V, n, 3)).astype(np.float32)
    vc[r.random((V, n)) < 0.2] = 0.0
    small = {k: dev(r.normal(size=sh).astype(np.float32)) for k, sh in (("vmeans", (n, 3)), ("vopacities", (n, 1)),
                                                                         ("vscales", (n, 3)), ("vrot", (n, 4)))}

    def run(fill):
        raw = {k: dev(v) for k, v in host.items()}
        opts = {k: O.Adam(raw[k], 1e-3, eps=1e-15) for k in O.GROUPS}
        act = list(R.prologue_forward(raw["features_dc"], raw["features_rest"], raw["opacities"], raw["scales"]))
        poison(act[0], fill)
        unread = empty(n, 1 + kr, 3, fill=fill)
        st, _ = O.tail_state(opts, raw, *act)
        tg = L.TailGrads(small["vmeans"].data_ptr(), unread.data_ptr(), small["vopacities"].data_ptr(),
                         small["vscales"].data_ptr(), small["vrot"].data_ptr())
        vcd = dev(vc)
        L.check(L.load().gsr_sh_grad_from_views_tail(n, 1 + kr, deg, V, centers.data_ptr(), vcd.data_ptr(), C.byref(tg),
                                                     C.byref(st), _stream()))
        torch.cuda.synchronize()
        return dict(raw=[raw[k].clone() for k in O.GROUPS], mu=[opts[k].mu.clone() for k in O.GROUPS],
                    nu=[opts[k].nu.clone() for k in O.GROUPS], act=[a.clone() for a in act])

    clean = _same_whatever_the_fill(run)
    assert not torch.equal(clean["raw"][1], dev(host["features_dc"]))


def test_ply_pack_and_unpack_rows(pkg):
    """gsr_ply_pack_rows into a pre-filled row matrix (the normal columns included), gsr_ply_unpack_rows into pre-filled
    arrays: the round trip returns the model bit for bit."""
    L = pkg._lib
    n, kr = 1000, 15
    rng = np.random.default_rng(12)
    src = [dev(rng.normal(size=sh).astype(np.float32)) for sh in ((n, 3), (n, 1, 3), (n, kr, 3), (n, 1), (n, 3), (n, 4))]

    def run(fill):
        rows = empty(n, 17 + 3 * kr, fill=fill)
        L.check(L.load().gsr_ply_pack_rows(n, kr, *[t.data_ptr() for t in src], rows.data_ptr(), _stream()))
        back = [empty(*t.shape, fill=fill) for t in src]
        L.check(L.load().gsr_ply_unpack_rows(n, kr, rows.data_ptr(), *[t.data_ptr() for t in back], _stream()))
        torch.cuda.synchronize()
        return dict(rows=rows, back=back)

    clean = _same_whatever_the_fill(run)
    assert not clean["rows"][:, 3:6].view(torch.int32).any()
    assert all(torch.equal(a, b) for a, b in zip(clean["back"], src))


def test_gather_and_compose_row_destinations(pkg):
    """gsr_gather_rows / gsr_compose_rows (densification's row surgery) into pre-filled destinations: kept rows, copied
    selections (two repetitions, as a split) and the zero rows of the Adam moments (new_zero)."""
    L = pkg._lib
    n, words = 3000, (3, 1, 48, 4)
    rng = np.random.default_rng(13)
    src = [dev(rng.normal(size=(n, w)).astype(np.float32)) for w in words]
    keep = np.sort(rng.choice(n, 2000, replace=False)).astype(np.uint32)
    sel = np.sort(rng.choice(n, 300, replace=False)).astype(np.uint32)
    kd, sd = dev(keep, torch.int32), dev(sel, torch.int32)

    def run(fill):
        gdst = [empty(len(keep), w, fill=fill) for w in words]
        gg = (L.GatherGroup * len(words))(*[L.GatherGroup(s.data_ptr(), d.data_ptr(), w) for s, d, w in zip(src, gdst, words)])
        L.check(L.load().gsr_gather_rows(gg, len(words), kd.data_ptr(), len(keep), _stream()))
        cdst = [empty(len(keep) + 2 * len(sel), w, fill=fill) for w in words]
        cg = (L.ComposeGroup * len(words))(*[L.ComposeGroup(s.data_ptr(), d.data_ptr(), w, int(k % 2 == 1))
                                            for k, (s, d, w) in enumerate(zip(src, cdst, words))])
        L.check(L.load().gsr_compose_rows(cg, len(words), kd.data_ptr(), len(keep), sd.data_ptr(), len(sel), 2, _stream()))
        torch.cuda.synchronize()
        return dict(gather=gdst, compose=cdst)

    clean = _same_whatever_the_fill(run)
    kl, sl = torch.as_tensor(keep.astype(np.int64)).cuda(), torch.as_tensor(sel.astype(np.int64)).cuda()
    for k, (s_, g_, c_) in enumerate(zip(src, clean["gather"], clean["compose"])):
        assert torch.equal(g_, s_[kl]) and torch.equal(c_[:len(keep)], s_[kl])
        tail = c_[len(keep):]
        assert (not tail.view(torch.int32).any()) if k % 2 == 1 else torch.equal(tail, s_[sl].repeat(2, 1))


@pytest.mark.parametrize("channels", [3, 5])
def test_bilateral_slice_tv_and_adam_tail(pkg, channels):
    """The bilateral grid's entry points with every output AND their caller-owned scratch (float per-workgroup partials,
    gsr_ops.cpp) pre-filled: slice forward, its pullback into a separate vimage, TV loss and gradient, the fused TV + Adam
    tail (the grids, moments, ∇grid and TV term it leaves)."""
    B, L = pkg.bilateral_grid, pkg._lib
    lib = L.load()
    H, W, nimg, (gx, gy, gz) = 45, 70, 3, (8, 6, 4)
    rng = np.random.default_rng(14)
    image = dev(rng.uniform(0, 1, (H, W, channels)).astype(np.float32))
    vout = dev(rng.normal(size=(H, W, channels)).astype(np.float32))
    grids0 = np.zeros((nimg, 12, gz, gy, gx), np.float32)
    for d in range(3):
        grids0[:, d * 4 + d] = 1.0
    grids0 += rng.normal(scale=0.05, size=grids0.shape).astype(np.float32)
    nb_slice = lib.gsr_bilateral_scratch_bytes(W, H, gx, gy, gz)
    nb_tv = lib.gsr_bilateral_tv_scratch_bytes(nimg)

    def run(fill):
        grids = dev(grids0)
        out = B.slice_forward(image, grids[1], out=empty(H, W, channels, fill=fill))
        scratch = {"slice": _scratch_bytes(nb_slice, fill), "tv": _scratch_bytes(nb_tv, fill)}
        vimage, vgrid = B.slice_backward(image, grids[1], vout, vimage=empty(H, W, channels, fill=fill),
                                         vgrid=empty(12, gz, gy, gx, fill=fill), scratch=scratch)
        loss, g = empty(1, fill=fill), empty(*grids.shape, fill=fill)
        buf = _scratch_bytes(nb_tv, fill)
        L.check(lib.gsr_bilateral_tv(nimg, gx, gy, gz, grids.data_ptr(), 10.0, loss.data_ptr(), g.data_ptr(), buf.data_ptr(),
                                     buf.numel(), _stream()))
        bg = B.BilateralGrid(nimg, size=(gx, gy, gz))
        bg.grids.copy_(grids)
        bg._scratch = {"slice": _scratch_bytes(nb_slice, fill), "tv": _scratch_bytes(nb_tv, fill)}
        poison(bg.vgrid, fill)
        poison(bg.tv_term, fill)
        vo = vout.clone()
        bg.slice_backward_(image, 1, vo)
        term = bg.step(1, trainer_step=10).clone()
        torch.cuda.synchronize()
        return dict(out=out, vimage=vimage, vgrid=vgrid, loss=loss, tv_grad=g, vo=vo, grids=bg.grids.clone(),
                    mu=bg.optimizer.mu.clone(), nu=bg.optimizer.nu.clone(), tv_term=term)

    clean = _same_whatever_the_fill(run)
    assert torch.isfinite(clean["loss"]).all() and torch.isfinite(clean["vgrid"]).all() and torch.isfinite(clean["grids"]).all()
    if channels > 3:
        assert torch.equal(clean["out"][:, :, 3:], image[:, :, 3:]) and torch.equal(clean["vimage"][:, :, 3:], vout[:, :, 3:])


# ---------------------------------------------------------------------------------------------------------------------
# c. stale state: view A, then view B on the same handle == B on a fresh handle (index, key and count buffers included).
# form_tuner=False everywhere: the tuner times views (a wall-clock decision); the binning forms give identical results, but
# a pinned form keeps the sequence deterministic.
def _seq(pkg, views, **kw):
    """[(scene, forward_only, vp)] on one handle; the outputs of the last view."""
    last = views[-1][0]
    rast = pkg.rasterizer.GaussianRasterizer(last.W, last.H, mode=last.mode, form_tuner=False, **kw)
    try:
        for sc, fwd_only, vp, release in views:
            if release:
                rast.release_scene_buffers()
            n = sc.means.shape[0]
            t = [dev(sc.means), dev(sc.shs), dev(np.asarray(sc.opac).reshape(-1, 1)), dev(sc.scales), dev(sc.rots)]
            camera = pcam(pkg, sc.cam)
            img = rast.forward_raw(*t, camera, sc.deg, sc.bg, image_out=empty(sc.H, sc.W, rast.channels, fill="nan"),
                                   forward_only=fwd_only)
            out = dict(image=img.clone(), final_T=rast.accum_alpha, n_contrib=rast.n_contrib)
            if not fwd_only:
                g = rast.backward_raw(dev(vp), *t, camera, sc.deg, sc.bg, arena=empty((11 + 3 * sc.shs.shape[1]) * n, fill="nan"))
                out["grads"] = [x.clone() for x in g[:5]]
                out["vmeans2d"] = rast.gstate.grad_means_2d.clone()
                if rast.stats.n_rendered:
                    out["ranges"], out["ids"] = rast.ranges, rast.values_sorted
            torch.cuda.synchronize()
        return out
    finally:
        rast.close()


def _vp(sc, seed=11):
    return np.random.default_rng(seed).standard_normal((sc.H, sc.W, CH[sc.mode])).astype(np.float32)


@pytest.mark.parametrize("prec", [None, "accurate"])
def test_stale_long_lists_then_ordinary(pkg, orc, prec):
    a = _hot_scene(pkg, orc, "rgbd", False)
    b = make(pkg, orc, "rgbd", 600, 96, 64, 1, 321, a.bg, sigma_px=3.0, view=0)
    fresh = _seq(pkg, [(b, False, _vp(b), False)], grad_precision=prec)
    assert_same(fresh, _seq(pkg, [(a, False, _vp(a), False), (b, False, _vp(b), False)], grad_precision=prec), "after A")


def test_stale_large_then_small_n(pkg, orc):
    a = make(pkg, orc, "rgbdn", 12000, 101, 70, 2, 323, (0.1, 0.2, 0.3), sigma_px=5.0)
    b = make(pkg, orc, "rgbdn", 700, 101, 70, 2, 325, (0.1, 0.2, 0.3))
    fresh = _seq(pkg, [(b, False, _vp(b), False)])
    assert_same(fresh, _seq(pkg, [(a, False, _vp(a), False), (b, False, _vp(b), False)]), "after A")


def test_stale_forward_only_then_training(pkg, orc):
    b = make(pkg, orc, "rgb", 2000, 101, 70, 3, 327, (0.0, 0.0, 0.0))
    fresh = _seq(pkg, [(b, False, _vp(b), False)])
    assert_same(fresh, _seq(pkg, [(b, True, None, False), (b, False, _vp(b), False)]), "after forward-only")


def test_stale_nothing_visible_then_normal(pkg, orc):
    b = make(pkg, orc, "rgbd", 2000, 101, 70, 1, 329, (0.5, 0.5, 0.5))
    a = Scene(**vars(b))
    a.means = b.means.copy()
    a.means[:, 2] = -3.0
    fresh = _seq(pkg, [(b, False, _vp(b), False)])
    assert_same(fresh, _seq(pkg, [(a, False, _vp(a), False), (b, False, _vp(b), False)]), "after an empty view")


def test_stale_release_scene_buffers_then_same_view(pkg, orc):
    b = make(pkg, orc, "rgb", 2000, 101, 70, 2, 331, (0.0, 0.0, 0.0))
    fresh = _seq(pkg, [(b, False, _vp(b), False)])
    assert_same(fresh, _seq(pkg, [(b, False, _vp(b), False), (b, False, _vp(b), True)]), "after release")
