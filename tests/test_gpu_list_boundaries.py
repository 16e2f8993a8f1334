"""-m gpu: tile lists of a CHOSEN length on every boundary at which a kernel changes path.

One 16 x 16 tile, reference-list mode: the list length is the Gaussian count (tests/list_scenes.py; its premises are held on
the oracle alone by tests/test_list_scenes_cpu.py).  Lengths sit on and one past
  * the one-wave sort's classes (64 .. 1024), the run edges of the LDS sorts (2048 .. 8192), the chunk / merge-pass edges of
    the longer sorts (8193, 12289, 16385, 32769) — tile_sort_device.h, binning.hip;
  * the fused sort-and-forward kernel's 256-entry LDS chunks and its 1024-entry cut, the tier launches — composite.hip;
  * the one-wave backward's 64-entry batches, the split length (always 1024 on a one-tile view: gsr_policy_bwd_split cuts at
    the lowest tier while the tiles are few; an accurate handle splits nothing) and the 32 segments of composite_bwd_long_kernel
    (tile_last = 2048: 32 full segments; 2049: a seventeenth segment of ONE entry) — composite.hip;
  * the key bins' capacity (cap - 1, cap, cap + 1 keys) — gsr_policy.cpp.
Criteria: compare_forward / compare_backward of hip_helpers, unchanged; n_contrib equal to the oracle's at EVERY pixel (the
builders keep each saturation decision a factor >= 2 from its threshold); and the BOUNDARY-ROW check — every gradient tensor
restricted to the Gaussians within 2 list positions of a boundary, of the first and of the last entry meets compare_backward's
relative L2 of 1e-4 by itself, so that one wrong visit cannot hide under the norm of 65 000 correct rows."""
import collections

import numpy as np
import pytest

import list_scenes as ls
from hip_helpers import HipRun, compare_backward, compare_forward, dev, rel_l2

pytestmark = pytest.mark.gpu

BG = (0.3, 0.1, 0.6)
Ref = collections.namedtuple("Ref", "sc st vp g")
_refs = {}
worst = {}   # (test family, tier) -> largest boundary-row relative L2 seen, printed by every check


def tier_of(L):
    """gsr_stats.tier_tiles of a view whose only list has L entries: (1024, 4096], (4096, 8192], > 8192."""
    return [int(1024 < L <= 4096), int(4096 < L <= 8192), int(L > 8192)]


def tier_name(L):
    return "<= 1024" if L <= 1024 else "(1024, 4096]" if L <= 4096 else "(4096, 8192]" if L <= 8192 else "> 8192"


def reference_for(orc, key, build, vp_seed, mode="rgb", bg=BG, deterministic=True):
    """Scene (build()), oracle forward, cotangent and oracle gradients of a case: computed once, shared, never modified."""
    if key not in _refs:
        sc = build()
        st = orc.forward(*sc.args, sc.cam, sc.deg, background=bg, mode=mode)
        vp = np.random.default_rng(vp_seed).standard_normal(st.image.shape).astype(np.float32)
        g = orc.backward(st, vp, *sc.args, sc.cam, sc.deg, background=bg, deterministic=deterministic)
        for a in (st.image, st.n_contrib, st.accum_alpha, st.values_sorted,
                  g.vmeans, g.vshs, g.vopacities, g.vscales, g.vrots):
            a.setflags(write=False)
        _refs[key] = Ref(sc, st, vp, g)
    return _refs[key]


def reference(orc, kind, L, stop=None, mode="rgb", bg=BG, second=0):
    if kind == "full":
        build = lambda: ls.single_tile_scene(L, 7)  # noqa: E731
    elif kind == "walled":
        build = lambda: ls.walled_scene(L, stop, 11)  # noqa: E731
    else:
        build = lambda: ls.two_tile_scene(L, second, 13)  # noqa: E731
    return reference_for(orc, (kind, L, stop, mode, bg, second), build, 1000 + L, mode, bg)


def hip_run(pkg, ref, mode="rgb", bg=BG, **kw):
    sc = ref.sc
    return HipRun(pkg, *sc.args, sc.cam, sc.deg, bg, mode, **kw)


def show(ref, run):
    sc = ref.sc
    run.t = [dev(sc.means), dev(sc.shs), dev(sc.opac.reshape(-1, 1)), dev(sc.scales), dev(sc.rots)]


def boundary_rows(ref, out, L, stop=None, family="full walk", ids=None):
    """The gradient rows of the Gaussians at ls.boundary_positions(L, stop) (or of `ids`), by themselves, at compare_backward's
    figure."""
    if ids is None:
        ids = ref.sc.order[ls.boundary_positions(L, stop)]
    vm, vs, vo, vsc, vr = [o.cpu().numpy() for o in out[:5]]
    g = ref.g
    errs = {}
    for name, a, b in (("vmeans", vm, g.vmeans), ("vshs", vs, g.vshs), ("vopacities", vo.reshape(-1), g.vopacities),
                       ("vscales", vsc, g.vscales), ("vrotations", vr, g.vrots)):
        errs[name] = rel_l2(a[ids], np.asarray(b)[ids])
    top = max(errs.values())
    key = (family, tier_name(L))
    worst[key] = max(worst.get(key, 0.0), top)
    print(f"boundary rows [{family}] L={L} stop={stop} rows={ids.size}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items())
          + f" | worst so far {key}: {worst[key]:.2e}")
    for name, e in errs.items():
        assert e <= 1e-4, (name, e, L, stop)


def check_forward(ref, run, L, second=0):
    """compare_forward, then what it leaves open: n_contrib at every pixel, the list length and the tier it implies
    (`second`: entries of the second tile's list, two_tile_scene)."""
    img = run.forward()
    compare_forward(ref.st, run, img, ref.sc.opac)
    nc = run.rast.n_contrib.cpu().numpy().astype(np.uint32)
    assert np.array_equal(nc, ref.st.n_contrib), "n_contrib must equal the oracle's at every pixel"
    s = run.rast.stats
    assert s.n_rendered == L + second and s.max_tile_instances == L
    assert list(s.tier_tiles) == tier_of(L)
    if second:
        assert run.rast.ranges.cpu().numpy().tolist() == [[0, L], [L, L + second]] == ref.st.ranges.tolist()
    return img


def check_backward(ref, run, L, stop=None, family="full walk", second=0):
    out = run.backward(ref.vp)
    compare_backward(ref.g, out, ref.st.radii > 0)
    assert rel_l2(run.rast.grad_means_2d.cpu().numpy(), ref.g.vmeans2d) <= 1e-4
    boundary_rows(ref, out, L, stop, family)    # (two tiles: order[:L] is the first tile's list)
    if second:
        # the second list by itself: its rows are 100 to 1000 times larger than the first's and would hide them in one norm
        boundary_rows(ref, out, L, family=family + ", second tile", ids=ref.sc.order[L:L + second])
    return out


def check_two_views(ref, run, L, family):
    """The same view twice.  The first forward of a handle has no per-instance buffers yet, so no early fused sort-and-forward
    launch is sent (gsr_forward: it needs cap_instances > 0) and the separate sort + strip forward run.  The second one is
    the fused kernel's (lists of up to 1024 entries; longer ones hold it beside the tier launches): the buffers the first
    view sized hold it, the bins are in use, and no early launch had to be redone."""
    for view in range(2):
        check_forward(ref, run, L)
        check_backward(ref, run, L, family=family)
    s = run.rast.stats
    assert s.bin_capacity >= L and s.compact_binning == 0 and s.fused_relaunches == 0


# ---- a. the whole list is walked, :rgb ----
@pytest.mark.parametrize("L", ls.FULL_WALK_LENGTHS)
def test_full_walk_rgb(pkg, orc, L):
    ref = reference(orc, "full", L)
    assert (ref.st.n_contrib == L).all()
    check_two_views(ref, hip_run(pkg, ref), L, "full walk")


# ---- b. the depth / normal instantiations, zero background (the BG0 kernels) and a coloured one ----
@pytest.mark.parametrize("bg", [(0.0, 0.0, 0.0), BG], ids=["bg0", "bg"])
@pytest.mark.parametrize("L", ls.MODE_LENGTHS)
@pytest.mark.parametrize("mode", ["rgbd", "rgbdn"])
def test_full_walk_depth_and_normal_modes(pkg, orc, mode, L, bg):
    ref = reference(orc, "full", L, mode=mode, bg=bg)
    check_two_views(ref, hip_run(pkg, ref, mode, bg), L, f"full walk :{mode}")


@pytest.mark.parametrize("L", ls.MODE_LENGTHS)
def test_full_walk_rgb_zero_background(pkg, orc, L):
    """(:rgb takes the zero-background instantiation only in composite_bwd_long_kernel: lists beyond the split length)"""
    ref = reference(orc, "full", L, bg=(0.0, 0.0, 0.0))
    check_two_views(ref, hip_run(pkg, ref, bg=(0.0, 0.0, 0.0)), L, "full walk :rgb bg0")


# ---- c. the library's default lists (exact tile cull) and the accurate backward arithmetic ----
@pytest.mark.parametrize("L", ls.MODE_LENGTHS)
def test_exact_cull_handle_renders_the_same_bits(pkg, orc, L):
    """exact_tile_cull=True drops the instances that reach alpha >= 1/255 nowhere (about 2 % of the thinnest front): a shorter
    list, the same image and transmittance bit for bit, the same gradients."""
    import torch
    ref = reference(orc, "full", L)
    lists, cull = hip_run(pkg, ref), hip_run(pkg, ref, exact_tile_cull=True)
    for _ in range(2):   # (the second view of a handle is the fused kernel's: check_two_views)
        a, b = lists.forward().clone(), cull.forward().clone()
        assert torch.equal(a, b) and torch.equal(lists.rast.accum_alpha, cull.rast.accum_alpha)
        assert 0 < cull.rast.stats.n_rendered <= lists.rast.stats.n_rendered == L
        out = cull.backward(ref.vp)
        compare_backward(ref.g, out, ref.st.radii > 0)
        boundary_rows(ref, out, L, family="exact cull")


@pytest.mark.parametrize("L", ls.MODE_LENGTHS)
def test_accurate_gradient_handle(pkg, orc, L):
    ref = reference(orc, "full", L)
    check_two_views(ref, hip_run(pkg, ref, grad_precision="accurate"), L, "accurate")


# ---- d. the walk stops at a chosen entry ----
@pytest.mark.parametrize("L,stop,precision", [c + (None,) for c in ls.EARLY_STOPS]
                         + [(2500, 1025, "accurate"), (2500, 2049, "accurate"), (9000, 4097, "accurate")])
def test_early_stop(pkg, orc, L, stop, precision):
    """Walls end every pixel's walk after `stop` entries (n_contrib == stop everywhere): nothing behind them may receive a
    gradient — exact zeros, on the first pair of a handle and on a second pair whose walk stops EARLIER.  Both scenes put the
    same Gaussians at the same positions (walled_scene: the permutation depends on L only), so the rows between the two stops
    held gradients a moment ago: a row that is not zeroed again is stale, not zero.  (The earliest stop has none before it: it
    is the second pair of the next one; 65, 1025 and 2049 fall back past their neighbour.)  Lists of 1 000 entries are the
    one-wave backward's, 2 500 and 9 000 the long kernel's — except on an accurate handle, which splits nothing."""
    stops = sorted({s for l, s in ls.EARLY_STOPS if l == L})
    earlier = [e for e in stops if e <= stop - 3]     # (a front row between the two stops: the walls take three positions)
    first, then = (stop, earlier[-1]) if earlier else (stops[1], stop)
    run = None
    for pair, st_pos in enumerate((first, then)):
        ref = reference(orc, "walled", L, st_pos)
        assert (ref.st.n_contrib == st_pos).all()
        if run is None:
            run = hip_run(pkg, ref, grad_precision=precision)
        else:
            show(ref, run)
        check_forward(ref, run, L)
        family = "early stop" if precision is None else "early stop, accurate"
        out = [o.cpu().numpy() for o in check_backward(ref, run, L, st_pos, family=family)[:5]]
        if pair == 0:
            between = ref.sc.order[then:first - 2]
            assert np.array_equal(between, reference(orc, "walled", L, then).sc.order[then:first - 2])
            assert np.abs(out[0][between]).max(1).astype(bool).mean() > 0.9, "the rows the second pair must zero carry gradients now"
        behind = ref.sc.order[st_pos:]
        for name, o in zip(("vmeans", "vshs", "vopacities", "vscales", "vrotations"), out):
            assert not o[behind].any(), (name, "pair", pair, "stop", st_pos)
        assert not run.rast.grad_means_2d.cpu().numpy()[behind].any()


# ---- e. the key bins filled to the last slot, and one key more ----
def _bins_walk(pkg, orc, L1, kind, delta, second=0, third=None):
    """Two views of L1 entries settle the bins' capacity `cap` (read from gsr_stats, equal to gsr_bins_capacity_after); the
    third view brings a list of cap + delta keys.  One handle per delta: the capacity grows after every view whose list + 25 %
    exceeds it (gsr_policy_end_view), so on one handle only the first probe would meet the capacity it was aimed at.
    third = (Ref, L3, family): the third view (and the one after it) shows this scene of L3 > cap entries instead (delta is ignored)."""
    W = 32 if second else 16
    lib = pkg._lib.load()
    ref = reference(orc, kind, L1, second=second)
    run = hip_run(pkg, ref)

    def view(L):
        r, family = (third[0], third[2]) if third and L == third[1] else (reference(orc, kind, L, second=second), None)
        show(r, run)
        check_forward(r, run, L, second)
        check_backward(r, run, L, family=family or ("bin capacity, two tiles" if second else "bin capacity"), second=second)
        return run.rast.stats

    s1 = view(L1)
    first_cap = int(s1.bin_capacity)
    assert s1.compact_binning == 0 and first_cap >= L1
    s2 = view(L1)
    cap = int(s2.bin_capacity)
    assert cap == lib.gsr_bins_capacity_after(L1 + second, L1, W, 16, 0, first_cap) and s2.compact_binning == 0
    if third:
        assert L1 != third[1] > cap
        delta = third[1] - cap
    s = view(cap + delta)
    assert int(s.bin_capacity) == cap
    if delta <= 0:
        assert s.compact_binning == 0, "a list of up to `capacity` keys — the bin filled to its last slot — stays in its bin"
    else:
        # one key too many: bins of >= 1024 keys scatter the overflowing list a second time, smaller ones finish the view compactly
        assert s.compact_binning == (2 if cap >= 1024 else 1), (cap, s.compact_binning)
        L3 = third[1] if third else cap + 1
        s = view(L3)
        assert s.compact_binning == 0, "the next view has bins that hold the list"
        assert int(s.bin_capacity) == lib.gsr_bins_capacity_after(L3 + second, L3, W, 16, 0, cap) >= L3
    return cap


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("L1", sorted(ls.BIN_FIRST_VIEWS))
def test_bin_capacity_edges(pkg, orc, L1, delta):
    cap = _bins_walk(pkg, orc, L1, "full", delta)
    assert (cap >= 1024) == (L1 == 1000)


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("L1", sorted(ls.TWO_TILE_FIRST_VIEWS))
def test_bin_capacity_edges_with_a_second_tile(pkg, orc, L1, delta):
    """32 x 16: the full bin is the FIRST tile's, and a second list of ten entries starts right behind it (tile_start of a
    tile that is not the first)."""
    cap = _bins_walk(pkg, orc, L1, "two", delta, second=ls.TWO_TILE_SECOND)
    assert (cap >= 1024) == (L1 == 1000)
