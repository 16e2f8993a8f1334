"""The :rgb backward on a zero background: composite_bwd_kernel_rgb_bg0 (composite.hip) and the reduction
of two instances in one network (wave_reduce.h wave_reduce_rowcol_rgb_pair).

-m gpu.  With background (0, 0, 0) and the default grad_precision the :rgb backward is the zero-background kernel: an instance
that blends a pixel of the wave waits for the next one that does, the two are reduced together, and an instance left without a
partner when a 64-entry batch or the list ends is reduced alone.  Scenes, all through a 40 x 24 camera (partial tiles, pixels of
the second tile row outside the image), on buffers poisoned with GSR_DEBUG_FILL=nan:
  * the one-tile lists of list_scenes.single_tile_scene with 1, 2, 3, 63, 64, 65, 66 and 129 entries, every one of which blends
    a pixel (asserted on the oracle): odd and even counts, a partner-less instance at the end of a batch (63, 65: the 64-entry
    batches are cut from the BACK of the list, 65 = 64 + 1) and at the end of the list;
  * a list of 130 in which every second entry has opacity 0.0039 < 1/255 and blends nowhere: partners separated by skipped
    instances, whose rows stay exact zeros;
  * splats confined to rows 12-15 (test_gpu_bwd_instance_trims.band_scene): the first visited pixel group is not group 0;
  * each of them again with background (0.3, 0.2, 0.1), which takes the general kernel.
Every gradient row is held to the oracle and the float64 model by the row criterion of tests/gradient_rows.py (the tolerances of
test_gpu_parity.py), the tensors by hip_helpers.compare_backward, and a second backward on the same forward must give torch.equal
gradients.

Without a GPU: the lane bookkeeping of wave_reduce_rowcol_rgb_pair restated in numpy — which lane ends with which of the 18 sums —
and each sum compared, in float32 with the association of the network, with the unpaired network's."""
import numpy as np
import pytest

import gradient_rows as gr
import list_scenes as ls

W, H = 40, 24
LENGTHS = (1, 2, 3, 63, 64, 65, 66, 129)
BACKGROUNDS = {"bg0": (0.0, 0.0, 0.0), "bg": (0.3, 0.2, 0.1)}
F = np.float32


# ------------------------------------------------------------------------------------------------------------------
# CPU: the two networks on the 64 lanes of a wave, float32, one rounding per add / multiply as the kernel's
# ------------------------------------------------------------------------------------------------------------------
LANE = np.arange(64)


def _bit(mask):
    return (LANE & mask) != 0


def _pair(a, b, bit, partner):
    """One pairing level: lanes with `bit` clear carry on with a, the others with b; each adds its partner lane's share."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.where(bit, b + b[partner], a + a[partner]).astype(F)


def swap32(a, b): return _pair(a, b, _bit(32), LANE ^ 32)
def swap16(a, b): return _pair(a, b, _bit(16), LANE ^ 16)
def ror8(a, b): return _pair(a, b, _bit(8), LANE ^ 8)       # row_ror:8 within a row of 16 lanes
def xor1(a, b): return _pair(a, b, _bit(1), LANE ^ 1)
def xor2(a, b): return _pair(a, b, _bit(2), LANE ^ 2)


def shr4(z):
    """row_shr:4: lane i adds lane i - 4 of its row, lanes 0-3 of a row add zero."""
    got = np.where((LANE & 15) >= 4, z[np.maximum(LANE - 4, 0)], F(0)).astype(F)
    return (z + got).astype(F)


def unpaired_network(P, U1, U2, c0, c1, c2, dx):
    """wave_reduce_rowcol_rgb and RowColConsts: {accumulator slot: (lane, value)} of one instance."""
    r = LANE >> 4
    e1, e3 = ((r == 0) | (r == 2)).astype(F), (r == 0).astype(F)
    k2, k4 = (r == 1).astype(F), (r == 2).astype(F)
    a0, a1, a2 = swap32(P, U1), swap32(c0, c1), swap32(U2, c2)
    b0, b1 = swap16(a0, a1), swap16(a2, a2)
    o0 = b0
    o1 = ((b0 * (dx * e1).astype(F)).astype(F) + (b1 * k2).astype(F)).astype(F)
    o2 = ((b0 * ((dx * dx).astype(F) * e3).astype(F)).astype(F) + (b1 * k4).astype(F)).astype(F)
    x0, x1 = ror8(o0, o1), ror8(o2, o2)
    y = xor1(x0, x1)
    total = shr4(xor2(y, y))
    table = [[3, 7, 4], [0, 6, -1], [8, 5, 2], [1, -1, -1]]
    out = {}
    for lane in range(64):
        j = 2 if lane & 1 else (1 if lane & 8 else 0)
        writer = (lane & 6) == 4 and not ((lane & 1) and (lane & 8))
        slot = table[lane >> 4][j] if writer else -1
        if slot >= 0:
            assert slot not in out
            out[slot] = (lane, total[lane])
    return out


def pair_slot(lane):
    """RowColConstsPair: (instance 0 = A / 1 = B, accumulator slot) the lane writes, or None."""
    j = 2 if lane & 2 else (3 if lane & 1 else 0) + (1 if lane & 8 else 0)
    writer = bool(lane & 4) and (not (lane & 2) or not (lane & 9))
    slot = [[3, 7, 4, 0, 6], [8, 5, -1, 1, 2]][lane >> 5][j]
    return ((lane >> 4) & 1, slot) if writer and slot >= 0 else None


def paired_network(A, B):
    """wave_reduce_rowcol_rgb_half on A = (P, U1, U2, c0, c1, c2, dx) and on B, then wave_reduce_rowcol_rgb_pair: the per-lane
    totals."""
    PA, U1A, U2A, c0A, c1A, c2A, dxA = A
    PB, U1B, U2B, c0B, c1B, c2B, dxB = B
    A0, A1, A2 = swap32(PA, U1A), swap32(c0A, c1A), swap32(U2A, c2A)   # the first level, each instance by itself
    B0, B1, B2 = swap32(PB, U1B), swap32(c0B, c1B), swap32(U2B, c2B)
    b0, b1, b2 = swap16(A0, B0), swap16(A1, B1), swap16(A2, B2)
    dx = np.where(_bit(16), dxB, dxA).astype(F)
    o1, o2 = (b0 * dx).astype(F), (b0 * (dx * dx).astype(F)).astype(F)
    x0, x1, x2 = ror8(b0, o1), ror8(b1, b2), ror8(o2, o2)
    y0, y1 = xor1(x0, x1), xor1(x2, x2)
    return shr4(xor2(y0, y1))


def _instance(rng):
    """Six per-lane sums and dx = (splat x) - (pixel x): a function of the lane's column only."""
    sums = [rng.standard_normal(64).astype(F) * F(10.0 ** rng.uniform(-3, 3)) for _ in range(6)]
    dx = (F(rng.uniform(-20.0, 36.0)) - (LANE & 15).astype(F)).astype(F)
    return (*sums, dx)


@pytest.mark.parametrize("seed", range(8))
def test_paired_network_writes_each_sum_once_and_equals_the_unpaired_one(seed):
    rng = np.random.default_rng(seed)
    A, B = _instance(rng), _instance(rng)
    total = paired_network(A, B)
    writers = {}
    for lane in range(64):
        s = pair_slot(lane)
        if s is not None:
            assert s not in writers, f"sum {s} has two writer lanes"
            writers[s] = lane
    assert sorted(writers) == [(i, k) for i in range(2) for k in range(9)], "18 sums, each written by exactly one lane"
    for i, inst in enumerate((A, B)):
        ref = unpaired_network(*inst)
        assert sorted(ref) == list(range(9))
        for k in range(9):
            got, want = total[writers[(i, k)]], ref[k][1]
            assert got.dtype == np.float32 and got == want, (i, k, got, want)
    # the sums are what they are meant to be, in float64 (to the rounding of 64 float32 terms)
    P, U1, U2, c0, c1, c2, dx = (np.asarray(x, np.float64) for x in B)
    terms = {0: c0, 1: c1, 2: c2, 3: P, 4: dx * dx * P, 5: dx * U1, 6: U2, 7: dx * P, 8: U1}
    for k, t in terms.items():
        got = float(total[writers[(1, k)]])
        assert abs(got - t.sum()) <= 8 * 2.0 ** -24 * np.abs(t).sum(), (k, got, t.sum())


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _wide(sc):
    from test_gpu_bwd_instance_trims import wide
    return wide(sc)


def _alternating(L=130):
    """single_tile_scene(L) with the entries at list positions 1, 3, ..., L - 3 made too faint to blend anywhere (opacity
    0.0039 < 1/255); the backdrop at L - 1 stays as it is."""
    sc = ls.single_tile_scene(L, 41)
    ghosts = sc.order[1:L - 1:2]
    sc.opac[ghosts] = 0.0039
    sc.ghosts = ghosts
    return sc


def _band():
    from test_gpu_bwd_instance_trims import band_scene
    return band_scene((3,), 0, 23)


def _build(name):
    if name.startswith("tile-"):
        return _wide(ls.single_tile_scene(int(name[5:]), 43))
    return _wide(_alternating()) if name == "alternating" else _band()


SCENES = tuple(f"tile-{L}" for L in LENGTHS) + ("alternating", "rows12-15")
_refs = {}


def reference(orc, name, bgname):
    """Scene, oracle state and the gradients of the oracle and of the float64 model: computed once per case, read-only."""
    if (name, bgname) not in _refs:
        from hip_helpers import blend_boundary_pixels
        sc, bg = _build(name), BACKGROUNDS[bgname]
        n = sc.means.shape[0]
        vp = np.random.default_rng(47).standard_normal((H, W, 3)).astype(np.float32)
        rs = gr.RowScene(f"{name}-{bgname}", sc.args, sc.cam, sc.deg, "rgb", bg, vp, sc.order)
        st = orc.forward(*sc.args, sc.cam, sc.deg, background=bg, mode="rgb")
        g = gr.oracle_gradients(orc, rs, st)
        f64 = gr.f64_gradients(sc.args, sc.cam, sc.deg, "rgb", bg, st, vp)
        bmask, _, ids = blend_boundary_pixels(st, sc.opac, W, H, with_ids=True)
        touched = np.zeros(n, bool)
        touched[list(ids)] = True
        s = np.abs(np.asarray(sc.scales, np.float64))
        ill = s.max(1) / np.maximum(s.min(1), 1e-30) > gr.ILL_RATIO
        positions = np.full(n, -1, np.int64)
        first = ls.list_positions(st)
        positions[first] = np.arange(first.size)
        graw = orc.backward(st, vp, *sc.args, sc.cam, sc.deg, background=bg)
        _refs[(name, bgname)] = (sc, graw, gr.Reference(rs, st, g, f64, st.radii > 0, touched, ill, positions, bmask))
    return _refs[(name, bgname)]


def _scene_conditions(name, sc, st):
    """What the case is about, on the oracle: who is in the first tile's list and who blends there."""
    from test_gpu_bwd_instance_trims import blended_rows
    first = ls.list_positions(st)
    blends = np.array([blended_rows(st, sc.opac, i).size > 0 for i in first])
    if name.startswith("tile-"):
        L = int(name[5:])
        assert first.size == L and blends.all(), "a one-tile list of L instances, each of which blends a pixel"
        assert int(st.n_contrib[:16, :16].max()) == L, "walked to its end"
    elif name == "alternating":
        assert first.size == 130 and np.array_equal(first, sc.order)
        assert not blends[1:129:2].any() and blends[0::2].all() and blends[129]
    else:
        assert first.size >= 30 and blends.sum() >= 30
        for i in first[blends]:
            assert (blended_rows(st, sc.opac, i) >= 12).all(), "rows 12-15 only"


@pytest.mark.gpu
def test_the_built_library_holds_the_zero_background_kernel(pkg):
    """composite_bwd_kernel_rgb_bg0 is a kernel of its own, not an instantiation of composite_bwd_kernel<C, BG0, VC, ACC>: the census
    of tests/test_gpu_poisoned_buffers.py (the template's instantiations, by mangled name) does not list it.  Its cells with :rgb, a
    zero background and the default precision run it on poisoned buffers, as the "bg0" cases below do; here: it is compiled, and
    the template has no <3, true, ...> twin of it."""
    blob = open(pkg._lib.LIB_PATH, "rb").read()
    assert b"composite_bwd_kernel_rgb_bg0" in blob
    assert b"composite_bwd_kernelILi3ELb1" not in blob


@pytest.mark.gpu
@pytest.mark.parametrize("bgname", list(BACKGROUNDS))
@pytest.mark.parametrize("name", SCENES)
def test_rows_against_the_oracle_on_poisoned_buffers(pkg, orc, name, bgname):
    import torch
    from hip_helpers import HipRun, compare_backward
    from test_gpu_bwd_instance_trims import env
    sc, graw, ref = reference(orc, name, bgname)
    st, n = ref.st, sc.means.shape[0]
    _scene_conditions(name, sc, st)
    with env("GSR_DEBUG_FILL", "nan"):
        run = HipRun(pkg, *sc.args, sc.cam, sc.deg, BACKGROUNDS[bgname], "rgb")
        run.forward()
        assert run.rast.stats.n_rendered == st.n_rendered
        assert np.array_equal(run.rast.values_sorted.cpu().numpy().astype(np.uint32), st.values_sorted)
        out = run.backward(ref.sc.vp)
        first = [o.clone() for o in out[:5]] + [run.rast.grad_means_2d.clone()]
        out2 = run.backward(ref.sc.vp)
        second = list(out2[:5]) + [run.rast.grad_means_2d]
    for nm, a, b in zip(gr.ALL_NAMES, first, second):
        assert torch.equal(a, b), f"{nm}: two backwards of one forward differ"
    compare_backward(graw, out, st.radii > 0)
    rows = {nm: o.cpu().numpy().astype(np.float64).reshape(n, -1) for nm, o in zip(gr.ALL_NAMES, first)}
    for nm in gr.ALL_NAMES:
        assert np.isfinite(rows[nm]).all(), nm
        assert not rows[nm][~ref.vis].any(), nm
    gr.check_scene(ref, rows)
    if name == "alternating":
        for nm in gr.ALL_NAMES:
            assert not rows[nm][sc.ghosts].any(), "an instance no lane blends keeps exact zero rows"
