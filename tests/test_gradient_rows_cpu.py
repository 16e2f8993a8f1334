"""The per-row gradient criterion of tests/gradient_rows.py, held on the CPU oracle alone (no GPU): the premises of
tests/test_gpu_gradient_rows.py.

  * the oracle itself meets the criterion on every scene the GPU file uses — in the roles check_rows(hip := the oracle with double
    sums, orc := the oracle in the reference's own form, fp32 atomics) and directly against float64 — with the exempt rows within
    the 2 % cap and the boundary pixels within compare_forward's bound;
  * planted faults: gradient copies that hip_helpers.compare_backward (rel-L2 <= 1e-4 per tensor) accepts and check_rows refuses;
  * the blindness table of DESIGN.md §3: non-zero rows that could be zeroed unnoticed, under the norm and under the rows."""
import types

import numpy as np
import pytest
import torch

import gradient_rows as gr
from hip_helpers import compare_backward, rel_l2


def _reference_form(orc, ref):
    """The oracle's like-for-like mode (deterministic=False: fp32 `omp atomic` accumulators, render.jl:242,262-282) on ONE thread:
    the order of the float additions is then fixed and the test reproducible."""
    threads = orc.num_threads()
    try:
        orc.set_num_threads(1)
        return gr.oracle_gradients(orc, ref.sc, ref.st, deterministic=False)
    finally:
        orc.set_num_threads(threads)


@pytest.mark.parametrize("name", gr.SCENES)
def test_oracle_alone_meets_the_row_criterion(pkg, orc, name):
    ref = gr.reference(pkg, orc, name)
    assert ref.vis.any() and gr.boundary_pixels_ok(ref.bmask), (int(ref.bmask.sum()), ref.bmask.size)
    form = _reference_form(orc, ref)
    for nm in gr.ALL_NAMES:
        rep = gr.check_rows(f"{name} {nm}", ref.orc[nm], form[nm], ref.f64[nm], ref.vis, ref.touched, ref.ill, ref.positions)
        print(f"rows {rep.name} [oracle | fp32 atomics | f64]: checked {rep.checked}, z {rep.z}, a {rep.a}, f {rep.f}, b {rep.b}, "
              f"exempt {rep.exempt}, worst {rep.worst:.3f}")
        assert rep.exempt <= gr.EXEMPT_CAP * rep.checked
        assert rep.z + rep.a + rep.f + rep.b + rep.exempt == rep.checked
        # ... and the oracle against float64 directly: every row outside the two exemption sets within T_i(f64); the rows of
        # those sets that miss it are few (measured: 5 touched rows of 400 on cell-103, one needle row on edge-3 and needle-1)
        T, _ = gr.row_tolerance(ref.f64[nm], ref.vis)
        miss = ref.vis & (np.linalg.norm(ref.orc[nm] - ref.f64[nm], axis=1) > T)
        assert not (miss & ~ref.touched & ~ref.ill).any(), (nm, np.flatnonzero(miss & ~ref.touched & ~ref.ill))
        assert miss.sum() <= gr.EXEMPT_CAP * rep.checked, (nm, int(miss.sum()))
        # culled Gaussians: exact zeros on all three sides
        assert not ref.orc[nm][~ref.vis].any() and not ref.f64[nm][~ref.vis].any()


def test_the_float64_means_2d_is_the_oracles(pkg, orc):
    """f64_gradients' "vmeans2d" (the cotangent of the model's m2) is g.vmeans2d: same units, same terms — to the oracle's own
    fp32 error, row by row, on a scene without a boundary pair."""
    ref = gr.reference(pkg, orc, "cell-101")
    assert not ref.touched.any() and ref.f64["vmeans2d"].shape == (ref.vis.size, 2)
    assert rel_l2(ref.orc["vmeans2d"], ref.f64["vmeans2d"]) <= 1e-5
    T, _ = gr.row_tolerance(ref.f64["vmeans2d"], ref.vis)
    assert (np.linalg.norm(ref.orc["vmeans2d"] - ref.f64["vmeans2d"], axis=1) <= T).all()


@pytest.mark.parametrize("name", gr.ONE_TILE)
def test_one_tile_scenes_give_the_rows_the_gpu_file_reads(pkg, orc, name):
    """List position p holds Gaussian order[p]; nothing behind an early stop has a gradient; the 64 positions before the stop (the
    low-T tail of the walk) hold rows with signal."""
    import list_scenes as ls
    ref = gr.reference(pkg, orc, name)
    sc = ref.sc
    assert np.array_equal(ls.list_positions(ref.st), sc.order) and sc.order.size == sc.length
    end = sc.length if sc.stop is None else sc.stop
    assert (ref.st.n_contrib == end).all()
    for nm in gr.ALL_NAMES:
        assert not ref.orc[nm][sc.order[end:]].any() and not ref.f64[nm][sc.order[end:]].any()
    tail = sc.order[max(0, end - 64):end]
    assert (ref.orc["vmeans"][tail].any(1)).sum() >= tail.size // 2


# ---- planted faults ----
def _faint_first(nrm, candidates):
    """The candidate rows, faintest first."""
    idx = np.flatnonzero(candidates)
    return idx[np.argsort(nrm[idx], kind="stable")]


def _within_budget(rows, weight, total, budget):
    """The longest prefix of `rows` whose fault — of norm weight[i] on row i — keeps the tensor's rel-L2 <= budget."""
    if rows.size == 0:
        return rows
    return rows[np.sqrt(np.cumsum(weight[rows] ** 2)) <= budget * total]


BUDGET = 0.9e-4   # of compare_backward's 1e-4: "a fainter variant" wherever the fault as listed would show in the norm


def _fault_zero(o, nrm, cand, total, rms):
    rows = _within_budget(_faint_first(nrm, cand), nrm, total, BUDGET)[:100]
    h = o.copy(); h[rows] = 0.0
    return h, rows, nrm


def _fault_scale(o, nrm, cand, total, rms):
    below = cand & (nrm < np.median(nrm[cand]))
    rows = _within_budget(_faint_first(nrm, below), 0.01 * nrm, total, BUDGET)
    h = o.copy(); h[rows] *= 1.01
    return h, rows, 0.01 * nrm


def _fault_band(o, nrm, cand, total, rms):
    K = o.shape[1] // 3
    k = min(5, K - 1)                      # (a degree-0 scene has the one band)
    band = np.linalg.norm(o[:, 3 * k:3 * k + 3], axis=1)
    below = cand & (nrm < np.median(nrm[cand]))
    rows = _within_budget(_faint_first(nrm, below), band, total, BUDGET)
    h = o.copy(); h[rows, 3 * k:3 * k + 3] = 0.0
    return h, rows, band


def _fault_swap(o, nrm, cand, total, rms):
    """Two rows adjacent in the ranking by norm, the strongest pair that stays inside the budget."""
    order = _faint_first(nrm, cand)
    d = np.zeros_like(nrm)
    d[order[:-1]] = np.linalg.norm(o[order[:-1]] - o[order[1:]], axis=1)     # |o_i - o_next|: the fault on EACH row of the pair
    ok = np.flatnonzero(np.sqrt(2.0) * d[order[:-1]] <= BUDGET * total)
    if ok.size == 0:
        return o.copy(), np.zeros(0, np.int64), d
    i = order[ok[-1]]; j = order[ok[-1] + 1]
    h = o.copy(); h[[i, j]] = o[[j, i]]
    moved = np.zeros_like(nrm)
    moved[[i, j]] = d[i]
    return h, np.array([i, j]), moved


def _fault_plant(o, nrm, cand_zero, total, rms):
    i = np.flatnonzero(cand_zero)[0]
    h = o.copy(); h[i, 0] = 1e-3 * rms
    w = np.zeros_like(nrm); w[i] = 1e-3 * rms
    return h, np.array([i]), w


# fault -> (builder, tensors that take it, the tensor on which check_rows MUST fail)
FAULTS = {"zero the faintest rows": (_fault_zero, gr.ALL_NAMES, "vmeans"),
          "scale the rows below the median by 1.01": (_fault_scale, gr.ALL_NAMES, "vmeans"),
          "drop one SH band below the median": (_fault_band, ("vshs",), "vshs"),
          "swap two adjacent faint rows": (_fault_swap, ("vmeans", "vshs", "vscales", "vrots", "vmeans2d"), "vmeans"),
          "write 1e-3 rms into an exactly-zero row": (_fault_plant, gr.ALL_NAMES, "vmeans")}


@pytest.mark.parametrize("fault", list(FAULTS))
@pytest.mark.parametrize("name", gr.FAULT_SCENES)
def test_planted_fault_passes_the_norm_and_fails_the_rows(pkg, orc, name, fault):
    """Each fault goes into a copy of the ORACLE's gradients, on rows that are visible and in no exemption set (not `touched`, axis
    ratio <= 10), in every tensor that can take it at once.  "A fainter variant": where the fault as listed would move a tensor's
    norm by more than 0.9e-4 (walled_scene: every front row is about as large as the typical one), only the faintest rows up to
    that budget take it, and a tensor in which not even one row fits stays as it is — the norm is not blind there (∇shs of the
    degree-0 walled scene: dropping ANY row is 1.5e-4 of the tensor; the SH-band fault therefore runs on the same list at degree
    2, where band 5 is a small part of a row).
    Asserted: compare_backward, and the rel-L2 that the parity tests hold ∇means_2d to, accept the faulted copy; on the fault's
    expected tensor some faulted row is moved by more than T_i against both references (+ the oracle's own distance from float64:
    a premise on the references alone) — and check_rows refuses every tensor with such a row, naming rows."""
    make, tensors, expected = FAULTS[fault]
    if make is _fault_band and name.startswith("walled"):
        name += "-deg2"
    ref = gr.reference(pkg, orc, name)
    plain = ref.vis & ~ref.touched & ~ref.ill
    hip, moved = dict(ref.orc), {}
    for nm in tensors:
        o, f = ref.orc[nm], ref.f64[nm]
        nrm = np.linalg.norm(o, axis=1)
        To, rms = gr.row_tolerance(o, ref.vis)
        Tf, _ = gr.row_tolerance(f, ref.vis)
        cand = plain & ~o.any(1) & ~f.any(1) if make is _fault_plant else plain & (nrm > 0)
        h, rows, delta = make(o, nrm, cand, float(np.linalg.norm(o)), rms)
        seen = (delta[rows] > 1.01 * To[rows]) & (delta[rows] > 1.01 * (Tf[rows] + np.linalg.norm(o - f, axis=1)[rows]))
        hip[nm], moved[nm] = h, (rows, int(seen.sum()))
    assert moved[expected][1] > 0, (expected, "no faulted row is moved beyond its own tolerance", moved[expected])
    n = ref.vis.size
    shaped = [torch.from_numpy(hip[nm].astype(np.float32).reshape(np.asarray(a).shape if nm != "vopacities" else (n, 1)))
              for nm, a in zip(gr.NAMES, ref.sc.arrays)]
    g = types.SimpleNamespace(**{nm: ref.orc[nm].reshape(t.shape if nm != "vopacities" else -1) for nm, t in zip(gr.NAMES, shaped)})
    compare_backward(g, shaped + [None, None], ref.vis)
    assert rel_l2(hip["vmeans2d"], ref.orc["vmeans2d"]) <= 1e-4
    for nm in tensors:
        args = (ref.orc[nm], ref.f64[nm], ref.vis, ref.touched, ref.ill, ref.positions)
        gr.check_rows(nm, ref.orc[nm], *args)                      # the unfaulted copy passes
        rows, seen = moved[nm]
        if not seen:
            print(f"{name} | {fault} | {nm}: {rows.size} rows faulted, none beyond its tolerance")
            continue
        with pytest.raises(AssertionError, match="fail the row criterion") as e:
            gr.check_rows(nm, hip[nm], *args)
        print(f"{name} | {fault} | {nm}: {rows.size} rows faulted, {seen} beyond tolerance; rel-L2 of the tensor "
              f"{rel_l2(hip[nm], ref.orc[nm]):.2e}; check_rows: {str(e.value).splitlines()[0]}")


def test_blindness_of_the_norm_and_of_the_rows(pkg, orc):
    """DESIGN.md §3's table: per scene and tensor, the non-zero visible rows that can be set to ZERO unnoticed under the tensor norm
    and under the row rule.  A row the row rule lets go is below 1e-5 of the typical row, so the row rule never lets more go than
    the norm does; on the two deep scenes the norm lets a third of the rows go."""
    print(f"{'scene':18s} {'tensor':11s} non-zero  norm  rows")
    for name in gr.SCENES:
        ref = gr.reference(pkg, orc, name)
        for nm in gr.ALL_NAMES:
            o = ref.orc[nm]
            live = int((ref.vis & o.any(1)).sum())
            by_norm, by_rows = gr.zeroable_rows(o, ref.vis, "norm"), gr.zeroable_rows(o, ref.vis, "rows")
            print(f"{name:18s} {nm:11s} {live:8d} {by_norm:5d} {by_rows:5d}")
            assert by_rows <= by_norm <= live
            if name in ("sweep-5", "edge-2"):
                assert by_norm >= 0.3 * live, (name, nm, live, by_norm, by_rows)
