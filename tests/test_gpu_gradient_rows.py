"""-m gpu: every Gaussian's gradient ROW against the oracle and the float64 autograd model (tests/gradient_rows.py; its premises
are held on the oracle alone by tests/test_gradient_rows_cpu.py).

hip_helpers.compare_backward — the one helper behind the parity, list-boundary, sort-tie, tier-routing, walk-class, instance-trim
and scale tests — holds a tensor's relative L2 to 1e-4.  Adam and `densify` consume the gradients per Gaussian, and on a deep list
a third of the non-zero rows can be zeroed under that norm.  Here all five gradient tensors and `rast.grad_means_2d` are held row
by row: T_i = 1e-4 · |ref_i| + 1e-5 · rms(ref), a row passing if it is exactly zero where both references are (z), within T_i of
the oracle (a) or of float64 (f), or — axis ratio above 10 — no farther from float64 than 4 x the oracle + T_i (b); rows that
blend into a pixel with a pair on the alpha = 1/255 boundary and meet neither (a) nor (f) are exempt, at most 2 % of a tensor.

Scenes (gradient_rows.SCENES): the five small cells of test_forward_backward_vs_oracle, fuzz_scenes.sweep_scene(0..11) and
edge_scene(0..5) (modes :rgb / :rgbd / :rgbdn by case), needle_scene(1), the one-tile lists of 65, 1025 (:rgb and :rgbdn) and
2049 entries walked to their end and of 1000 / 2500 entries stopped after 64 / 1025.  Handle forms: reference lists, exact tile
cull (sweep and edge), and the three `grad_precision` settings on sweep 5, edge 2, needle 1 and the 2500-entry walled list.
Lists beyond 1024 entries are composite_bwd_long_kernel's on a default handle (asserted through gsr_stats.tier_tiles); an
accurate handle splits nothing, so there the one-wave kernel walks the 2500 entries.

Measured (MI355X, all scenes): 85 946 rows pass by (a), 27 362 by (z), one each by (f) and (b) — the ∇rotations / ∇means rows of one
600 : 1 needle of needle_scene(1) —, none is exempt, none fails.  Worst |hip_i - orc_i| / T_i apart from that needle: 0.95 on the
default handle (∇scales, edge_scene(3)), 0.55 accurate, 0.27 fp32-reference; the relative term the well-conditioned rows outside
`touched` would need against float64 with the floor unchanged: 1.9e-5 default (∇scales), 4.1e-7 accurate, 9.6e-7 fp32-reference —
so 1e-4 holds for all three precisions and the default arithmetic has no term of its own.

Every case prints, per tensor, the rows checked, the rows passed by each rule, the rows exempt and the worst
|hip_i - orc_i| / T_i."""
import collections

import numpy as np
import pytest

import gradient_rows as gr
from hip_helpers import HipRun

pytestmark = pytest.mark.gpu

Hip = collections.namedtuple("Hip", "rows tier_tiles values_sorted n_contrib")
_runs = {}


def hip_rows(pkg, ref, **form):
    """One forward + backward of the scene on a fresh handle of the given form -> the six tensors as {name: (N, k) float64}.  Kept
    per (scene, form): the one-tile tests read the default run again."""
    key = (ref.sc.name, tuple(sorted(form.items())))
    if key not in _runs:
        sc = ref.sc
        run = HipRun(pkg, *sc.arrays, sc.cam, sc.deg, sc.bg, sc.mode, **form)
        run.forward()
        out = run.backward(sc.vp.copy())   # (the shared cotangent is read-only)
        n = ref.vis.size
        rows = {nm: o.cpu().numpy().astype(np.float64).reshape(n, -1) for nm, o in zip(gr.NAMES, out[:5])}
        rows["vmeans2d"] = run.rast.grad_means_2d.cpu().numpy().astype(np.float64).reshape(n, -1)
        _runs[key] = Hip(rows, list(run.rast.stats.tier_tiles), run.rast.values_sorted.cpu().numpy().astype(np.int64),
                         run.rast.n_contrib.cpu().numpy().astype(np.int64))
    return _runs[key]


def check(pkg, orc, name, label="", **form):
    ref = gr.reference(pkg, orc, name)
    hip = hip_rows(pkg, ref, **form)
    for nm in gr.ALL_NAMES:   # culled Gaussians: exact zeros, ∇means_2d included
        assert not hip.rows[nm][~ref.vis].any(), nm
    return gr.check_scene(ref, hip.rows, label=label)


@pytest.mark.parametrize("name", gr.SCENES)
def test_rows_reference_lists(pkg, orc, name):
    check(pkg, orc, name)


@pytest.mark.parametrize("name", gr.SWEEP + gr.EDGE)
def test_rows_exact_tile_cull(pkg, orc, name):
    check(pkg, orc, name, " [exact_tile_cull]", exact_tile_cull=True)


@pytest.mark.parametrize("name", gr.PRECISION_SCENES)
@pytest.mark.parametrize("precision", [None, "accurate", "fp32_reference"])
def test_rows_grad_precision(pkg, orc, precision, name):
    check(pkg, orc, name, f" [grad_precision={precision}]", grad_precision=precision)


@pytest.mark.parametrize("name", gr.ONE_TILE)
def test_one_tile_rows_by_list_position(pkg, orc, name):
    """The list is read back from the run (position p holds Gaussian order[p], as the builder promises), so a failure names the
    position.  Rows past an early stop are exactly zero; each of the 64 positions before the end of the walk — the low-T tail,
    where a liveness trim or a segment composition that is off by one entry shows — passes by a rule of its own, not by exemption."""
    ref = gr.reference(pkg, orc, name)
    sc = ref.sc
    hip = hip_rows(pkg, ref)
    L = sc.length
    assert hip.tier_tiles == [int(1024 < L <= 4096), 0, 0], "lists beyond 1024 entries: composite_bwd_long_kernel"
    assert np.array_equal(hip.values_sorted[:L], sc.order)
    end = L if sc.stop is None else sc.stop
    assert (hip.n_contrib == end).all()
    for nm in gr.ALL_NAMES:
        behind = hip.rows[nm][sc.order[end:]]
        assert not behind.any(), (nm, "positions with a gradient behind the stop", end + np.flatnonzero(behind.any(1))[:8])
    tail = sc.order[max(0, end - 64):end]
    for nm in gr.ALL_NAMES:
        rule, ratio = gr.classify_rows(hip.rows[nm], ref.orc[nm], ref.f64[nm], ref.vis, ref.touched, ref.ill)
        bad = [(int(ref.positions[i]), str(rule[i]), float(ratio[i])) for i in tail if rule[i] not in "zafb"]
        assert not bad, (nm, "(list position, rule, |hip - orc| / T) of the tail rows that do not pass", bad)
        print(f"tail {name} {nm}: positions {max(0, end - 64)} .. {end - 1}: "
              + ", ".join(f"{k} {int((rule[tail] == k).sum())}" for k in "zafb") + f", worst |hip - orc| / T = {ratio[tail].max():.3f}")
