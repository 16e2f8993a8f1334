"""The float64 definition of density control (tests/densify_ref.py) against the fp32 restatement oracle/densify.py, without a
GPU — and the measurements that tests/test_gpu_density_edges.py takes its tolerances and its undecided-row cap from, made on
that test's own inputs (densify_ref.py holds them), so that none of them comes from the code under test:
  * the restatement's largest error against the definition for the normals, the split children's points and scales and the
    reset opacities: asserted not to exceed densify_ref.RESTATEMENT_ERR (and to be within a factor of two of it: the recorded
    figures are measurements, not allowances);
  * the number of undecided rows of the random mask model: at most 1 % for every gamma and min_opacity the GPU test uses;
  * the hand rows of the masks: the definition, the restatement and the mask written down by hand agree, the NaN rows included.
Run with -s to see the figures."""
import numpy as np
import pytest

import densify_ref as R
from oracle import densify as dz

f32, f64 = np.float32, np.float64


def restatement_mask(c):
    """oracle/densify.py's statements for one gsr_densify_mask call (densify_clone :175, densify_split :184-187,
    densify_and_prune :212-215)."""
    n = c["n"]
    with np.errstate(invalid="ignore", over="ignore"):
        if c["kind"] == R.PRUNE:
            valid = dz.sigmoid(c["opacities"]).reshape(-1) > f32(c["min_opacity"])
            if c["max_screen_size"] > 0:
                valid &= (c["max_radii"] < c["max_screen_size"]) & (dz.max_exp_scale(c["scales"]) < f32(c["gamma"]))
            return valid
        padded = np.zeros(n, f32)
        if c["n_grad"]:
            padded[:c["n_grad"]] = c["grad"][:c["n_grad"]]
        if c["kind"] == R.CLONE:
            return (padded > f32(c["thr"])) & (dz.max_exp_scale(c["scales"]) < f32(c["gamma"]))
        return (padded >= f32(c["thr"])) & (dz.max_exp_scale(c["scales"]) > f32(c["gamma"]))


def definition_mask(c):
    return R.masks(c["kind"], c["grad"], c["n_grad"], c["scales"], c["opacities"], c["max_radii"], c["thr"], c["gamma"],
                   c["min_opacity"], c["max_screen_size"])


@pytest.mark.parametrize("sd", [1, 3])
def test_hand_rows_definition_restatement_and_hand_agree(sd):
    calls = R.hand_mask_calls(sd)
    assert len(calls) >= 17
    for c in calls:
        mask, decided = definition_mask(c)
        assert decided.all(), (c["name"], np.flatnonzero(~decided))
        assert np.array_equal(mask.astype(np.uint8), c["expect"]), (c["name"], mask.astype(np.uint8), c["expect"])
        assert np.array_equal(restatement_mask(c).astype(np.uint8), c["expect"]), c["name"]


@pytest.mark.parametrize("sd", [1, 3])
def test_random_mask_rows_are_decided_and_match_the_restatement(sd):
    scales, opac, grad, radii = R.mask_case(sd)
    n, worst = R.MASK_ROWS, 0
    for kind in (R.CLONE, R.SPLIT, R.PRUNE):
        for gamma in R.GAMMAS:
            for mo in R.MIN_OPACITIES:
                c = dict(kind=kind, n=n, n_grad=n - 5, grad=grad, scales=scales, opacities=opac, max_radii=radii, thr=R.MASK_THR,
                         gamma=gamma, min_opacity=mo, max_screen_size=R.MASK_SCREEN)
                mask, decided = definition_mask(c)
                und = int((~decided).sum())
                worst = max(worst, und)
                # the cap is a condition on the inputs, not a measurement: a seed that breaks it is replaced, never the cap
                assert und <= n // 100, (kind, gamma, mo, und)
                assert np.array_equal(mask[decided], restatement_mask(c)[decided]), (kind, gamma, mo)
                assert 0 < mask.sum() < n, "both outcomes occur"
    print(f"\nundecided rows of {n} (scale_dims {sd}), worst of every kind, gamma and min_opacity: {worst}")


def measure_split(sd):
    """Largest errors of the restatement's split children against the definition over densify_ref.split_cases(sd), both seeds."""
    out = dict(normal=0.0, step=0.0, scale=0.0)
    for seed in R.SPLIT_SEEDS:
        xi64, r = R.normals(seed, R.SPLIT_ROWS)
        out["normal"] = max(out["normal"], float((np.abs(dz.randn3(seed, R.SPLIT_ROWS) - xi64) / np.maximum(1.0, r)).max()))
        for name, (p, q, s) in R.split_cases(sd).items():
            p32, s32 = dz.split_transform(p, q, s, seed)
            p64, s64, sx = R.split_children(p, q, s, seed, sd)
            out["step"] = max(out["step"], float((np.linalg.norm(p32 - p64, axis=1) / np.linalg.norm(sx, axis=1)).max()))
            out["scale"] = max(out["scale"], float(np.abs(s32 - s64).max()))
    return out


def measure_reset():
    o, above = R.reset_case()
    with np.errstate(over="ignore", divide="ignore"):
        got = dz.inverse_sigmoid(np.minimum(f32(0.1), dz.sigmoid(o)))
    want = R.reset_opacity(o)
    low = np.isfinite(want) & ~above
    assert low.sum() > 200 and above.sum() > 500
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and np.isneginf(want).sum() == 1       # the row at -100
    return float(np.abs(got[low] - want[low]).max()), got, want, above


def test_restatement_error_of_split_children_and_reset_opacity():
    m = measure_split(1)
    for k, v in measure_split(3).items():
        m[k] = max(m[k], v)
    m["reset"], got, want, above = measure_reset()
    print("\nrestatement against the float64 definition, largest error: " + ", ".join(f"{k} {v:.3e}" for k, v in m.items()))
    for k, v in m.items():
        assert 0.5 * R.RESTATEMENT_ERR[k] <= v <= R.RESTATEMENT_ERR[k], (k, v, R.RESTATEMENT_ERR[k])
    # rows above the cut: the restatement returns ONE value, within the reset tolerance of the definition's
    assert np.unique(got[above]).size == 1 and np.unique(want[above]).size == 1
    assert abs(f64(got[above][0]) - want[above][0]) <= R.RESTATEMENT_ERR["reset"]


def test_definition_special_values():
    """What the GPU test asserts by hand, on the definition itself."""
    nan, inf = f32(np.nan), f32(np.inf)
    g = R.grad_mean(f32([0, 2, -2, 1e-30, nan, inf, 3]), f32([0, 0, 0, 1e10, 1, inf, 2]))
    assert np.array_equal(g.view(np.uint32), f32([0, inf, -inf, f32(1e-30) / f32(1e10), 0, 0, 1.5]).view(np.uint32))
    assert 0 < g[3] < np.finfo(f32).tiny, "a subnormal quotient is kept"
    r = R.reset_opacity(f32([nan, -100, 100, 0]))
    assert np.isnan(r[0]) and r[1] == -inf and r[2] == r[3] and abs(r[2] - np.log(1 / 9)) < 1e-7
    # NaN through the restatement as through the definition (np.minimum, np.max propagate it)
    with np.errstate(invalid="ignore"):
        assert np.isnan(dz.inverse_sigmoid(np.minimum(f32(0.1), dz.sigmoid(f32([nan]))))[0])
        assert np.isnan(dz.max_exp_scale(f32([[nan, 0, 0], [0, nan, 0], [0, 0, nan]]))).all()
    # a zero quaternion: NaN points, finite scales
    p, s, _ = R.split_children(np.zeros((2, 3), f32), np.zeros((2, 4), f32), np.zeros((2, 3), f32), 1, 3)
    assert np.isnan(p).all() and np.isfinite(s).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        p32, _ = dz.split_transform(np.zeros((2, 3), f32), np.zeros((2, 4), f32), np.zeros((2, 3), f32), 1)
    assert np.isnan(p32).all()
    # morton: lo, hi (a power-of-two extent: (hi - lo) * inv is exactly 1), outside, NaN, a degenerate axis
    lo, hi = f32([-1, -2, 0.5]), f32([1, 2, 0.5])
    pts = f32([[-1, -2, 0.5], [1, 2, 0.5], [-9, 9, 9], [nan, 0, 0], [inf, -inf, nan]])
    full = np.uint64(2 ** 21 - 1)
    x_all = sum(np.uint64(1) << np.uint64(3 * b) for b in range(21))
    assert full == 2097151
    want = [0, x_all | (x_all << np.uint64(1)), x_all << np.uint64(1), R.morton(f32([[-1, 0, 0.5]]), lo, hi)[0], x_all]
    assert np.array_equal(R.morton(pts, lo, hi), np.asarray(want, np.uint64))
    # compose, gather, nonfinite
    src = np.arange(12, dtype=np.int32).reshape(6, 2)
    assert np.array_equal(R.compose(src, [5, 0], 2, [1, 3], 2, 2, 0), src[[5, 0, 1, 3, 1, 3]])
    assert np.array_equal(R.compose(src, None, 3, [4], 1, 2, 1), np.concatenate([src[:3], np.zeros((2, 2), np.int32)]))
    assert np.array_equal(R.compose(src, [2, 2], 2, None, 0, 0, 0), src[[2, 2]])
    assert np.array_equal(R.gather(src, [3, 3, 0]), src[[3, 3, 0]])
    a = np.zeros((5, 2), f32); a[3] = nan, inf; a[1, 0] = -inf
    cnt, first = R.nonfinite([a, np.full((5, 1), np.finfo(f32).max, f32)])
    assert cnt.tolist() == [2, 0] and first.tolist() == [1, 0xFFFFFFFF]
