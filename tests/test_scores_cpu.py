"""No GPU: the premises of the contribution-score comparator (tests/scores_ref.py) and the argument contracts of the new entry
points that fail before any launch.

  per scene of scores_ref.SCENES: the interval caps (total slack of the hit counts <= 2 %, at least 40 % of the Gaussians that can
      be hit at all have a one-value interval), printed;
  the comparator's own test: scores made from the definition pass; four mutations fail — one Gaussian's hits beyond its slack, a
      max_weight raised by 2 tol on a Gaussian with sure hits only, a view dropped from a two-view accumulation, two rows swapped;
  the list scenes of tests/score_scenes.py (the cases of tests/test_gpu_score_boundaries.py): the seeds re-derived, the post-filter
      list lengths the ones asked for, nothing removed, slack <= 1e-3 and exact share >= 0.99, every entry next to a boundary surely
      hit, nothing behind a stop hit — printed per case; five mutations the scored kernels could produce fail check_scores;
  gsr_forward_scored / gsr_contribution_mask reject NULL, misaligned and unknown arguments with GSR_E_INVALID_ARG, and the Python
      layer rejects CPU tensors, unknown rules and bad thresholds."""
import ctypes as C

import numpy as np
import pytest

import definition_ref as dr
import list_scenes as ls
import score_scenes as ss
import scores_ref as sr


@pytest.mark.parametrize("name", sr.SCENES)
def test_scene_meets_the_interval_caps(pkg, name):
    defn = dr.definition(pkg, name)
    dr.conditions(defn)
    iv = sr.scene_intervals(pkg, name)
    sr.conditions(iv, name)
    assert (iv.hits_lo <= iv.hits).all() and (iv.hits <= iv.hits_hi).all()
    assert not iv.hits_hi[~defn.d.visible].any(), "a culled Gaussian cannot be hit"


def test_tier_scenes_have_the_lists_they_are_there_for(pkg):
    assert dr.definition(pkg, "deep-276").shares["longest"] > 1024
    assert dr.definition(pkg, "deep-5911").shares["longest"] > 4096


@pytest.mark.parametrize("name", sr.SCENES)
def test_definitions_own_scores_pass(pkg, name):
    iv = sr.scene_intervals(pkg, name)
    m = sr.check_scores(iv, *sr.got_from_definition(iv))
    assert m["worst_max_weight"] == 0.0 and m["worst_weight_sum_per_hit"] == 0.0
    two = sr.accumulate(iv, iv)
    bits, hits, q = sr.got_from_definition(iv)
    sr.check_scores(two, bits, 2 * hits, 2 * q)


def _sure_gaussian(iv):
    """A Gaussian with sure hits only whose max_weight interval is the plain +- tol (nothing widened it)."""
    mw = iv.bits.view(np.float32).astype(np.float64)
    ok = np.flatnonzero((iv.hits_hi == iv.hits_lo) & (iv.hits_lo > 0) & (iv.mw_hi - mw <= 1.5 * sr.TOL))
    assert ok.size, "no Gaussian with an unwidened interval"
    return int(ok[0])


@pytest.mark.parametrize("name", ["sweep-3", "ragged", "deep-276"])
def test_mutations_fail(pkg, name):
    iv = sr.scene_intervals(pkg, name)
    g = _sure_gaussian(iv)
    # one Gaussian's hits beyond its slack
    bits, hits, q = sr.got_from_definition(iv)
    worst = int(np.argmax(iv.hits_hi - iv.hits_lo))
    hits[worst] = iv.hits_lo[worst] + (iv.hits_hi[worst] - iv.hits_lo[worst]) + 1
    with pytest.raises(AssertionError, match="hits outside"):
        sr.check_scores(iv, bits, hits, q)
    # a max_weight raised by 2 tol on a sure Gaussian
    bits, hits, q = sr.got_from_definition(iv)
    w = np.float32(bits[g:g + 1].view(np.float32)[0] + np.float32(2 * sr.TOL))
    bits[g] = np.array([w], np.float32).view(np.uint32)[0]
    with pytest.raises(AssertionError, match="max_weight outside"):
        sr.check_scores(iv, bits, hits, q)
    # a dropped view in a two-view accumulation
    two = sr.accumulate(iv, iv)
    with pytest.raises(AssertionError, match="hits outside"):
        sr.check_scores(two, *sr.got_from_definition(iv))
    # two Gaussians' rows swapped
    a = int(np.argmax(iv.hits_lo))
    below = np.flatnonzero(iv.hits_hi < iv.hits_lo[a])
    assert below.size, "no two Gaussians with disjoint hit intervals"
    b = int(below[0])
    got = sr.got_from_definition(iv)
    for arr in got:
        arr[[a, b]] = arr[[b, a]]
    with pytest.raises(AssertionError, match="hits outside"):
        sr.check_scores(iv, *got)


@pytest.mark.parametrize("case", ss.CASES, ids=ss.case_id)
def test_list_scene_has_the_lengths_asked_for_and_exact_hit_counts(case):
    if case[0] != "grid" and not (case[0] == "full" and case[1] in ss.TRIMMED_FULL):
        assert ss.smallest_whole_seed(case) == ss.seed_of(case), "SEEDS must hold the smallest seed the filter leaves whole"
    defn = ss.definition(case)
    again = dr.robust_scene(defn.fs)
    assert again.note["removed"] == (0, sum(ss.lengths_of(case))), "robust_scene removes nothing from the delivered scene"
    ss.conditions(case, defn, ss.intervals(case))


@pytest.mark.parametrize("mode", ["rgbd", "rgbdn"])
@pytest.mark.parametrize("L", ss.MODE_LENGTHS)
def test_list_scene_mode_twins_are_the_same_lists(L, mode):
    a, b = ss.definition(("full", L)), ss.definition(("full", L), mode)
    assert b.fs.mode == mode and b.lengths == (L,) and np.array_equal(a.tl.values_sorted, b.tl.values_sorted)
    assert np.array_equal(a.fs.opac, b.fs.opac) and np.array_equal(a.d.conic, b.d.conic)   # the intervals read nothing else


def test_trimmed_scenes_lose_only_what_was_built_on_top():
    """The trimming of ss.fuzz_scene: every fragile Gaussian goes, and with the others dropped exactly extra(L) entries per list."""
    want = ss.GRID_LENGTHS
    slack = max(ss.extra(L) for L in want)
    built = tuple(L + ss.extra(L) for L in want)
    sc = ls.many_tile_scene(*ss.GRID, built, ss.GRID_SEED, 0, slack=slack)
    frag = ss._fragile(sc)
    assert frag.any(), "the grid is trimmed because the filter takes some of it"
    args = ss.trim(sc, built, want, slack)
    assert args[0].shape[0] == sum(want)
    kept = {a.tobytes() for a in args[0]}
    assert not any(m.tobytes() in kept for m in sc.means[frag]), "a fragile Gaussian stayed"


def _list_ids(case):
    return ss.definition(case).tl.lists[0]


def test_mutations_of_the_scored_kernels_fail():
    # a dropped chunk flush: positions 256 .. 511 of a list of 1025 never reach the arrays
    case = ("full", 1025)
    iv, ids = ss.intervals(case), _list_ids(case)
    sr.check_scores(iv, *sr.got_from_definition(iv))
    got = sr.got_from_definition(iv)
    for a in got:
        a[ids[256:512]] = 0
    with pytest.raises(AssertionError, match="hits outside"):
        sr.check_scores(iv, *got)
    # position 255's words credited to position 256
    bits, hits, q = sr.got_from_definition(iv)
    a, b = ids[255], ids[256]
    bits[b], hits[b], q[b] = max(bits[a], bits[b]), hits[a] + hits[b], q[a] + q[b]
    bits[a] = hits[a] = q[a] = 0
    with pytest.raises(AssertionError, match="hits outside"):
        sr.check_scores(iv, bits, hits, q)
    # every count doubled: a view taken twice
    bits, hits, q = sr.got_from_definition(iv)
    with pytest.raises(AssertionError, match="hits outside"):
        sr.check_scores(iv, bits, 2 * hits, 2 * q)
    # one hit behind the stop
    case = ("walled", 1000, 257)
    iv, ids = ss.intervals(case), _list_ids(case)
    bits, hits, q = sr.got_from_definition(iv)
    g = ids[257 + 1]
    assert hits[g] == 0
    bits[g], hits[g], q[g] = np.float32(0.004).view(np.uint32), 1, int(0.004 * sr.Q_ONE)
    with pytest.raises(AssertionError, match="hits outside"):
        sr.check_scores(iv, bits, hits, q)
    # max_weight of the last entry of a 64-entry batch of the tier walk (position 1024 + 63) swapped with the next batch's first
    case = ("full", 1089)
    iv, ids = ss.intervals(case), _list_ids(case)
    bits, hits, q = sr.got_from_definition(iv)
    a, b = ids[1087], ids[1088]
    assert abs(float(bits[a:a + 1].view(np.float32)[0]) - float(bits[b:b + 1].view(np.float32)[0])) > 4 * sr.TOL
    bits[a], bits[b] = bits[b], bits[a]
    with pytest.raises(AssertionError, match="max_weight outside"):
        sr.check_scores(iv, bits, hits, q)


def test_scored_entry_points_reject_bad_arguments_before_any_launch(pkg):
    L = pkg._lib
    lib = L.load()
    assert C.sizeof(L.Scores) == 32
    assert lib.gsr_forward_scored(None, None, None, None, None, None, None, None) == L.GSR_E_INVALID_ARG
    ok = L.Scores(None, None, None, 0, 0)
    assert lib.gsr_forward_scored(None, None, None, None, None, C.byref(ok), None, None) == L.GSR_E_INVALID_ARG
    for sc, word in ((L.Scores(None, None, None, 1, 0), b"gsr_scores.flags"), (L.Scores(None, None, None, 0, 7), b"gsr_scores.flags"),
                     (L.Scores(None, 0x1004, None, 0, 0), b"aligned"), (L.Scores(None, None, 0x1004, 0, 0), b"aligned"),
                     (L.Scores(0x1002, None, None, 0, 0), b"aligned")):
        assert lib.gsr_forward_scored(None, None, None, None, None, C.byref(sc), None, None) == L.GSR_E_INVALID_ARG
        assert word in lib.gsr_last_error_string(), lib.gsr_last_error_string()
    mask = lib.gsr_contribution_mask
    assert mask(4, 3, 0.5, None, None, None, None, None) == L.GSR_E_INVALID_ARG and b"rule" in lib.gsr_last_error_string()
    assert mask(4, -1, 0.5, None, None, None, None, None) == L.GSR_E_INVALID_ARG
    assert mask(-1, 0, 0.5, None, None, None, None, None) == L.GSR_E_INVALID_ARG
    for bad in (-0.5, float("nan"), float("inf")):
        assert mask(4, 0, bad, None, None, None, None, None) == L.GSR_E_INVALID_ARG and b"threshold" in lib.gsr_last_error_string()
    assert mask(4, L.SCORE_HITS, 1e30, None, None, None, None, None) == L.GSR_E_INVALID_ARG
    for rule in (L.SCORE_MAX_WEIGHT, L.SCORE_WEIGHT_SUM, L.SCORE_HITS):
        assert mask(4, rule, 0.5, None, None, None, None, None) == L.GSR_E_INVALID_ARG and b"null" in lib.gsr_last_error_string()
        assert mask(0, rule, 0.5, None, None, None, None, None) == L.GSR_OK            # nothing to do
    assert mask(4, L.SCORE_HITS, 1.0, None, 0x1004, None, 0x2000, None) == L.GSR_E_INVALID_ARG and b"aligned" in lib.gsr_last_error_string()
    assert mask(4, L.SCORE_WEIGHT_SUM, 1.0, None, None, 0x1004, 0x2000, None) == L.GSR_E_INVALID_ARG


def test_python_layer_rejects_cpu_tensors_and_bad_rules(pkg):
    K = pkg.contribution
    with pytest.raises(ValueError, match="HIP device"):
        K.ContributionScores(8, "cpu")
    with pytest.raises(ValueError, match="unknown rule"):
        K._check_rule("median", 0.1)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="threshold"):
            K._check_rule("hits", bad)
    with pytest.raises(TypeError):
        K.prune_mask(np.zeros(4), "hits", 1)
    assert K.RULES == {"max_weight": 0, "weight_sum": 1, "hits": 2}
