"""The list scenes of tests/list_scenes.py as DEFINITIONS (tests/definition_ref.py) with score intervals (tests/scores_ref.py): tile
lists of a chosen length AFTER definition_ref.robust_scene, for tests/test_gpu_score_boundaries.py and its premises in
tests/test_scores_cpu.py.

robust_scene removes the Gaussians whose radius / rect decisions sit on a rounding edge, which shortens a list: single_tile_scene(
1023, 7) arrives with 1022 entries.  A boundary test needs the length it asked for, so
  * the one-tile builders take the smallest seed (from the builder's usual one) at which the filter removes nothing — SEEDS,
    re-derived by smallest_whole_seed in the CPU test;
  * where no seed below 60 does (8193 entries in one tile; every many_tile_scene, whose off-axis tiles lose about 0.15 %), each list
    is built EXTRA(L) entries longer and trimmed as a pure function of the scene: the fragile entries first, then unpinned front
    splats from the back of the list.  The builders pin boundary_positions(L', slack = EXTRA): whatever is dropped, the entries that
    end within 2 positions of a boundary of the FINAL list, first and last were pinned, and an unpinned one never ends there.
Fragility is a per-Gaussian decision (the near-tie rule names the higher id of a PAIR: dropping one of two never creates a pair), so
a trimmed scene has nothing fragile left; `definition` asserts it.

A case is a tuple: ("full", L), ("walled", L, stop), ("two", L) (+ list_scenes.TWO_TILE_SECOND in the second tile), ("tied", L)
(groups of TIED_GROUPS) or ("grid",) (GRID_LENGTHS on a 4 x 3 grid).  numpy only; nothing here computes with the oracle or the product."""
import numpy as np

import definition_ref as dr
import fuzz_scenes as fz
import list_scenes as ls
import scores_ref as sr

BG = (0.3, 0.1, 0.6)
MAX_SLACK, MIN_EXACT = 1e-3, 0.99       # these scenes allow it (measured: <= 6e-5, >= 0.999); sr.MAX_SLACK / MIN_EXACT are the fuzz scenes'

FULL_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1088, 1089, 2049, 4096, 4097, 8193)
MODE_LENGTHS = (256, 257, 1024, 1025)                       # the :rgbd and :rgbdn twins
WALLED = ((1000, 2), (1000, 64), (1000, 65), (1000, 256), (1000, 257), (1000, 512), (2500, 1024), (2500, 1025), (2500, 1089))
TWO_LENGTHS = (1024, 1025)
TIED_LENGTHS = (257, 1024, 1025)
TIED_GROUPS = 5
GRID = (4, 3)
GRID_LENGTHS = (1025, 10, 4097, 256, 1024, 257, 64, 2049, 65, 1, 8193, 10)
GRID_SEED = 5
TRIMMED_FULL = (8193,)                                      # no seed below 60 leaves these whole

FIRST_SEED = {"full": 7, "walled": 11, "two": 13, "tied": 17}
# case -> the smallest seed >= FIRST_SEED[kind] at which robust_scene removes nothing (cases not listed: FIRST_SEED itself)
SEEDS = {("full", 512): 8, ("full", 769): 9, ("full", 1023): 9, ("full", 1089): 9, ("full", 2049): 19, ("full", 4096): 40,
         ("walled", 1000, 65): 12, ("walled", 1000, 256): 15, ("walled", 1000, 512): 16, ("walled", 2500, 1024): 23,
         ("walled", 2500, 1025): 34, ("walled", 2500, 1089): 23,
         ("two", 1024): 15, ("two", 1025): 17,
         ("tied", 1024): 19, ("tied", 1025): 21}

CASES = (tuple(("full", L) for L in FULL_LENGTHS) + tuple(("walled",) + c for c in WALLED) + tuple(("two", L) for L in TWO_LENGTHS)
         + tuple(("tied", L) for L in TIED_LENGTHS) + (("grid",),))


def case_id(case):
    return "-".join(str(x) for x in case)


def extra(L):
    """Entries a trimmed list is built longer by: 2 + one per 256 (the filter takes about 0.15 %)."""
    return 2 + (L + 255) // 256


def seed_of(case):
    return SEEDS.get(case, FIRST_SEED[case[0]])


def lengths_of(case):
    """The list length per tile, row-major, that the case asks for."""
    if case[0] == "two":
        return (case[1], ls.TWO_TILE_SECOND)
    return GRID_LENGTHS if case[0] == "grid" else (case[1],)


def _built(case, seed, deg):
    kind = case[0]
    if kind == "full":
        return ls.single_tile_scene(case[1], seed, deg)
    if kind == "walled":
        return ls.walled_scene(case[1], case[2], seed, deg)
    if kind == "two":
        return ls.two_tile_scene(case[1], ls.TWO_TILE_SECOND, seed, deg)
    assert kind == "tied"
    return ls.tied_tile_scene(case[1], TIED_GROUPS, seed, deg)


def _fragile(sc):
    return dr.decide(sc.means, sc.scales, sc.rots, sc.cam).fragile_gaussian


def smallest_whole_seed(case, limit=60):
    """The smallest seed in [FIRST_SEED[kind], limit) at which the case's scene has no fragile Gaussian, or None."""
    for seed in range(FIRST_SEED[case[0]], limit):
        if not _fragile(_built(case, seed, 0)).any():
            return seed
    return None


def trim(sc, built, want, slack):
    """`sc` whose tile lists are sc.order cut into `built` lengths, without built[t] - want[t] entries of list t: every fragile
    entry, then the unpinned ones (not in boundary_positions(built[t], slack=slack)) from the back of the list — in the tiny lists
    that are pinned throughout, whatever sits at the back.  Returns the five arrays of the Gaussians that stay."""
    frag = _fragile(sc)
    keep = np.ones(sc.means.shape[0], bool)
    start = 0
    for Lb, Lw in zip(built, want):
        ids = sc.order[start:start + Lb]
        start += Lb
        fr = frag[ids]
        more = Lb - Lw - int(fr.sum())
        assert 0 <= Lb - Lw <= slack and more >= 0, f"a list of {Lb} entries has {int(fr.sum())} fragile ones: more than the {Lb - Lw} it can lose"
        pinned = np.zeros(Lb, bool)
        pinned[ls.boundary_positions(Lb, slack=slack)] = True
        free = np.flatnonzero(~fr & ~pinned)
        if free.size < more:
            free = np.flatnonzero(~fr)
        drop = np.concatenate([np.flatnonzero(fr), free[free.size - more:]])
        keep[ids[drop]] = False
    return tuple(np.ascontiguousarray(a[keep]) for a in sc.args)


def fuzz_scene(case, mode="rgb", bg=BG, deg=0):
    """The case's scene as a fuzz_scenes.FuzzScene (trimmed where the case needs it), and the list lengths it asks for."""
    want = lengths_of(case)
    if case[0] == "grid":
        slack = max(extra(L) for L in want)
        built = tuple(L + extra(L) for L in want)
        sc = ls.many_tile_scene(*GRID, built, GRID_SEED, deg, slack=slack)
        args = trim(sc, built, want, slack)
    elif case[0] == "full" and case[1] in TRIMMED_FULL:
        built = (case[1] + extra(case[1]),)
        sc = ls.single_tile_scene(built[0], seed_of(case), deg)
        assert not _fragile(sc)[-1], "the backdrop must stay"
        args = trim(sc, built, want, extra(case[1]))
    else:
        sc = _built(case, seed_of(case), deg)
        args = sc.args
    rng = np.random.default_rng([sum(want), len(mode), deg])
    return fz.FuzzScene(*args, sc.cam, deg, mode, tuple(bg), rng), want


_definitions, _intervals = {}, {}


def definition(case, mode="rgb", bg=BG, deg=0):
    """dr.define(dr.robust_scene(fuzz_scene(case))), whose lists have the lengths asked for (`defn.lengths`) because the filter
    removed nothing (`defn.shares["removed"]`): computed once, shared, read-only like dr.definition's."""
    key = (case, mode, tuple(bg), deg)
    if key not in _definitions:
        fs, want = fuzz_scene(case, mode, bg, deg)
        fs = dr.robust_scene(fs)
        assert fs.note["removed"][0] == 0, (case, fs.note["removed"])
        defn = dr.define(fs)
        defn.name, defn.case, defn.lengths = case_id(case), case, tuple(want)
        assert tuple(len(l) for l in defn.tl.lists) == defn.lengths, (case, [len(l) for l in defn.tl.lists])
        dr._freeze(defn)
        for a in (fs.means, fs.shs, fs.opac, fs.scales, fs.rots):
            a.setflags(write=False)
        _definitions[key] = defn
    return _definitions[key]


def intervals(case, deg=0):
    """sr.intervals of the case's definition (they depend on geometry and opacity alone, not on mode or background): once, read-only."""
    if (case, deg) not in _intervals:
        have = [d for (c, _, _, g), d in _definitions.items() if c == case and g == deg]
        iv = sr.intervals(have[0] if have else definition(case, deg=deg))
        for v in vars(iv).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _intervals[case, deg] = iv
    return _intervals[case, deg]


def conditions(case, defn, iv):
    """What a boundary case must meet, on the definition alone; prints the post-filter list lengths, slack and exact share."""
    dr.conditions(defn)
    slack, exact = sr.shares(iv)
    removed = defn.shares["removed"]
    print(f"score scene {defn.name}: list lengths {list(len(l) for l in defn.tl.lists)} (asked {list(defn.lengths)}), filter removed "
          f"{removed[0]} of {removed[1]}, hits in [{int(iv.hits_lo.sum())}, {int(iv.hits_hi.sum())}], slack {slack:.2e}, exact share "
          f"{exact:.4f}, never hit {int((iv.hits_hi == 0).sum())}")
    assert tuple(len(l) for l in defn.tl.lists) == defn.lengths == tuple(lengths_of(case))
    assert removed[0] == 0 and removed[1] == defn.d.n == sum(defn.lengths)
    assert slack <= MAX_SLACK, (defn.name, slack)
    assert exact >= MIN_EXACT, (defn.name, exact)
    assert (iv.hits_lo <= iv.hits).all() and (iv.hits <= iv.hits_hi).all()
    stop = case[2] if case[0] == "walled" else None
    for t, ids in enumerate(defn.tl.lists):
        # (the stop's neighbourhood: the walls and what stands in front of them; behind the stop nothing is hit)
        P = ls.boundary_positions(len(ids), stop)
        P = P[P < stop] if stop is not None else P
        dark = P[iv.hits_lo[ids[P]] < 1]
        assert dark.size == 0, f"{defn.name}, tile {t}: the entries at {dark} next to a boundary are not surely hit"
    if stop is not None:
        ids = defn.tl.lists[0]
        assert (defn.r.n_contrib == stop).all(), "every pixel's walk ends at the stop"
        assert not iv.hits_hi[ids[stop:]].any(), "an entry behind the stop can be hit"
        assert (iv.hits_lo[ids[stop - 2:stop]] == defn.d.W * defn.d.H).all(), "both blended walls are hit at every pixel"
    elif case[0] in ("full", "tied"):
        assert (defn.r.n_contrib == defn.lengths[0]).all(), "every pixel walks the list to its end"
