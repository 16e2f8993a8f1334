"""The per-Gaussian contribution scores (include/gsr.h: gsr_scores) from the per-pixel float64 DEFINITION of tests/definition_ref.py,
as an INTERVAL per Gaussian, and the comparator of tests/test_scores_cpu.py and tests/test_gpu_contribution_scores.py.

The scores transpose the walk's blend weights w = alpha·T: per Gaussian the count of (pixel, entry) pairs that blend it (hits), the
largest w (max_weight) and the sum of w (weight_sum).  Almost every Gaussian shares a tile with some pixel whose skip / stop
decisions sit on a rounding boundary, so nothing is excluded by tile or by Gaussian; each (pixel, entry) pair is classified:

  sure     blended by the definition, in front of the pixel's first fragile entry, and not itself on the alpha = 1/255 boundary
  unsure   may or may not blend in a correct fp32 evaluation:
             - an entry that is `near_a` (|sigma - ln 255 o| inside definition_ref's window): alpha ~ 1/255, in or out;
             - everything at or behind the pixel's first `near_0` (sigma ~ 0: skipped or blended at full opacity) or `near_t`
               (T' ~ 1e-4: stops here or one entry later) entry that can blend at all (passes the alpha test or sits on one of its
               boundaries) and lies in front of the SURE stop: the stop of the walk with the largest transmittance any evaluation
               can have there (every boundary entry skipped, a stop only at T' < 1e-4 (1 - window)).
  dead     everything else: skipped by the alpha test away from its boundaries, or at / behind a sure stop.
A near_a entry in front changes T for everything behind it by the factor (1 - alpha) with alpha <= (1 + BLEND_MARGIN) / 255: the
relative weight tolerance of every later entry of the pixel widens by that much per such entry, and so does the window of the stop.

  hits        in [#sure, #sure + #unsure]
  max_weight  in [max_sure(w (1 - widen)) - tol, max(max_sure(w (1 + widen)), max_unsure alpha) + tol]       (w <= alpha)
  weight_sum  in [sum_sure w (1 - widen) - (tol + 2^-25) hits_lo, sum_sure w (1 + widen) + sum_unsure alpha + (tol + 2^-25) hits_hi]
On the list scenes of tests/score_scenes.py (tile lists of a chosen length) the hit interval is ONE value for 99.9 % of the Gaussians:
there "inside the interval" is the exact hit count, at every boundary of the scored kernels (tests/test_gpu_score_boundaries.py).
tol = 1e-4: what the suite grants the per-PIXEL sums of the same w (test_gpu_definition.test_covisibility_and_uncertainty,
hip_helpers.compare_forward) — a single w cannot be further off than a sum of them; 2^-25 per term: the fixed point's rounding."""
from types import SimpleNamespace

import numpy as np

import definition_ref as dr

TOL = 1e-4
Q_ONE = float(1 << 24)
Q_HALF_ULP = 2.0 ** -25
WIDEN = (1.0 + dr.BLEND_MARGIN) / 255.0      # one near_a entry in front: T off by at most this factor
SCENES = ("sweep-3", "single-tile", "ragged", "ties") + dr.DEEP   # rgb, rgbd, rgbdn, rgb ties, lists above the 1024 and the 4096 tier
MAX_SLACK, MIN_EXACT = 0.02, 0.40


def intervals(defn):
    """The score intervals of ONE view of the definition `defn` (definition_ref.definition), and the definition's own scores.
    Returns a namespace of (N,) arrays: hits_lo / hits_hi (int64), mw_lo / mw_hi, ws_lo / ws_hi (float64), and hits / bits (uint32:
    the fp32 bits of the largest w) / q (int64: sum of rint(fp32(w) · 2^24)) as the definition itself blends."""
    d, tl = defn.d, defn.tl
    n = d.n
    o_all = dr._f32(defn.fs.opac).reshape(-1)
    hits_lo, hits_un = np.zeros(n, np.int64), np.zeros(n, np.int64)
    mw_lo, mw_hi = np.zeros(n), np.zeros(n)
    ws_lo, ws_hi = np.zeros(n), np.zeros(n)
    hits, q = np.zeros(n, np.int64), np.zeros(n, np.int64)
    mw32 = np.zeros(n, np.float32)
    for t, ids in enumerate(tl.lists):
        if ids.size == 0 or tl.n_rendered == 0:
            continue
        ys, xs = dr._tile_pixels(d, t)
        o = o_all[ids]
        sig, big = dr._sigma(d, ids, ys, xs)
        with np.errstate(all="ignore"):
            alpha = np.minimum(dr.ALPHA_MAX, o[None, :] * np.exp(-sig))
            a_up = np.minimum(dr.ALPHA_MAX, o[None, :] * np.exp(-np.maximum(sig, 0.0))) * (1.0 + 1e-6)   # what it could blend with
            tau = np.log(255.0 * o)
        keep = (sig >= 0) & (alpha >= dr.ALPHA_MIN)
        al = np.where(keep, alpha, 0.0)
        Tn = np.cumprod(1.0 - al, 1)
        stop = keep & (Tn < dr.T_MIN)
        nstop = np.cumsum(stop, 1)
        dead = nstop > 0
        met = ~dead | (stop & (nstop == 1))
        blended = keep & ~dead
        alb = np.where(blended, al, 0.0)
        Tincl = np.cumprod(1.0 - alb, 1)
        Texcl = np.concatenate([np.ones((ys.size, 1)), Tincl[:, :-1]], 1)
        w = alb * Texcl
        can = (o >= dr.ALPHA_MIN)[None, :] & np.isfinite(tau)[None, :]
        with np.errstate(invalid="ignore"):
            near_a = can & (np.abs(sig - tau[None, :]) <= dr.SIGMA_ULPS * dr.EPS32 * np.maximum(big, np.abs(tau)[None, :]))
        near_0 = can & (sig <= dr.SIGMA_ULPS * dr.EPS32 * big) & (sig >= -dr.SIGMA_ULPS * dr.EPS32 * big)
        # near_a entries in front of an entry (met ones: nothing behind the stop acts on T), and what they widen
        ka = np.cumsum(near_a & met, 1) - (near_a & met)
        widen = ka * WIDEN
        near_t = keep & (np.abs(Tn - dr.T_MIN) <= (dr.T_WINDOW + widen) * dr.T_MIN)
        frag = met & (near_0 | near_t | (stop & near_a))     # (a stopping entry on the alpha boundary: skipped, the walk goes on)
        behind = np.cumsum(frag, 1) > 0                      # at or behind the pixel's first fragile entry
        # the walk of the largest transmittance: boundary entries skipped, a stop only where every evaluation stops
        al_hi = np.where(keep & ~near_a & ~near_0, alpha, 0.0)
        Tn_hi = np.cumprod(1.0 - al_hi, 1)
        sure_dead = np.cumsum((al_hi > 0) & (Tn_hi < dr.T_MIN * (1.0 - dr.T_WINDOW)), 1) > 0    # the sure stop and behind it
        possible = keep | near_a | near_0
        sure = blended & ~behind & ~near_a
        unsure = possible & ~sure_dead & (behind | (near_a & met & ~dead)) & ~sure
        assert not (blended & ~sure & ~unsure).any(), "a blended entry is neither sure nor unsure"
        wl, wh = np.where(sure, w * (1.0 - widen), 0.0), np.where(sure, w * (1.0 + 1.01 * widen), 0.0)
        au = np.where(unsure, a_up, 0.0)
        hits_lo[ids] += sure.sum(0)
        hits_un[ids] += unsure.sum(0)
        mw_lo[ids] = np.maximum(mw_lo[ids], wl.max(0))
        mw_hi[ids] = np.maximum(mw_hi[ids], np.maximum(wh.max(0), au.max(0)))
        ws_lo[ids] += wl.sum(0)
        ws_hi[ids] += wh.sum(0) + au.sum(0)
        # the definition's own scores
        w32 = np.where(blended, w, 0.0).astype(np.float32)
        hits[ids] += blended.sum(0)
        mw32[ids] = np.maximum(mw32[ids], w32.max(0))
        q[ids] += np.rint(w32.astype(np.float64) * Q_ONE).astype(np.int64).sum(0)
    hits_hi = hits_lo + hits_un
    return SimpleNamespace(n=n, hits_lo=hits_lo, hits_hi=hits_hi,
                           mw_lo=np.where(hits_lo > 0, np.maximum(mw_lo - TOL, 0.0), 0.0), mw_hi=np.where(hits_hi > 0, mw_hi + TOL, 0.0),
                           ws_lo=np.maximum(ws_lo - (TOL + Q_HALF_ULP) * hits_lo, 0.0), ws_hi=ws_hi + (TOL + Q_HALF_ULP) * hits_hi,
                           hits=hits, bits=mw32.view(np.uint32).copy(), q=q)


def accumulate(*ivs):
    """The intervals (and the definition's scores) of several views accumulated into one set: (+, max, +)."""
    out = SimpleNamespace(n=ivs[0].n)
    for k in ("hits_lo", "hits_hi", "ws_lo", "ws_hi", "hits", "q"):
        setattr(out, k, sum(getattr(iv, k) for iv in ivs))
    for k in ("mw_lo", "mw_hi", "bits"):
        setattr(out, k, np.maximum.reduce([getattr(iv, k) for iv in ivs]))
    return out


_intervals = {}


def scene_intervals(pkg, name):
    """intervals(definition(name)): computed once, shared, read-only."""
    if name not in _intervals:
        iv = intervals(dr.definition(pkg, name))
        for v in vars(iv).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _intervals[name] = iv
    return _intervals[name]


def shares(iv):
    """(total slack of the hit intervals sum(hi - lo) / sum(lo), share of the Gaussians with hi > 0 whose interval is one value)."""
    live = iv.hits_hi > 0
    return float((iv.hits_hi - iv.hits_lo).sum()) / max(1, int(iv.hits_lo.sum())), float((iv.hits_hi == iv.hits_lo)[live].mean())


def conditions(iv, name=""):
    """The caps a scene must meet for its intervals to say anything; prints the measured shares."""
    slack, exact = shares(iv)
    print(f"scores {name}: {int((iv.hits_hi > 0).sum())} of {iv.n} Gaussians can be hit, hits in [{int(iv.hits_lo.sum())}, "
          f"{int(iv.hits_hi.sum())}], slack {slack:.5f}, exact share {exact:.3f}")
    assert slack <= MAX_SLACK, (name, slack)
    assert exact >= MIN_EXACT, (name, exact)


def got_from_definition(iv):
    """(bits uint32, hits int64, q int64) as the definition itself blends (writable copies: the mutation tests corrupt them)."""
    return iv.bits.copy(), iv.hits.copy(), iv.q.copy()


def check_scores(iv, bits, hits, q):
    """The three score arrays of a forward (max_weight's bits as uint32, hits, weight_sum in units of 2^-24) against the intervals.
    Returns the worst |max_weight - definition| and |weight_sum - definition| / hits over the Gaussians whose hits are exact."""
    bits, hits, q = (np.asarray(a) for a in (bits, hits, q))
    assert bits.shape == hits.shape == q.shape == (iv.n,)
    mw = bits.astype(np.uint32).view(np.float32).astype(np.float64)
    hits = hits.astype(np.int64)
    ws = q.astype(np.float64) / Q_ONE
    bad = np.flatnonzero((hits < iv.hits_lo) | (hits > iv.hits_hi))
    assert bad.size == 0, f"hits outside the interval at {bad[:5]}: {hits[bad[:5]]} not in [{iv.hits_lo[bad[:5]]}, {iv.hits_hi[bad[:5]]}]"
    assert np.isfinite(mw).all()
    bad = np.flatnonzero((mw < iv.mw_lo) | (mw > iv.mw_hi))
    assert bad.size == 0, f"max_weight outside the interval at {bad[:5]}: {mw[bad[:5]]} not in [{iv.mw_lo[bad[:5]]}, {iv.mw_hi[bad[:5]]}]"
    bad = np.flatnonzero((ws < iv.ws_lo) | (ws > iv.ws_hi))
    assert bad.size == 0, f"weight_sum outside the interval at {bad[:5]}: {ws[bad[:5]]} not in [{iv.ws_lo[bad[:5]]}, {iv.ws_hi[bad[:5]]}]"
    zero = hits == 0
    assert np.array_equal(zero, bits == 0) and np.array_equal(zero, q == 0), "hits == 0 <=> max_weight == 0 <=> weight_sum == 0"
    exact = (iv.hits_hi == iv.hits_lo) & (iv.hits_hi > 0)
    mw_def = iv.bits.view(np.float32).astype(np.float64)
    worst_mw = float(np.abs(mw - mw_def)[exact].max()) if exact.any() else 0.0
    worst_ws = float((np.abs(ws - iv.q / Q_ONE)[exact] / iv.hits_hi[exact]).max()) if exact.any() else 0.0
    return dict(worst_max_weight=worst_mw, worst_weight_sum_per_hit=worst_ws, exact=int(exact.sum()))
