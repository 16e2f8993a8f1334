"""Per-Gaussian contribution scores of a set of views, and pruning by them (include/gsr.h: gsr_forward_scored,
gsr_contribution_mask).  No reference counterpart: the reference prunes by opacity and screen size only (densification.jl:18-25).

The scores come from the compositing walk's blend weight w = alpha·T of Gaussian g at pixel p:
  max_weight  max over pixels and views of w — RadSplat's score (Niemeyer et al. 2024, eq. 7-8; prune below 0.01)
  weight_sum  sum of w, hits: the number of (pixel, view) pairs that blend g — the importance terms of LightGaussian
              (Fan et al. 2023) and Mini-Splatting (Fang & Wang 2024), without their volume weighting
all three accumulated as INTEGERS by the scored forward kernels (csrc/composite.hip), so they are bit-identical from run to run
and whatever path a view takes through the library.

  ContributionScores(n, device)   the three accumulators
  score_views(rast, gs_tensors, cameras, sh_degree, background)   one forward-only scored render per camera
  prune_mask(scores, rule, threshold)       uint8 keep mask (gsr_contribution_mask)
  prune_by_contribution(strategy, gs, optimizers, scores, rule, threshold)   through densification.prune_points
"""
from __future__ import annotations

import math

import torch

from . import _lib as L

RULES = {"max_weight": L.SCORE_MAX_WEIGHT, "weight_sum": L.SCORE_WEIGHT_SUM, "hits": L.SCORE_HITS}
WEIGHT_ONE = float(1 << 24)  # weight_sum's fixed point: q = round-to-nearest-even(w · 2^24)


class ContributionScores:
    """The three per-Gaussian accumulators of gsr_scores for a model of `n` Gaussians, zero-initialised on `device`.
    They are accumulated into by every scored forward and never cleared by the library: `zero_()` starts a new round.
      bits        int32 (n): the bits of max_weight;  `max_weight`: the same memory viewed as float32
      hits        int64 (n)
      q           int64 (n): weight_sum in units of 2^-24;  `weight_sum`: float64 = q / 2^24 (a new tensor)
      n_views     scored forwards since the last zero_()"""

    def __init__(self, n: int, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("ContributionScores live on the HIP device (no CPU path)")
        if n < 0:
            raise ValueError("negative n")
        self.n = int(n)
        self.bits = torch.zeros(self.n, dtype=torch.int32, device=device)
        self.hits = torch.zeros(self.n, dtype=torch.int64, device=device)
        self.q = torch.zeros(self.n, dtype=torch.int64, device=device)
        self.n_views = 0

    @property
    def device(self):
        return self.bits.device

    @property
    def max_weight(self) -> torch.Tensor:
        return self.bits.view(torch.float32)

    @property
    def weight_sum(self) -> torch.Tensor:
        return self.q.to(torch.float64) / WEIGHT_ONE

    def zero_(self):
        self.bits.zero_(); self.hits.zero_(); self.q.zero_()
        self.n_views = 0
        return self

    def as_struct(self, n: int, device) -> L.Scores:
        """The gsr_scores of a forward on `n` Gaussians on `device`."""
        if n != self.n:
            raise ValueError(f"scores of {self.n} Gaussians on a model of {n}")
        want = torch.device(device)
        if want.index is not None and self.device.index is not None and want.index != self.device.index:
            raise ValueError(f"scores on {self.device}, forward on {want}")
        return L.Scores(L.ptr(self.bits, True), L.ptr(self.hits, True), L.ptr(self.q, True), 0, 0)


def score_views(rast, gs_tensors, cameras, sh_degree, background=(0.0, 0.0, 0.0), scores=None) -> ContributionScores:
    """One forward-only scored render per camera of `cameras`, accumulated into `scores` (a new ContributionScores when None).
    gs_tensors = (means_3d, shs, opacities_act, scales_act, rotations), the arguments of `forward_raw`.  No read-back and no
    torch arithmetic on the scores: V launches of the scored forward, nothing else."""
    means_3d = gs_tensors[0]
    if scores is None:
        scores = ContributionScores(int(means_3d.shape[0]), means_3d.device)
    bg = tuple(float(b) for b in background)
    for camera in cameras:
        rast.forward_raw(*gs_tensors, camera, sh_degree, bg, forward_only=True, scores=scores)
    return scores


def _check_rule(rule, threshold):
    if rule not in RULES:
        raise ValueError(f"unknown rule {rule!r}: one of {sorted(RULES)}")
    threshold = float(threshold)
    if not (math.isfinite(threshold) and threshold >= 0.0):
        raise ValueError("threshold must be finite and >= 0")
    return RULES[rule], threshold


def prune_mask(scores: ContributionScores, rule: str = "max_weight", threshold: float = 0.01) -> torch.Tensor:
    """uint8 (n): 1 where the Gaussian is KEPT — score >= threshold, compared in the score's own integers
    (gsr_contribution_mask).  rule: "max_weight" (threshold 0.01 is RadSplat's published value, only a default), "weight_sum",
    "hits"."""
    kind, threshold = _check_rule(rule, threshold)
    if not isinstance(scores, ContributionScores):
        raise TypeError("scores must be a ContributionScores")
    valid = torch.empty(scores.n, dtype=torch.uint8, device=scores.device)
    with torch.cuda.device(scores.device):
        L.check(L.load().gsr_contribution_mask(scores.n, kind, threshold, L.ptr(scores.bits, True), L.ptr(scores.hits, True),
                                               L.ptr(scores.q, True), L.ptr(valid, True), L.stream()))
    return valid


def prune_by_contribution(strategy, gs, optimizers, scores: ContributionScores, rule: str = "max_weight",
                          threshold: float = 0.01) -> int:
    """Remove the Gaussians `prune_mask(scores, rule, threshold)` does not keep, through `densification.prune_points`: the
    model's rows, both Adam moments and the strategy's statistics go through that one row composition.  Returns the number
    removed.  `scores` must be of this model as it is now (score it after the last densification).

    `strategy` is a `DefaultStrategy`.  An `MCMCStrategy` is REFUSED with a TypeError: it holds the model at a fixed budget and
    replaces dead Gaussians by relocation (mcmc.relocate), its row composition has no pruning form, and dropping rows behind its
    back would leave its budget accounting wrong — relocate by score there instead."""
    from . import densification as D
    if not isinstance(strategy, D.DefaultStrategy):
        raise TypeError(f"prune_by_contribution works with DefaultStrategy, not {type(strategy).__name__}: an MCMCStrategy "
                        "keeps a fixed budget and relocates instead of pruning")
    if scores.n != len(gs):
        raise ValueError(f"scores of {scores.n} Gaussians on a model of {len(gs)}")
    valid = prune_mask(scores, rule, threshold)
    before = len(gs)
    D.prune_points(strategy, gs, optimizers, valid)
    return before - len(gs)
