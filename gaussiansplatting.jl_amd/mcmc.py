"""MCMCStrategy: the reference's second density-control strategy (`strategy = :mcmc`, src/strategy.jl:16, src/mcmc.jl) on
the device.  The control flow below is the reference's, function for function (post_train_step! -> relocate_gaussians! ->
add_gaussians! -> inject_noise!, mcmc.jl:109-124); every per-Gaussian pass — in the reference a chain of device->host copies,
host loops and re-uploads (:135-258) — is one library launch (gsr_mcmc_*; appending goes through gsr_compose_rows).  It works
on `densification.GaussianModel` and the dict of `optim.Adam`, `ids` included.

Two intended deviations (include/gsr.h): every random number is a pure function of (seed, index, draw) of the
project's counter-based generator, and the multinomial draw runs on integer weights floor(sigmoid(o)·2^30) with exact uint64
prefix sums.  The seeds of a run derive from (`seed`, counter) the way `DefaultStrategy.next_split_seed` does, with separate
counters for the sampling rounds and the per-step noise; both travel in checkpoints (state_dict).

A refine round reads back at most two words (the number of dead rows, the sampler's total); a plain step reads nothing.
The one exception is a degenerate model: when the relocation finds dead rows but no weight on the alive ones (NaN opacities on
every alive row, or a `min_opacity` below 2^-30) it has used both reads to find that out, and the growth that follows reads its own total, a third word — the
growth weighs the dead rows too, so the relocation's zero says nothing about it."""
from __future__ import annotations

import ctypes as C

import numpy as np

import torch

from . import _lib as L
from .densification import PARAMS, GaussianModel, _compose, _ptr, findall

f32 = np.float32


def binom_coefficients(n_max: int) -> np.ndarray:
    """mcmc_binom_coefficients (mcmc.jl:79-90): binoms[n, k] = C(n, k)·(-1)^k/√(k+1) as float32, (n_max, n_max) row-major."""
    b = np.zeros((n_max, n_max), f32)
    for n in range(n_max):
        c = 1.0
        for k in range(n + 1):
            sign = f32(1) if k % 2 == 0 else f32(-1)
            b[n, k] = f32(c) * sign / np.sqrt(f32(k + 1), dtype=f32)
            if k < n:
                c *= (n - k) / (k + 1)
    return b


class MCMCStrategy:
    """MCMCStrategy (mcmc.jl:43-77): the eleven hyper-parameters with the reference's defaults, + the seed of the run."""
    STATE_KEYS = ("seed_base", "sample_rounds", "noise_steps")   # what checkpoint.save_state / load_state carry

    def __init__(self, max_cap=2_000_000, min_opacity=0.005, max_scale=0.1, start_refine=500, stop_refine=25_000,
                 refine_every=100, grow_factor=1.05, noise_lr=5e5, opacity_reg=0.01, scale_reg=0.01, n_max=51, seed: int = 0):
        self.max_cap, self.start_refine, self.stop_refine = int(max_cap), int(start_refine), int(stop_refine)
        self.refine_every, self.n_max = int(refine_every), int(n_max)
        if self.n_max < 1:
            raise ValueError("n_max must be at least 1")
        self.min_opacity, self.max_scale, self.grow_factor = float(f32(min_opacity)), float(f32(max_scale)), float(f32(grow_factor))
        self.noise_lr, self.opacity_reg, self.scale_reg = float(f32(noise_lr)), float(f32(opacity_reg)), float(f32(scale_reg))
        self.binoms = binom_coefficients(self.n_max)   # host table, built once; its device copy follows the model's device
        self._binoms_dev = None
        self._sample_scratch = None
        self.seed_base = int(seed) & 0xFFFFFFFF
        self.sample_rounds = 0
        self.noise_steps = 0

    def binoms_on(self, device) -> torch.Tensor:
        if self._binoms_dev is None or self._binoms_dev.device != device:
            self._binoms_dev = torch.from_numpy(self.binoms).to(device)
        return self._binoms_dev

    def sample_scratch(self, words: int, device) -> torch.Tensor:
        """The sampler's scratch (int64 words), kept across refine rounds; it grows by half again when the model outgrows it."""
        t = self._sample_scratch
        if t is None or t.device != device or t.numel() < words:
            self._sample_scratch = t = torch.empty(words + words // 2, dtype=torch.int64, device=device)
        return t

    def state_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k in self.STATE_KEYS}

    def load_state_dict(self, d: dict):
        self.seed_base = int(d["seed_base"]) & 0xFFFFFFFF
        self.sample_rounds = int(d["sample_rounds"])
        self.noise_steps = int(d["noise_steps"])

    def next_sample_seed(self) -> int:
        """Seed of the next multinomial draw (one per relocation, one per growth): distinct for every draw of this object."""
        self.sample_rounds += 1
        return (self.seed_base * 0x9E3779B1 + self.sample_rounds * 0x85EBCA6B) & 0xFFFFFFFF

    def next_noise_seed(self) -> int:
        """Seed of the next step's position noise; a stream of its own (another multiplier than the sampling rounds')."""
        self.noise_steps += 1
        return (self.seed_base * 0x9E3779B1 + self.noise_steps * 0xC2B2AE35 + 0x27D4EB2F) & 0xFFFFFFFF

    def refining(self, step: int) -> bool:
        return self.start_refine < step < self.stop_refine and step % self.refine_every == 0   # mcmc.jl:114-116


def _sd(gs: GaussianModel) -> int:
    return int(gs.scales.shape[1])


def n_new_gaussians(strategy: MCMCStrategy, n: int) -> int:
    """min(max_cap, floor(Int, grow_factor * n)) - n with Julia's Float32 product (mcmc.jl:186)."""
    return min(strategy.max_cap, int(np.floor(f32(strategy.grow_factor) * f32(n)))) - n


def weights(gs: GaussianModel, min_opacity: float = 0.0, log_max_scale: float = 0.0, with_dead: bool = False):
    """gsr_mcmc_weights: (q, dead) — uint32 sampling weights (held in an int32 tensor) and, with_dead, the uint8 dead mask."""
    n, dev = len(gs), gs.points.device
    q = torch.empty(n, dtype=torch.int32, device=dev)
    dead = torch.empty(n, dtype=torch.uint8, device=dev) if with_dead else None
    L.check(L.load().gsr_mcmc_weights(n, _sd(gs), _ptr(gs.opacities), _ptr(gs.scales), float(min_opacity), float(log_max_scale),
                                      _ptr(q), _ptr(dead), L.stream()))
    return q, dead


def multinomial_sample(q: torch.Tensor, m: int, seed: int, strategy: MCMCStrategy = None):
    """multinomial_sample (mcmc.jl:220-225) + the multiplicities of split_sampled! (:237-240) on the weights `q`:
    (sampled int32 (m), counts int32 (n), total int64 (1)) — device tensors; nothing is read back.  With total == 0 `sampled`
    holds zeros and means nothing.  The library zeroes `counts` itself; with `strategy` the scan's scratch (8 B per row) is the
    buffer that object keeps from round to round, not a fresh allocation."""
    n, dev = q.numel(), q.device
    sampled = torch.zeros(m, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    if m == 0:   # the library touches nothing
        return sampled, torch.zeros(n, dtype=torch.int32, device=dev), total
    lib = L.load()
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    nb = int(lib.gsr_mcmc_sample_scratch_bytes(n))
    words = max(nb // 8, 1)
    scratch = strategy.sample_scratch(words, dev) if strategy is not None else torch.empty(words, dtype=torch.int64, device=dev)
    L.check(lib.gsr_mcmc_sample(n, _ptr(q), int(m), int(seed) & 0xFFFFFFFF, _ptr(sampled), _ptr(counts), total.data_ptr(),
                                scratch.data_ptr(), scratch.numel() * 8, L.stream()))
    return sampled, counts, total


def relocation_params(strategy: MCMCStrategy, o: torch.Tensor, ratio: torch.Tensor):
    """relocation_params (mcmc.jl:266-280) on device arrays: activated opacities `o` (float32) and `ratio` (int32) ->
    (new_o, coeff).  The device function `split_sampled` applies (gsr_mcmc_relocation_params)."""
    if not (o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and ratio.is_cuda and ratio.dtype == torch.int32
            and ratio.is_contiguous() and ratio.numel() == o.numel()):
        raise ValueError("o (float32) and ratio (int32) must be contiguous HIP device tensors of one length (no CPU path)")
    new_o, coeff = torch.empty_like(o), torch.empty_like(o)
    L.check(L.load().gsr_mcmc_relocation_params(o.numel(), _ptr(o), _ptr(ratio), _ptr(strategy.binoms_on(o.device)), strategy.n_max,
                                                strategy.min_opacity, _ptr(new_o), _ptr(coeff), L.stream()))
    return new_o, coeff


def split_sampled(strategy: MCMCStrategy, gs: GaussianModel, counts: torch.Tensor):
    """split_sampled! (mcmc.jl:232-260): Eq. 9 in place on every row with counts > 0, as if it were split into 1 + counts
    identical copies."""
    L.check(L.load().gsr_mcmc_split_sampled(len(gs), _sd(gs), _ptr(counts), _ptr(strategy.binoms_on(gs.points.device)), strategy.n_max,
                                            strategy.min_opacity, _ptr(gs.opacities), _ptr(gs.scales), L.stream()))


def _relocate_rows(gs: GaussianModel, optimizers, dead_idx: torch.Tensor, sampled: torch.Tensor):
    groups = []
    for k in PARAMS:
        x = getattr(gs, k)
        rw = int(np.prod(x.shape[1:]))
        if rw == 0:   # empty features_rest (mcmc.jl:157,168)
            continue
        opt = optimizers[k]
        groups += [L.ComposeGroup(None, x.data_ptr(), rw, 0), L.ComposeGroup(None, opt.mu.data_ptr(), rw, 1),
                   L.ComposeGroup(None, opt.nu.data_ptr(), rw, 1)]
    if gs.ids is not None:   # mcmc.jl:162
        groups.append(L.ComposeGroup(None, gs.ids.data_ptr(), 1, 0))
    arr = (L.ComposeGroup * len(groups))(*groups)
    L.check(L.load().gsr_mcmc_relocate_rows(arr, len(groups), len(gs), _ptr(dead_idx), _ptr(sampled), dead_idx.numel(), L.stream()))


def relocate_gaussians(strategy: MCMCStrategy, gs: GaussianModel, optimizers, extent: float, seed=None) -> int:
    """relocate_gaussians! (mcmc.jl:132-178): move the dead Gaussians (opacity <= min_opacity, or a scale above
    max_scale·extent) onto alive ones sampled ∝ opacity, correcting the sources by Eq. 9; the Adam moments of every touched row
    restart from zero.  Returns the number of relocated rows.  `seed`: the draw's (None: the strategy's advancing counter)."""
    n = len(gs)
    if n == 0:
        return 0
    log_max_scale = np.log(f32(strategy.max_scale) * f32(extent), dtype=f32)
    q, dead = weights(gs, strategy.min_opacity, log_max_scale, with_dead=True)
    dead_idx = findall(dead)                       # read-back 1: the number of dead rows
    m = dead_idx.numel()
    if m == 0 or m == n:                           # isempty(dead) || isempty(alive)
        return 0
    if seed is None:
        seed = strategy.next_sample_seed()
    sampled, counts, total = multinomial_sample(q, m, seed, strategy)
    if int(total.item()) == 0:                     # read-back 2: `total > 0 || return Int[]`
        return 0
    split_sampled(strategy, gs, counts)
    _relocate_rows(gs, optimizers, dead_idx, sampled)
    return m


def add_gaussians(strategy: MCMCStrategy, gs: GaussianModel, optimizers, seed=None, total_is_positive: bool = False) -> int:
    """add_gaussians! (mcmc.jl:184-217): grow the model by grow_factor (up to max_cap): sample sources ∝ opacity, split them by
    Eq. 9 and append the copies with zeroed Adam moments.  Returns the number of appended rows.  `total_is_positive`: the
    caller knows that some row has a positive weight (a relocation just ran: every row it wrote has an opacity of at least
    max(1e-6, min_opacity)) — the sampler's total is then not read back."""
    n = len(gs)
    n_new = n_new_gaussians(strategy, n)
    if n_new <= 0:
        return 0
    if seed is None:
        seed = strategy.next_sample_seed()
    q, _ = weights(gs)
    sampled, counts, total = multinomial_sample(q, n_new, seed, strategy)
    if not total_is_positive and int(total.item()) == 0:
        return 0
    split_sampled(strategy, gs, counts)
    _compose(gs, optimizers, None, n, sampled, n_new, 1)   # append_gaussians! + _append_optimizer!; repeated sources are fine
    return n_new


def inject_noise(strategy: MCMCStrategy, gs: GaussianModel, points_lr: float, extent: float, seed=None):
    """inject_noise! (mcmc.jl:288-325): perturb the positions with noise ∝ Σ·ξ, gated to near-dead Gaussians and capped at half
    the relocation size threshold.  Runs on EVERY step."""
    n = len(gs)
    if n == 0:
        return
    if seed is None:
        seed = strategy.next_noise_seed()
    max_kick = f32(0.5) * f32(strategy.max_scale) * f32(extent)
    lr = f32(points_lr) * f32(strategy.noise_lr)
    L.check(L.load().gsr_mcmc_inject_noise(n, _sd(gs), _ptr(gs.points), _ptr(gs.opacities), _ptr(gs.scales), _ptr(gs.rotations),
                                           float(lr), float(max_kick), int(seed) & 0xFFFFFFFF, L.stream()))


def regularization_loss(strategy: MCMCStrategy, opacities: torch.Tensor, scales: torch.Tensor, vopacities: torch.Tensor = None,
                        vscales: torch.Tensor = None, scratch: torch.Tensor = None) -> torch.Tensor:
    """regularization_loss (mcmc.jl:104-107) over the RAW opacities (N,1) and scales (N,3) / (N,1): opacity_reg ·
    mean(sigmoid(o)) + scale_reg · mean(exp(s)) as a device scalar.  With `vopacities` (N,1) / `vscales` (N,3) — the gradients
    `rast.backward_raw` wrote, w.r.t. the ACTIVATED values — the regulariser's gradient is added onto them; the step then runs
    `optim.trainer_tail_step` (the fused tail never materialises these arrays)."""
    for t, nm in ((opacities, "opacities"), (scales, "scales"), (vopacities, "vopacities"), (vscales, "vscales")):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{nm} must be a contiguous float32 HIP device tensor (no CPU path)")
    n = int(opacities.shape[0])
    if opacities.numel() != n or scales.dim() != 2 or scales.shape[0] != n or scales.shape[1] not in (1, 3):
        raise ValueError("opacities must be (N,1) and scales (N,3) or (N,1)")
    if vopacities is not None and vopacities.numel() != n:
        raise ValueError("vopacities must hold N elements")
    if vscales is not None and tuple(vscales.shape) != (n, 3):
        raise ValueError("vscales must be (N,3): the gradient w.r.t. the activated scales")
    lib = L.load()
    nb = int(lib.gsr_mcmc_regularization_scratch_bytes(n))
    if scratch is None:
        scratch = torch.empty(max(nb, 4), dtype=torch.uint8, device=opacities.device)
    loss = torch.empty((), dtype=torch.float32, device=opacities.device)
    L.check(lib.gsr_mcmc_regularization(n, int(scales.shape[1]), _ptr(opacities), _ptr(scales), strategy.opacity_reg,
                                        strategy.scale_reg, loss.data_ptr(), _ptr(vopacities), _ptr(vscales), scratch.data_ptr(),
                                        scratch.numel(), L.stream()))
    return loss


def post_train_step(strategy: MCMCStrategy, gs: GaussianModel, optimizers, rast, step: int, extent: float) -> bool:
    """post_train_step! (mcmc.jl:109-124), called once per train step after the optimizer update.  Returns whether this was a
    refine step (the raw opacities / scales were rewritten and the model may have grown: activated copies are stale)."""
    refining = strategy.refining(step)
    if refining:
        n_before = max(len(gs), 1)
        relocated = relocate_gaussians(strategy, gs, optimizers, extent)
        add_gaussians(strategy, gs, optimizers, total_is_positive=relocated > 0)
        # the model changed size: re-size the rasterizer's scratch here, as densification.post_train_step does — the reference
        # empties its allocation cache at this very place (mcmc.jl:118)
        if rast is not None and hasattr(rast, "reserve"):
            grow = len(gs) / n_before
            rast.reserve(int(1.5 * len(gs)), int(1.5 * max(grow, 1.0) * int(rast.stats.n_rendered)))
    inject_noise(strategy, gs, optimizers["points"].lr, extent)
    return refining
