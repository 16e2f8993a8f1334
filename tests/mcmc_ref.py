"""Numpy restatement of src/mcmc.jl (MCMCStrategy) — TEST INFRASTRUCTURE ONLY: what tests/test_mcmc_cpu.py pins to the
reference's own unit test and tests/test_gpu_mcmc.py compares the device against.

Follows mcmc.jl statement by statement (mcmc_binom_coefficients :79-90, regularization_loss :104-107, relocate_gaussians!
:132-178, add_gaussians! :184-217, multinomial_sample :220-225, split_sampled! :232-260, relocation_params :266-280,
inject_noise! / _inject_noise! :288-325) on the C-order arrays of oracle/densify.py (Gaussian index first), with the two
intended deviations of the device path (include/gsr.h):

 1. random numbers come from the project's counter-based generator (`_mix32`, `uniform01`, `randn3` of oracle/densify.py);
 2. the multinomial draw works on integer weights q = floor(sigmoid(o)·2^30), exact integer prefix sums, r = (h·total) >> 64
    with h the 64 generator bits of (seed, draw index), and selects the first row whose inclusive prefix is > r.  Python
    integers: exact.

Functions that evaluate floating-point expressions take `dtype`: np.float32 restates the reference's arithmetic, np.float64
evaluates the same expression on the same fp32 inputs in double — the yardstick tolerances are derived from."""
from __future__ import annotations

import bisect
from dataclasses import dataclass, field

import numpy as np

from oracle.densify import (PARAMS, Model, _mix32, inverse_sigmoid, new_optimizers, randn3, sigmoid, uniform01,  # noqa: F401
                            unnorm_quat2rot)

f32 = np.float32
WEIGHT_ONE = 1 << 30


def binom_coefficients(n_max: int) -> np.ndarray:
    """mcmc_binom_coefficients (mcmc.jl:79-90): binoms[n, k] = C(n, k)·(-1)^k/√(k+1); the running product in double, the rest
    in float32."""
    b = np.zeros((n_max, n_max), f32)
    for n in range(n_max):
        c = 1.0
        for k in range(n + 1):
            sign = f32(1) if k % 2 == 0 else f32(-1)
            b[n, k] = f32(c) * sign / np.sqrt(f32(k + 1), dtype=f32)
            if k < n:
                c *= (n - k) / (k + 1)
    return b


@dataclass
class Strategy:
    """MCMCStrategy (mcmc.jl:43-77)"""
    max_cap: int = 2_000_000
    min_opacity: float = 0.005
    max_scale: float = 0.1
    start_refine: int = 500
    stop_refine: int = 25_000
    refine_every: int = 100
    grow_factor: float = 1.05
    noise_lr: float = 5e5
    opacity_reg: float = 0.01
    scale_reg: float = 0.01
    n_max: int = 51
    binoms: np.ndarray = field(default=None, repr=False)

    def __post_init__(self):
        if self.binoms is None:
            self.binoms = binom_coefficients(self.n_max)


def relocation_params(strategy: Strategy, o, ratio: int, dtype=f32):
    """relocation_params (mcmc.jl:266-280) for an array (or scalar) of activated opacities `o` (float32 values) and ONE integer
    ratio, evaluated in `dtype`.  The constants are the reference's Float32 literals, the table is the Float32 table."""
    T = dtype
    lo_c, hi_c = T(f32(1e-6)), T(f32(1) - f32(1e-6))
    o = np.clip(np.asarray(o, f32).astype(T), lo_c, hi_c)
    new_o = T(1) - np.power(T(1) - o, T(1) / T(ratio), dtype=T)
    new_o = np.clip(new_o, max(lo_c, T(f32(strategy.min_opacity))), hi_c).astype(T)
    denom = np.zeros_like(o, dtype=T)
    for i in range(1, ratio + 1):
        for k in range(i):
            denom = (denom + T(strategy.binoms[i - 1, k]) * np.power(new_o, T(k + 1), dtype=T)).astype(T)
    denom = np.copysign(np.maximum(np.abs(denom), T(f32(1e-8))), denom)
    coeff = np.clip(o / denom, T(-1e6), T(1e6)).astype(T)
    return new_o, coeff


def weights(opacities, scales=None, min_opacity=0.0, log_max_scale=0.0, with_dead=False):
    """q = floor(sigmoid(o)·2^30) (int64 array; 0 on dead rows) and the dead mask of mcmc.jl:135-140 (None without)."""
    o = sigmoid(np.asarray(opacities, f32).reshape(-1))
    q = np.floor(o.astype(np.float64) * WEIGHT_ONE).astype(np.int64)
    dead = None
    if with_dead:
        s_max = np.asarray(scales, f32).max(axis=1)
        dead = (o <= f32(min_opacity)) | (s_max > f32(log_max_scale))
        q[dead] = 0
    return q, dead


def rand_bits(seed, rows, draw):
    with np.errstate(over="ignore"):
        return _mix32(_mix32(np.uint32(seed) ^ (np.asarray(rows).astype(np.uint32) * np.uint32(0x9E3779B9)))
                      + np.uint32(draw) * np.uint32(0x85EBCA6B))


def draw_positions(seed, m, total: int):
    """r_j = mulhi64(h_j, total), j < m — Python integers."""
    j = np.arange(m, dtype=np.uint32)
    hi, lo = rand_bits(seed, j, 0), rand_bits(seed, j, 1)
    return [(((int(a) << 32) | int(b)) * total) >> 64 for a, b in zip(hi, lo)]


def select_rows(q, positions):
    """first row whose inclusive prefix sum of `q` is > r, for every r of `positions` (all < sum(q))"""
    prefix, run = [], 0
    for v in np.asarray(q).tolist():
        run += int(v)
        prefix.append(run)
    return np.array([bisect.bisect_right(prefix, r) for r in positions], dtype=np.int64)


def multinomial_sample(q, m: int, seed: int):
    """(sampled (m) int64, counts (n) int32, total) — mcmc.jl:220-225 + :237-240 under deviation 2.  total == 0: no draws."""
    q = np.asarray(q)
    total = int(sum(int(v) for v in q.tolist()))
    if total == 0 or m == 0:
        return np.zeros(0, np.int64), np.zeros(q.shape[0], np.int32), total
    sampled = select_rows(q, draw_positions(seed, m, total))
    return sampled, np.bincount(sampled, minlength=q.shape[0]).astype(np.int32), total


def split_sampled(strategy: Strategy, gs: Model, counts, dtype=f32):
    """split_sampled! (mcmc.jl:232-260) in place on every row with counts > 0; `o` is the row's own activated opacity before
    the rewrite.  Returns the touched rows."""
    T = dtype
    rows = np.flatnonzero(np.asarray(counts) > 0)
    o = sigmoid(gs.opacities.reshape(-1))
    new_op = gs.opacities.astype(T)
    new_sc = gs.scales.astype(T)
    for ratio in np.unique(np.clip(np.asarray(counts)[rows] + 1, 1, strategy.n_max)):
        r = rows[np.clip(np.asarray(counts)[rows] + 1, 1, strategy.n_max) == ratio]
        new_o, coeff = relocation_params(strategy, o[r], int(ratio), T)
        new_op[r, 0] = np.log(new_o / (T(1) - new_o), dtype=T)
        s_old = np.exp(gs.scales[r].astype(T), dtype=T)
        new_sc[r] = np.log(np.maximum(np.abs(coeff[:, None] * s_old), T(f32(1e-10))), dtype=T)
    gs.opacities, gs.scales = new_op, new_sc
    return rows


def _zero_rows(opt, x, rows):
    shape = x.shape
    for key in ("mu", "nu"):
        m = opt[key].reshape(shape)
        m[rows] = 0
        opt[key] = m.reshape(-1)


def relocate_gaussians(strategy: Strategy, gs: Model, optimizers, extent, seed, ids=None, q=None, dtype=f32):
    """relocate_gaussians! (mcmc.jl:132-178).  `q`: weights to sample with instead of the restatement's own (the device's,
    so that the discrete draws are compared like for like); `ids` is relocated in place.  Returns dict(n=, dead=, sampled=,
    counts=, touched=) — n = 0 and nothing changed on the early returns."""
    none = dict(n=0, dead=np.zeros(0, np.int64), sampled=np.zeros(0, np.int64), counts=None, touched=np.zeros(0, np.int64))
    log_max_scale = np.log(f32(strategy.max_scale) * f32(extent), dtype=f32)
    q_own, is_dead = weights(gs.opacities, gs.scales, strategy.min_opacity, log_max_scale, with_dead=True)
    dead = np.flatnonzero(is_dead)
    if dead.size == 0 or dead.size == len(gs):
        return none
    sampled, counts, total = multinomial_sample(q_own if q is None else q, dead.size, seed)
    if total == 0:
        return none
    touched = split_sampled(strategy, gs, counts, dtype)
    for k in PARAMS:
        x = getattr(gs, k)
        if x.size == 0:
            continue
        x[dead] = x[sampled]
        _zero_rows(optimizers[k], x, np.union1d(sampled, dead))
    if ids is not None:
        ids[dead] = ids[sampled]
    return dict(n=dead.size, dead=dead, sampled=sampled, counts=counts, touched=touched)


def n_new_gaussians(strategy: Strategy, n: int) -> int:
    """min(max_cap, floor(Int, grow_factor * n)) - n, Julia's Float32 product (mcmc.jl:186)"""
    return min(strategy.max_cap, int(np.floor(f32(strategy.grow_factor) * f32(n)))) - n


def add_gaussians(strategy: Strategy, gs: Model, optimizers, seed, ids=None, q=None, dtype=f32):
    """add_gaussians! (mcmc.jl:184-217).  Returns dict(n=, sampled=, counts=, touched=, ids=)."""
    n = len(gs)
    n_new = n_new_gaussians(strategy, n)
    none = dict(n=0, sampled=np.zeros(0, np.int64), counts=None, touched=np.zeros(0, np.int64), ids=ids)
    if n_new <= 0:
        return none
    q_own, _ = weights(gs.opacities)
    sampled, counts, total = multinomial_sample(q_own if q is None else q, n_new, seed)
    if total == 0:
        return none
    touched = split_sampled(strategy, gs, counts, dtype)
    for k in PARAMS:
        x = getattr(gs, k)
        if x.size == 0:
            setattr(gs, k, np.zeros((n + n_new,) + x.shape[1:], x.dtype))
            continue
        z = np.zeros(x[sampled].size, f32)
        optimizers[k]["mu"] = np.concatenate([optimizers[k]["mu"], z])
        optimizers[k]["nu"] = np.concatenate([optimizers[k]["nu"], z])
        setattr(gs, k, np.concatenate([x, x[sampled]], 0))
    if ids is not None:
        ids = np.concatenate([ids, ids[sampled]])
    return dict(n=n_new, sampled=sampled, counts=counts, touched=touched, ids=ids)


def normals(seed, n, dtype=f32):
    """the three normals of every row: oracle.densify.randn3 in float32; in float64 the same Box-Muller on the same (exact)
    uniforms"""
    if dtype == f32:
        return randn3(seed, n)
    rows = np.arange(n, dtype=np.uint32)
    u1, u2, u3, u4 = (uniform01(seed, rows, d).astype(np.float64) for d in range(4))
    r1, r2 = np.sqrt(-2.0 * np.log(u1)), np.sqrt(-2.0 * np.log(u3))
    tp = np.float64(f32(6.2831853071795864))
    return np.stack([r1 * np.cos(tp * u2), r1 * np.sin(tp * u2), r2 * np.cos(tp * u4)], 1)


def noise_kick(gs: Model, lr, max_kick, seed, dtype=f32):
    """_inject_noise! (mcmc.jl:306-325): (Δ (N,3), ‖Δ‖ before the cap (N)) in `dtype`; points + Δ is the kernel's result."""
    T = dtype
    n = len(gs)
    xi = normals(seed, n, T).astype(T)
    if T == f32:
        R = unnorm_quat2rot(gs.rotations)
    else:
        q = gs.rotations.astype(T)
        q = q / np.sqrt((q * q).sum(1))[:, None]
        w, x, y, z = q.T
        R = np.empty((n, 3, 3), T)
        R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
        R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
        R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    s = np.broadcast_to(gs.scales, (n, 3)).astype(T)
    with np.errstate(over="ignore"):
        s2 = np.minimum(np.exp(T(2) * s, dtype=T), T(f32(1e8)))
        t = s2 * ((R[:, 0, :] * xi[:, 0:1] + R[:, 1, :] * xi[:, 1:2]) + R[:, 2, :] * xi[:, 2:3])          # S²·(Rᵀ·ξ)
        sx = (R[:, :, 0] * t[:, 0:1] + R[:, :, 1] * t[:, 1:2]) + R[:, :, 2] * t[:, 2:3]                    # R·(...)
        if T == f32:
            op = sigmoid(gs.opacities.reshape(-1))
        else:
            op = 1.0 / (1.0 + np.exp(-gs.opacities.reshape(-1).astype(T)))
        factor = T(f32(lr)) / (T(1) + np.exp(np.minimum(T(100) * op - T(0.5), T(80)), dtype=T))
    d = (factor[:, None] * sx).astype(T)
    l = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=T)
    capped = l > T(f32(max_kick))
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(capped, T(f32(max_kick)) / l, T(1)).astype(T)
    d = np.where(capped[:, None], d * k[:, None], d).astype(T)
    return d, l


def regularization(strategy: Strategy, opacities, scales):
    """regularization_loss (mcmc.jl:104-107) in float64 on the fp32 inputs -> (loss, ∇ w.r.t. the raw opacities (N,1), ∇ w.r.t.
    the raw scales (N,sd))."""
    o = np.asarray(opacities, np.float64)
    s = np.asarray(scales, np.float64)
    a = 1.0 / (1.0 + np.exp(-o))
    e = np.exp(s)
    oreg, sreg = float(f32(strategy.opacity_reg)), float(f32(strategy.scale_reg))
    loss = oreg * a.mean() + sreg * e.mean()
    return loss, oreg * a * (1 - a) / a.size, sreg * e / e.size
