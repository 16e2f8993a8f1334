"""-m gpu tests of the device MCMC strategy (gsr_mcmc_* through the host mirror mcmc.py) against the numpy restatement
tests/mcmc_ref.py: dead masks, draws, multiplicities, row copies, Adam moments and ids EXACT (the restatement samples with
the device's own integer weights, so the discrete choices are compared like for like); values that went through device
transcendentals within bounds derived from the fp32 restatement's own distance to its float64 evaluation (what a split
rewrote: within the Eq. 9 bound itself, the float64 evaluation starting from the device's own activated inputs).  Wherever an
input could sit on a decision threshold the test asserts, on the CPU, that it does not."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

import mcmc_ref as mr
from hip_helpers import dev, rel_l2
from oracle import densify as dz
from test_oracle_densify import make_model

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import train_harness as TH  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
TRANSC = 2e-6            # device vs glibc transcendentals: the bound tests/test_gpu_densify.py uses
EXTENT = 5.0
LOGIT_MIN = math.log(0.005 / 0.995)


def host(t):
    return t.detach().cpu().numpy()


def q_host(q):
    """device weights (uint32 bits in an int32 tensor) -> int64"""
    return host(q).view(np.uint32).astype(np.int64)


def to_device(pkg, m: dz.Model, ids=None):
    gs = pkg.densification.GaussianModel(*[dev(getattr(m, k)) for k in dz.PARAMS])
    if ids is not None:
        gs.ids = dev(ids, torch.int32)
    return gs


def random_optimizers(gs_o, seed):
    opt = dz.new_optimizers(gs_o)
    rng = np.random.default_rng(seed)
    for k in dz.PARAMS:
        opt[k]["mu"][:] = rng.normal(size=opt[k]["mu"].shape)
        opt[k]["nu"][:] = rng.uniform(0.1, 1.0, size=opt[k]["nu"].shape)
    return opt


def device_optimizers(pkg, gs_d, opt_o):
    out = {}
    for k in dz.PARAMS:
        a = pkg.optim.Adam(getattr(gs_d, k), 1e-3, eps=1e-15)
        a.mu, a.nu = dev(opt_o[k]["mu"]), dev(opt_o[k]["nu"])
        out[k] = a
    return out


def off_the_opacity_threshold(op):
    """raw opacities at least 1e-3 from logit(min_opacity): the dead decision then does not hang on the last bits of a
    sigmoid (1e-3 in the logit = 5e-6 in the opacity = 1e-3 relative, 500 x the transcendental bound)"""
    op = op.copy()
    near = np.abs(op - f32(LOGIT_MIN)) < 2e-3
    op[near] += f32(8e-3)
    assert (np.abs(op.astype(np.float64) - LOGIT_MIN) >= 1e-3).all()
    return op


def model(n, k_rest, seed, sd, op_mean=-1.0, op_std=2.0):
    m = make_model(n, k_rest, seed, sd)
    rng = np.random.default_rng(seed + 1000)
    m.opacities = off_the_opacity_threshold(rng.normal(op_mean, op_std, size=(n, 1)).astype(f32))
    return m


def device_activations(pkg, gs):
    """The device's own sigmoid(opacity) (n) and exp(scale) (n, sd) of a model, to be taken BEFORE a split rewrites them: the
    activated copies the forward prologue writes, which are the calls mcmc.hip makes (1/(1 + expf(-x)), expf(x)).  The weights
    tie the two: q == floor(o·2^30) on every row."""
    n, sd = len(gs), gs.scales.shape[1]
    _, oa, sa = pkg.rasterizer.prologue_forward(torch.zeros((n, 1, 3), device="cuda"), None, gs.opacities, gs.scales)
    torch.cuda.synchronize()
    o, e = host(oa).reshape(-1), host(sa)[:, :sd]
    assert np.array_equal(q_host(pkg.mcmc.weights(gs)[0]), np.floor(o.astype(np.float64) * 2 ** 30).astype(np.int64))
    return o, e


def assert_split_values(what, st_o, o_act, e_act, counts, op_dev, sc_dev):
    """Raw opacities / scales a split rewrote, held to the bound of the Eq. 9 test (eq9_grid) and to nothing wider.  The
    float64 evaluation of the restatement gets the device's own activated inputs (`o_act`, `e_act`: device_activations before
    the split), so that Eq. 9 is all that is compared; the device's results are read in the activated domain, where Eq. 9's
    values live: new_o = sigmoid(raw opacity), |coeff|·exp(s_old) = exp(raw scale).  Returns the two measured deviations."""
    bound = eq9_grid()[4]
    counts = np.asarray(counts)
    rows = np.flatnonzero(counts > 0)
    ratio = np.clip(counts[rows] + 1, 1, st_o.n_max)
    new_o, coeff = np.empty(rows.size), np.empty(rows.size)
    for r in np.unique(ratio):
        sel = ratio == r
        new_o[sel], coeff[sel] = mr.relocation_params(st_o, o_act[rows][sel], int(r), np.float64)
    want_s = np.maximum(np.abs(coeff[:, None] * e_act[rows].astype(np.float64)), float(f32(1e-10)))
    got_o = 1.0 / (1.0 + np.exp(-op_dev.reshape(-1)[rows].astype(np.float64)))
    got_s = np.exp(sc_dev[rows].astype(np.float64))
    e_o, e_s = np.abs(got_o / new_o - 1).max(), np.abs(got_s / want_s - 1).max()
    print(f"\n{what}: {rows.size} rows Eq. 9 rewrote (ratios {ratio.min()}..{ratio.max()}, o {o_act[rows].min():.2e}..{o_act[rows].max():.6f}) vs "
          f"float64: new_o {e_o:.3e}, coeff·exp(s) {e_s:.3e}; bound {bound:.3e}")
    assert e_o <= bound and e_s <= bound
    return e_o, e_s


def log_max_scale(strategy):
    return np.log(f32(strategy.max_scale) * f32(EXTENT), dtype=f32)


@functools.lru_cache(maxsize=None)
def eq9_grid():
    """(o (G), ratios, float64 new_o / coeff (R,G), bound): the bound of every Eq. 9 comparison = max(2e-6, 4 x the fp32
    restatement's own worst relative deviation from its float64 evaluation on this grid) — from the restatement, never from
    the device; the factor 4: the alternating binomial sum amplifies the 1-2 ulp between the device's powf and glibc's."""
    s = mr.Strategy()
    o = np.array([1e-4, 1e-3, 0.004, 0.005, 0.006, 0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99, 0.999], f32)
    ratios = np.arange(1, s.n_max + 1)
    r64 = [mr.relocation_params(s, o, int(r), np.float64) for r in ratios]
    r32 = [mr.relocation_params(s, o, int(r), f32) for r in ratios]
    no64, c64 = np.stack([a for a, _ in r64]), np.stack([b for _, b in r64])
    no32, c32 = np.stack([a for a, _ in r32]).astype(np.float64), np.stack([b for _, b in r32]).astype(np.float64)
    worst = max(np.abs(no32 / no64 - 1).max(), np.abs(c32 / c64 - 1).max())
    return o, ratios, no64, c64, max(TRANSC, 4.0 * float(worst))


# ---------------------------------------------------------------------------------------------------------------------
# 1. weights and dead mask
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sd", [1, 3])
def test_weights_and_dead_mask(pkg, sd):
    M = pkg.mcmc
    n = 2 * 1024 + 37                      # two scan-block boundaries and a ragged tail
    m = model(n, 0, 51 + sd, sd, op_mean=-3.5, op_std=2.5)
    st = mr.Strategy()
    lms = log_max_scale(st)
    q_ref, dead_ref = mr.weights(m.opacities, m.scales, st.min_opacity, lms, with_dead=True)
    by_opacity = mr.sigmoid(m.opacities.reshape(-1)) <= f32(st.min_opacity)
    by_scale = m.scales.max(1) > lms
    assert by_opacity.sum() > 100 and (by_scale & ~by_opacity).sum() > 5 and (~dead_ref).sum() > 500   # every class is present
    gs = to_device(pkg, m)
    q, dead = M.weights(gs, st.min_opacity, lms, with_dead=True)
    torch.cuda.synchronize()
    assert np.array_equal(host(dead).astype(bool), dead_ref)
    qd = q_host(q)
    assert not qd[dead_ref].any()
    err = np.abs(qd - q_ref).max()
    print(f"\nweights sd={sd}: max |q_dev - q_ref| = {err} of 2^30 ({err / 2 ** 30:.2e})")
    assert err <= 2 ** 30 * TRANSC
    # dead = NULL: every row is weighted (add_gaussians!)
    q_all, none = M.weights(gs)
    q_all_ref, _ = mr.weights(m.opacities)
    assert none is None and np.abs(q_host(q_all) - q_all_ref).max() <= 2 ** 30 * TRANSC
    assert np.array_equal(q_host(q_all)[~dead_ref], qd[~dead_ref])


# ---------------------------------------------------------------------------------------------------------------------
# 2. sampling is exact
# ---------------------------------------------------------------------------------------------------------------------
def sample_and_compare(pkg, q, m, seed):
    sampled, counts, total = pkg.mcmc.multinomial_sample(q, m, seed)
    torch.cuda.synchronize()
    s_ref, c_ref, t_ref = mr.multinomial_sample(q_host(q), m, seed)
    assert int(total.item()) == t_ref and t_ref > 0
    assert np.array_equal(host(sampled).astype(np.int64), s_ref)
    assert np.array_equal(host(counts), c_ref) and c_ref.sum() == m
    return s_ref, c_ref


def test_sampling_shape_a_dead_blocks(pkg):
    """dead rows at both ends and one whole 1024-row scan block without weight"""
    n, m = 2 * 1024 + 37, 700
    mod = model(n, 0, 61, 3)
    mod.scales[:] = f32(-3.0)
    dead_rows = np.r_[0, n - 1, 1024:2048, np.arange(5, 900, 7)]
    mod.opacities[dead_rows] = f32(-10.0)
    st = mr.Strategy()
    gs = to_device(pkg, mod)
    q, dead = pkg.mcmc.weights(gs, st.min_opacity, log_max_scale(st), with_dead=True)
    is_dead = host(dead).astype(bool)
    assert is_dead[dead_rows].all() and is_dead[0] and is_dead[-1] and is_dead[1024:2048].all() and (~is_dead).sum() > 500
    s_ref, _ = sample_and_compare(pkg, q, m, 12345)
    assert not is_dead[s_ref].any() and s_ref.min() > 0 and (s_ref > 2047).any() and (s_ref < 1024).any()


def test_sampling_shape_b_block_sums_beyond_one_workgroup(pkg):
    """1025 scan blocks: the scan of the block sums loops past its 1024 threads.  The first 1024·1024 rows are faint (o ≈ 3e-5,
    about 30 in all) and the 5 rows of block 1024 weigh 4.8, a seventh of the total: draws land on both sides, and the ones in
    block 1024 are right only if the second turn of that loop carried the first turn's sum."""
    n, m = 1024 * 1024 + 5, 64
    rng = np.random.default_rng(62)
    op_h = rng.normal(-11.0, 1.0, size=(n, 1)).astype(f32)
    op_h[1024 * 1024:] = f32(3.0)
    op = dev(op_h)
    gs = pkg.densification.GaussianModel(torch.zeros((n, 3), device="cuda"), torch.zeros((n, 1, 3), device="cuda"),
                                         torch.zeros((n, 0, 3), device="cuda"), torch.zeros((n, 1), device="cuda"),
                                         torch.zeros((n, 4), device="cuda"), op)
    q, _ = pkg.mcmc.weights(gs)
    s_ref, _ = sample_and_compare(pkg, q, m, 777)
    assert (s_ref >= 1024 * 1024).sum() >= 3 and (s_ref < 1024 * 1024).sum() >= 32


def test_sampling_shape_c_one_heavy_row_reaches_the_ratio_clamp(pkg):
    n, m, heavy = 500, 300, 123
    mod = model(n, 0, 63, 3)
    mod.opacities[:] = f32(-16.0)
    mod.opacities[heavy] = f32(3.0)
    gs = to_device(pkg, mod)
    M = pkg.mcmc
    q, _ = M.weights(gs)
    qh = q_host(q)
    assert qh[heavy] >= 0.99 * qh.sum() and (qh > 0).all()
    s_ref, c_ref = sample_and_compare(pkg, q, m, 99)
    st_o, st_d = mr.Strategy(), M.MCMCStrategy()
    assert c_ref[heavy] > st_o.n_max                                          # ratio = clamp(counts + 1, 1, n_max) clamps
    # ... and the split under the clamp: against the float64 evaluation of the restatement
    o_act, e_act = device_activations(pkg, gs)
    M.split_sampled(st_d, gs, dev(c_ref, torch.int32))
    torch.cuda.synchronize()
    assert_split_values("split under the ratio clamp", st_o, o_act, e_act, c_ref, host(gs.opacities), host(gs.scales))
    untouched = c_ref == 0
    assert np.array_equal(host(gs.opacities)[untouched], mod.opacities[untouched])
    assert np.array_equal(host(gs.scales)[untouched], mod.scales[untouched])


def test_sampling_total_zero_and_no_draws(pkg):
    lib, L = pkg._lib.load(), pkg._lib
    n = 1500
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = int(lib.gsr_mcmc_sample_scratch_bytes(n))
    scratch = torch.empty(nb // 8, dtype=torch.int64, device="cuda")

    def run(q, m):
        sampled = torch.full((max(m, 4),), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        total = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        L.check(lib.gsr_mcmc_sample(n, q.data_ptr(), m, 5, sampled.data_ptr(), counts.data_ptr(), total.data_ptr(),
                                    scratch.data_ptr(), nb, stream))
        torch.cuda.synchronize()
        return host(sampled), host(counts), int(total.item())

    zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    s, c, t = run(zero, 40)
    assert t == 0 and not c.any() and (s == -7).all()          # total = 0 is reported; no draw is written
    some = torch.ones(n, dtype=torch.int32, device="cuda")
    s, c, t = run(some, 0)
    assert t == -7 and (c == -7).all() and (s == -7).all()     # m = 0: nothing is touched
    # sigmoid(-40)·2^30 < 1: the weights kernel itself yields the all-zero case
    gs = to_device(pkg, model(n, 0, 64, 3))
    gs.opacities.fill_(-40.0)
    assert not q_host(pkg.mcmc.weights(gs)[0]).any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. Eq. 9 on the device
# ---------------------------------------------------------------------------------------------------------------------
def device_eq9(pkg, strategy, o, ratio):
    o, ratio = np.broadcast_arrays(np.asarray(o, f32), np.asarray(ratio, np.int32))
    a, c = pkg.mcmc.relocation_params(strategy, dev(o.reshape(-1)), dev(ratio.reshape(-1), torch.int32))
    torch.cuda.synchronize()
    return host(a).reshape(o.shape), host(c).reshape(o.shape)


def test_eq9_reference_properties_on_the_device(pkg):
    """the reference's "MCMC relocation (Eq. 9)" test set (test/runtests.jl:454-484) through gsr_mcmc_relocation_params"""
    st = pkg.mcmc.MCMCStrategy()
    new_o, coeff = device_eq9(pkg, st, [0.9], [1])
    assert abs(float(new_o[0]) - float(f32(0.9))) <= 1e-6 and abs(float(coeff[0]) - 1.0) <= 1e-5
    new_o, coeff = device_eq9(pkg, st, [0.9], [2])
    assert abs(float(new_o[0]) - (1.0 - math.sqrt(1.0 - float(f32(0.9))))) <= 1e-5 and 0.0 < coeff[0] < 1.0
    ratios = np.arange(1, st.n_max + 1)
    new_o, coeff = device_eq9(pkg, st, np.full(ratios.shape, 0.99, f32), ratios)
    assert (new_o >= f32(st.min_opacity)).all() and (new_o < 1).all() and (np.diff(new_o) <= 0).all()
    assert (coeff > 0).all() and (np.diff(coeff) <= 0).all() and coeff[0] <= 1.0 + 1e-5
    new_o, coeff = device_eq9(pkg, st, [0.004], [2])
    assert new_o[0] == f32(st.min_opacity) and np.isfinite(coeff[0]) and coeff[0] > 0
    # ratios outside [1, n_max] are clamped, not read past the table
    a, c = device_eq9(pkg, st, [0.5, 0.5, 0.5, 0.5], [0, 1, st.n_max, st.n_max + 40])
    assert a[0] == a[1] and c[0] == c[1] and a[2] == a[3] and c[2] == c[3]


def test_eq9_against_the_float64_evaluation(pkg):
    o, ratios, no64, c64, bound = eq9_grid()
    st = pkg.mcmc.MCMCStrategy()
    new_o, coeff = device_eq9(pkg, st, o[None, :], ratios[:, None])
    e_o, e_c = np.abs(new_o / no64 - 1).max(), np.abs(coeff / c64 - 1).max()
    print(f"\nEq. 9 on the device vs float64 over {o.size} opacities x {ratios.size} ratios: new_o {e_o:.3e}, coeff {e_c:.3e}; "
          f"bound {bound:.3e} (fp32 restatement's own worst deviation {bound / 4:.3e})")
    assert e_o <= bound and e_c <= bound


# ---------------------------------------------------------------------------------------------------------------------
# 4. one relocation round
# ---------------------------------------------------------------------------------------------------------------------
def assert_rows_equal(gs_d, before, rows, what):
    for k in dz.PARAMS:
        assert np.array_equal(host(getattr(gs_d, k))[rows], before[k][rows]), (what, k)


@pytest.mark.parametrize("sd,k_rest", [(3, 15), (1, 0)])
def test_relocate_round_matches_the_restatement(pkg, sd, k_rest):
    M = pkg.mcmc
    n, seed = 3000, 4711
    gs_o = model(n, k_rest, 71 + sd, sd)
    ids0 = (np.arange(n, dtype=np.int32) * 3 + 1)
    opt_o = random_optimizers(gs_o, 72)
    st_o, st_d = mr.Strategy(), M.MCMCStrategy(seed=3)
    gs_d = to_device(pkg, gs_o, ids0)
    opt_d = device_optimizers(pkg, gs_d, opt_o)
    before = {k: getattr(gs_o, k).copy() for k in dz.PARAMS}
    mom_before = {k: (opt_o[k]["mu"].copy(), opt_o[k]["nu"].copy()) for k in dz.PARAMS}
    q, dead_d = M.weights(gs_d, st_o.min_opacity, log_max_scale(st_o), with_dead=True)   # the launch relocate_gaussians makes
    qh = q_host(q)
    o_act, e_act = device_activations(pkg, gs_d)
    # the restatement (rows, moments, ids) on the device's weights
    g32, ids32 = gs_o.copy(), ids0.copy()
    r = mr.relocate_gaussians(st_o, g32, opt_o, EXTENT, seed, ids=ids32, q=qh)
    dead, sampled, counts, touched = r["dead"], r["sampled"], r["counts"], r["touched"]
    assert r["n"] == dead.size > 40 and counts.max() >= 2 and np.intersect1d(dead, sampled).size == 0
    assert np.array_equal(host(dead_d).astype(bool), np.isin(np.arange(n), dead))

    n_rel = M.relocate_gaussians(st_d, gs_d, opt_d, EXTENT, seed=seed)
    torch.cuda.synchronize()
    assert n_rel == r["n"] and len(gs_d) == n and st_d.sample_rounds == 0   # an explicit seed does not advance the counter
    changed = np.zeros(n, bool); changed[touched] = True; changed[dead] = True
    assert_rows_equal(gs_d, before, ~changed, "rows Eq. 9 and the relocation did not touch")
    for k in dz.PARAMS:
        a = host(getattr(gs_d, k))
        assert a.shape == getattr(g32, k).shape, k
        if a.size == 0:
            continue
        assert np.array_equal(a[dead], a[sampled]), k                        # the dead slots hold their (post-split) sources
        if k not in ("opacities", "scales"):
            assert np.array_equal(a, getattr(g32, k)), k
        # moments: exactly zero on dead ∪ sampled, bit-equal everywhere else
        shape = a.shape
        zero = np.zeros(n, bool); zero[dead] = True; zero[sampled] = True
        for got, ref0, ref in ((host(opt_d[k].mu), mom_before[k][0], opt_o[k]["mu"]), (host(opt_d[k].nu), mom_before[k][1], opt_o[k]["nu"])):
            got = got.reshape(shape)
            assert not got[zero].any(), k
            assert np.array_equal(got[~zero], ref0.reshape(shape)[~zero]) and np.array_equal(got, ref.reshape(shape)), k
    assert np.array_equal(touched, np.flatnonzero(counts > 0))
    assert_split_values(f"relocation round sd={sd}", st_o, o_act, e_act, counts, host(gs_d.opacities), host(gs_d.scales))
    ids_d = host(gs_d.ids)
    assert np.array_equal(ids_d[dead], ids_d[sampled]) and np.array_equal(ids_d, ids32) and ids_d.dtype == np.int32
    # a source drawn twice: the source and both destinations hold identical bits
    src = int(np.flatnonzero(counts >= 2)[0])
    dst = dead[sampled == src]
    assert dst.size >= 2
    for k in dz.PARAMS:
        a = host(getattr(gs_d, k))
        if a.size:
            assert all(np.array_equal(a[d], a[src]) for d in dst), k


@pytest.mark.parametrize("case", ["no_dead", "no_alive"])
def test_relocate_early_returns_leave_the_model_untouched(pkg, case):
    M = pkg.mcmc
    n = 700
    gs_o = make_model(n, 3, 81, 3)
    gs_o.scales[:] = f32(-4.0)
    gs_o.opacities[:] = f32(0.5) if case == "no_dead" else f32(-10.0)
    opt_o = random_optimizers(gs_o, 82)
    ids0 = np.arange(n, dtype=np.int32)
    gs_d = to_device(pkg, gs_o, ids0)
    opt_d = device_optimizers(pkg, gs_d, opt_o)
    st = M.MCMCStrategy(seed=1)
    assert M.relocate_gaussians(st, gs_d, opt_d, EXTENT) == 0
    torch.cuda.synchronize()
    assert st.sample_rounds == 0                                             # nothing was drawn
    for k in dz.PARAMS:
        assert np.array_equal(host(getattr(gs_d, k)), getattr(gs_o, k)), k
        assert np.array_equal(host(opt_d[k].mu), opt_o[k]["mu"]) and np.array_equal(host(opt_d[k].nu), opt_o[k]["nu"]), k
    assert np.array_equal(host(gs_d.ids), ids0)
    assert mr.relocate_gaussians(mr.Strategy(), gs_o, opt_o, EXTENT, 1)["n"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. add_gaussians
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sd,k_rest", [(3, 3), (1, 0)])
def test_add_gaussians_matches_the_restatement(pkg, sd, k_rest):
    M = pkg.mcmc
    n, seed = 500, 31337
    kw = dict(grow_factor=1.25, max_cap=900)
    gs_o = model(n, k_rest, 91 + sd, sd)
    ids0 = np.arange(n, dtype=np.int32) + 10
    opt_o = random_optimizers(gs_o, 92)
    st_o, st_d = mr.Strategy(**kw), M.MCMCStrategy(seed=5, **kw)
    gs_d = to_device(pkg, gs_o, ids0)
    opt_d = device_optimizers(pkg, gs_d, opt_o)
    before = {k: getattr(gs_o, k).copy() for k in dz.PARAMS}
    mom_before = {k: (opt_o[k]["mu"].copy(), opt_o[k]["nu"].copy()) for k in dz.PARAMS}
    qh = q_host(M.weights(gs_d)[0])
    o_act, e_act = device_activations(pkg, gs_d)
    g32 = gs_o.copy()
    r = mr.add_gaussians(st_o, g32, opt_o, seed, ids=ids0.copy(), q=qh)
    sampled, touched = r["sampled"], r["touched"]
    assert r["n"] == 125 == sampled.size and np.unique(sampled).size < sampled.size   # some source is drawn twice

    n_new = M.add_gaussians(st_d, gs_d, opt_d, seed=seed)
    torch.cuda.synchronize()
    assert n_new == 125 and len(gs_d) == 625 == len(g32)
    untouched = np.ones(n, bool); untouched[touched] = False
    for k in dz.PARAMS:
        a = host(getattr(gs_d, k))
        assert a.shape == getattr(g32, k).shape, k
        if a.size == 0:
            continue
        assert np.array_equal(a[n:], a[sampled]), k                          # appended rows = their post-split sources, bit for bit
        assert np.array_equal(a[:n][untouched], before[k][untouched]), k
        if k not in ("opacities", "scales"):
            assert np.array_equal(a, getattr(g32, k)), k
        rw = a[0].size
        for got, ref0 in ((host(opt_d[k].mu), mom_before[k][0]), (host(opt_d[k].nu), mom_before[k][1])):
            assert got.shape == (625 * rw,) and not got[n * rw:].any(), k        # new moments are zero ...
            assert np.array_equal(got[:n * rw], ref0), k                         # ... old ones unchanged (sources included)
    assert np.array_equal(touched, np.flatnonzero(r["counts"] > 0))
    assert_split_values(f"growth sd={sd}", st_o, o_act, e_act, r["counts"], host(gs_d.opacities)[:n], host(gs_d.scales)[:n])
    assert np.array_equal(host(gs_d.ids), r["ids"])
    # the schedule: 500 -> 625 -> 781 -> 900 -> 900, and at max_cap nothing changes
    sizes = []
    for _ in range(3):
        M.add_gaussians(st_d, gs_d, opt_d)
        sizes.append(len(gs_d))
    assert sizes == [781, 900, 900] and st_d.sample_rounds == 2               # the call at the cap draws nothing
    snap = {k: getattr(gs_d, k).clone() for k in dz.PARAMS}
    mu_snap = {k: opt_d[k].mu.clone() for k in dz.PARAMS}
    assert M.add_gaussians(st_d, gs_d, opt_d) == 0
    torch.cuda.synchronize()
    for k in dz.PARAMS:
        assert torch.equal(getattr(gs_d, k), snap[k]) and torch.equal(opt_d[k].mu, mu_snap[k]), k
    assert gs_d.ids.numel() == 900


# ---------------------------------------------------------------------------------------------------------------------
# 6. position noise
# ---------------------------------------------------------------------------------------------------------------------
NOISE_N = 2 * 256 + 19
POINTS_LR = 1.6e-4


def noise_model(sd, seed):
    """three populations: gate fully open (o ≈ 0.002, small scales), gate closed (o ≈ 0.5), and scales large enough that
    the max_kick cap applies (gate open)"""
    n = NOISE_N
    m = make_model(n, 0, seed, sd)
    rng = np.random.default_rng(seed + 1)
    pop = np.arange(n) % 3
    m.opacities[:, 0] = np.where(pop == 1, rng.normal(0.0, 0.05, n), rng.normal(math.log(0.002 / 0.998), 0.05, n)).astype(f32)
    m.scales[:] = np.where((pop == 2)[:, None], rng.normal(-0.8, 0.25, (n, sd)), rng.normal(-4.5, 0.3, (n, sd))).astype(f32)
    m.points[:] = 0
    return m, pop


def noise_bound(m, st, seed):
    lr = f32(POINTS_LR) * f32(st.noise_lr)
    max_kick = f32(0.5) * f32(st.max_scale) * f32(EXTENT)
    d64, l64 = mr.noise_kick(m, lr, max_kick, seed, np.float64)
    d32, _ = mr.noise_kick(m, lr, max_kick, seed, f32)
    norm = np.linalg.norm(d64, axis=1)
    assert (norm > 1e-30).all()
    own = (np.linalg.norm(d32.astype(np.float64) - d64, axis=1) / norm).max()
    # asserted on the CPU: no row within 1e-3 (relative) of the cap — the cap decision cannot flip
    assert (np.abs(l64 / float(max_kick) - 1.0) > 1e-3).all()
    return d64, l64, norm, float(max_kick), max(TRANSC, 4.0 * float(own)), float(own)


@pytest.mark.parametrize("sd", [1, 3])
def test_noise_kick_matches_the_float64_restatement(pkg, sd):
    M = pkg.mcmc
    st_o, st_d = mr.Strategy(), M.MCMCStrategy(seed=8)
    m, pop = noise_model(sd, 100 + sd)
    seed = 2024
    d64, l64, norm, max_kick, bound, own = noise_bound(m, st_o, seed)
    capped = l64 > max_kick
    assert capped[pop == 2].mean() > 0.9 and not capped[pop != 2].any() and (pop == 0).sum() > 100
    assert norm[pop == 1].max() < 1e-15 < norm[pop == 0].min()                  # the gate: closed vs open
    gs = to_device(pkg, m)
    M.inject_noise(st_d, gs, POINTS_LR, EXTENT, seed=seed)
    torch.cuda.synchronize()
    kick = host(gs.points).astype(np.float64)                                  # points were 0: the output IS the kick
    err = np.linalg.norm(kick - d64, axis=1) / norm
    print(f"\nnoise sd={sd}: worst per-row |Δ_dev - Δ_f64| / |Δ_f64| = {err.max():.3e} (open {err[pop == 0].max():.3e}, closed "
          f"{err[pop == 1].max():.3e}, capped {err[pop == 2].max():.3e}); bound {bound:.3e} (fp32 restatement's own {own:.3e})")
    assert err.max() <= bound
    assert (np.abs(np.linalg.norm(kick[capped], axis=1) / max_kick - 1.0) <= TRANSC).all()
    assert st_d.noise_steps == 0
    # non-zero points: points_after == fp32(points_before + Δ) with Δ the device's own kick, bit for bit
    rng = np.random.default_rng(7)
    p0 = rng.normal(size=(NOISE_N, 3)).astype(f32)
    gs2 = to_device(pkg, m)
    gs2.points.copy_(dev(p0))
    M.inject_noise(st_d, gs2, POINTS_LR, EXTENT, seed=seed)
    torch.cuda.synchronize()
    assert np.array_equal(host(gs2.points), (p0 + host(gs.points)).astype(f32))
    for k in ("scales", "rotations", "opacities"):
        assert np.array_equal(host(getattr(gs2, k)), getattr(m, k)), k
    # the same seed twice: identical bits; another seed: another kick; the strategy's own seeds advance
    gs3 = to_device(pkg, m)
    M.inject_noise(st_d, gs3, POINTS_LR, EXTENT, seed=seed)
    gs4 = to_device(pkg, m)
    M.inject_noise(st_d, gs4, POINTS_LR, EXTENT, seed=seed + 1)
    gs5, gs6 = to_device(pkg, m), to_device(pkg, m)
    M.inject_noise(st_d, gs5, POINTS_LR, EXTENT)
    M.inject_noise(st_d, gs6, POINTS_LR, EXTENT)
    torch.cuda.synchronize()
    assert torch.equal(gs3.points, gs.points) and not torch.equal(gs4.points, gs.points)
    assert st_d.noise_steps == 2 and not torch.equal(gs5.points, gs6.points)


def test_noise_stays_finite_and_handles_empty_models(pkg):
    M = pkg.mcmc
    st = M.MCMCStrategy()
    n = 300
    m = make_model(n, 0, 111, 3)
    m.scales[:] = f32(100.0)                                                   # exp(2·100) overflows: the variance cap
    m.opacities[:150] = f32(math.log(0.002 / 0.998))                           # gate open: the kick is capped
    m.opacities[150:] = f32(20.0)                                              # o -> 1: the exponent cap
    m.points[:] = 0
    gs = to_device(pkg, m)
    M.inject_noise(st, gs, POINTS_LR, EXTENT, seed=1)
    torch.cuda.synchronize()
    p = host(gs.points)
    max_kick = float(f32(0.5) * f32(st.max_scale) * f32(EXTENT))
    assert np.isfinite(p).all()
    assert (np.abs(np.linalg.norm(p[:150].astype(np.float64), axis=1) / max_kick - 1.0) <= TRANSC).all()
    assert np.linalg.norm(p[150:], axis=1).max() < 1e-20
    empty = pkg.densification.GaussianModel(*[torch.zeros((0,) + getattr(m, k).shape[1:], device="cuda") for k in dz.PARAMS])
    M.inject_noise(st, empty, POINTS_LR, EXTENT, seed=1)                        # n = 0 is a no-op
    assert st.noise_steps == 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. regulariser
# ---------------------------------------------------------------------------------------------------------------------
# (200_003, 3): 3n / 2048 = 293 partials, more than the 256 threads of the final pass, so its strided loop adds a second term
@pytest.mark.parametrize("n,sd", [(2 * 2048 // 3 + 701, 3), (1500, 1), (5, 3), (200_003, 3)])
def test_regularization_loss_and_gradients(pkg, n, sd):
    M, R = pkg.mcmc, pkg.rasterizer
    st_o, st_d = mr.Strategy(opacity_reg=0.01, scale_reg=0.02), M.MCMCStrategy(opacity_reg=0.01, scale_reg=0.02)
    m = make_model(n, 0, 120 + sd, sd)
    loss_ref, go_ref, gs_ref = mr.regularization(st_o, m.opacities, m.scales)
    to, ts = dev(m.opacities), dev(m.scales)
    loss = M.regularization_loss(st_d, to, ts)                                  # NULL gradient pointers: the loss only
    torch.cuda.synchronize()
    e = abs(float(loss) - loss_ref) / abs(loss_ref)
    print(f"\nregulariser n={n} sd={sd}: loss {float(loss):.8f} vs float64 {loss_ref:.8f} ({e:.2e})")
    assert e <= TRANSC
    # gradients w.r.t. the ACTIVATED values, added onto what is there: v_after == fp32(v_before + c), bit for bit
    rng = np.random.default_rng(5)
    vo0, vs0 = rng.normal(size=(n, 1)).astype(f32), rng.normal(size=(n, 3)).astype(f32)
    vo, vs = dev(vo0), dev(vs0)
    dirty = torch.full((max(int(pkg._lib.load().gsr_mcmc_regularization_scratch_bytes(n)), 4),), 0xFF, dtype=torch.uint8, device="cuda")
    loss2 = M.regularization_loss(st_d, to, ts, vopacities=vo, vscales=vs, scratch=dirty)
    torch.cuda.synchronize()
    assert float(loss2) == float(loss)
    c_o = f32(st_d.opacity_reg) / f32(n)
    c_s = f32(st_d.scale_reg) / f32(n * sd)
    assert np.array_equal(host(vo), (vo0 + c_o).astype(f32))
    want = vs0.copy()
    want[:, :sd] = (vs0[:, :sd] + c_s).astype(f32)                              # scale_dims = 1: row 0 only
    assert np.array_equal(host(vs), want)
    # through the prologue pullback: the raw gradients are opacity_reg·a(1-a)/N and scale_reg·exp(s)/(N·d)
    shs, oa, sa = R.prologue_forward(torch.zeros((n, 1, 3), device="cuda"), None, to, ts)
    vo, vs = torch.zeros((n, 1), device="cuda"), torch.zeros((n, 3), device="cuda")
    M.regularization_loss(st_d, to, ts, vopacities=vo, vscales=vs)
    _, _, g_o, g_s = R.prologue_backward(oa, sa, torch.zeros((n, 1, 3), device="cuda"), vo, vs, scale_dims=sd)
    torch.cuda.synchronize()
    a, ex = host(oa), host(sa)
    assert np.array_equal(host(g_o), (c_o * (a * (f32(1) - a))).astype(f32))    # bit-exact from the device's own activations
    assert np.array_equal(host(g_s), (c_s * ex[:, :sd]).astype(f32))
    assert rel_l2(host(g_o), go_ref) <= 2 * TRANSC and rel_l2(host(g_s), gs_ref) <= 2 * TRANSC
    with pytest.raises(ValueError):
        M.regularization_loss(st_d, to, ts, vscales=torch.zeros((n, sd + 1), device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# 8. training chain through the harness
# ---------------------------------------------------------------------------------------------------------------------
CHAIN = dict(torch_pool_gb=0, width=96, height=64, n_gt=3000, n_init=500, n_views=4, seed=77, strategy="mcmc",
             mcmc=dict(start_refine=1, refine_every=2, grow_factor=1.25, max_cap=900))


def assert_same_state(a, b):
    assert len(a.gs) == len(b.gs)
    for k in TH.GROUPS:
        assert torch.equal(getattr(a.gs, k), getattr(b.gs, k)), k
        assert torch.equal(a.opts[k].mu, b.opts[k].mu) and torch.equal(a.opts[k].nu, b.opts[k].nu), k
        assert a.opts[k].current_step == b.opts[k].current_step, k
    assert a.strategy.state_dict() == b.strategy.state_dict()


def test_training_chain_with_the_mcmc_strategy(pkg, tmp_path):
    p = TH.Protocol(**CHAIN)
    gt = TH.ground_truth(pkg, p)
    init = TH.initial_model(p, gt)
    h = TH.Harness(pkg, p, init=init)
    ck = str(tmp_path / "step4.safetensors")
    sizes = []
    for step in range(1, 9):
        h.step()
        sizes.append(len(h.gs))
        if step == 4:
            h.save(ck)
    torch.cuda.synchronize()
    assert sizes == [500, 625, 625, 781, 781, 900, 900, 900], sizes        # the schedule, stopping at the cap
    assert [d["step"] for d in h.densify_log] == [2, 4, 6, 8]
    assert h.nonfinite() == 0 and np.isfinite(h.loss_values()).all()
    for k in TH.GROUPS:
        assert torch.isfinite(getattr(h.gs, k)).all() and torch.isfinite(h.opts[k].mu).all() and torch.isfinite(h.opts[k].nu).all(), k
        assert h.opts[k].mu.numel() == getattr(h.gs, k).numel()
    assert h.strategy.noise_steps == 8 and 4 <= h.strategy.sample_rounds <= 7   # noise every step; 3 growths + <= 4 relocations
    # the same seed again: identical bits
    h2 = TH.Harness(pkg, p, targets=h.targets, init=init)
    h2.run(8)
    torch.cuda.synchronize()
    assert_same_state(h, h2)
    assert torch.equal(torch.stack(h.losses), torch.stack(h2.losses))
    # checkpointed after step 4 and resumed: equal to the uninterrupted run, bit for bit
    r = TH.Harness.resume(pkg, p, ck, targets=h.targets)
    assert r.step_no == 4 and len(r.gs) == 781 and r.strategy.noise_steps == 4
    r.run(4)
    torch.cuda.synchronize()
    assert_same_state(h, r)
    assert torch.equal(torch.stack(r.losses), torch.stack(h.losses[4:]))
    for x in (h, h2, r):
        x.close()
