"""CPU checks of the MCMC strategy (no GPU): the numpy restatement tests/mcmc_ref.py is pinned to the reference — its own
"MCMC relocation (Eq. 9)" test set (test/runtests.jl:454-484), the binomial table, the sampler's edge cases, the growth
schedule under Julia's Float32 product — and the library exports the gsr_mcmc_* entry points with their argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import mcmc_ref as mr

f32 = np.float32


@pytest.fixture(scope="module")
def strategy():
    return mr.Strategy()


# ---- the reference's own test set, on the restatement ----
def test_eq9_ratio_one_is_the_identity(strategy):
    for o in (f32(0.01), f32(0.3), f32(0.9)):
        new_o, coeff = mr.relocation_params(strategy, o, 1)
        assert abs(float(new_o) - float(o)) <= 1e-6
        assert abs(float(coeff) - 1.0) <= 1e-5


def test_eq9_ratio_two_closed_form(strategy):
    for o in (f32(0.1), f32(0.5), f32(0.95)):
        new_o, coeff = mr.relocation_params(strategy, o, 2)
        assert abs(float(new_o) - (1.0 - math.sqrt(1.0 - float(o)))) <= 1e-5
        assert 0.0 < float(coeff) < 1.0


def test_eq9_monotone_over_the_ratio(strategy):
    vals = [mr.relocation_params(strategy, f32(0.99), r) for r in range(1, strategy.n_max + 1)]
    new_o = np.array([float(v[0]) for v in vals])
    coeff = np.array([float(v[1]) for v in vals])
    assert (new_o >= float(f32(strategy.min_opacity))).all() and (new_o < 1.0).all()
    assert (np.diff(new_o) <= 0).all()
    assert (coeff > 0).all() and (np.diff(coeff) <= 0).all() and coeff[0] <= 1.0 + 1e-5   # prev_coeff starts at 1f0 + 1f-5


def test_eq9_new_opacity_is_floored_at_min_opacity(strategy):
    new_o, coeff = mr.relocation_params(strategy, f32(0.004), 2)
    assert f32(new_o) == f32(strategy.min_opacity)
    assert np.isfinite(coeff) and float(coeff) > 0.0


def test_binomial_table_against_exact_binomials(strategy):
    b = strategy.binoms
    assert b.shape == (51, 51) and b.dtype == np.float32
    for n in range(51):
        for k in range(51):
            if k > n:
                assert b[n, k] == 0.0
                continue
            exact = math.comb(n, k) * (-1.0) ** k / math.sqrt(k + 1)
            # Float32(b) · sign / sqrt(Float32(k+1)): three fp32 roundings (the running double product is exact to 1e-15)
            assert abs(float(b[n, k]) - exact) <= 3 * 2.0 ** -24 * abs(exact), (n, k)


def test_the_package_builds_the_same_table(pkg):
    assert np.array_equal(pkg.mcmc.binom_coefficients(51), mr.binom_coefficients(51))
    assert np.array_equal(pkg.mcmc.MCMCStrategy(n_max=7).binoms, mr.binom_coefficients(7))


# ---- the integer sampler ----
def test_sampler_edges():
    q = np.array([0, 0, 5, 0, 0, 0, 3, 1, 0, 0], np.int64)
    total = int(q.sum())
    assert mr.select_rows(q, [0]).tolist() == [2]                   # r = 0: the first positive-weight row
    assert mr.select_rows(q, [total - 1]).tolist() == [7]           # r = total - 1: the last positive-weight row
    rows = mr.select_rows(q, list(range(total)))
    assert rows.tolist() == [2] * 5 + [6] * 3 + [7]                  # every r lands in a positive-weight row, ∝ its weight
    assert not np.isin(rows, np.flatnonzero(q == 0)).any()
    s, counts, tot = mr.multinomial_sample(q, 400, seed=11)
    assert tot == total and s.shape == (400,) and counts.sum() == 400
    assert set(s.tolist()) <= {2, 6, 7} and np.array_equal(counts, np.bincount(s, minlength=10))
    s0, c0, t0 = mr.multinomial_sample(np.zeros(6, np.int64), 9, seed=11)   # total = 0 yields nothing
    assert t0 == 0 and s0.size == 0 and not c0.any()


def test_sampler_is_uniform_on_the_total():
    """r = mulhi64(h, total) of 64 well-mixed bits: the draws follow the weights (a 6-sigma band on 20 000 draws)."""
    q = np.array([1 << 28, 0, 3 << 28, 1 << 29, 0, 1 << 27], np.int64)
    m = 20_000
    _, counts, total = mr.multinomial_sample(q, m, seed=4242)
    p = q / total
    assert (np.abs(counts - m * p) <= 6 * np.sqrt(m * p * (1 - p)) + 1e-9).all()
    assert all(0 <= r < total for r in mr.draw_positions(7, 50, total))


def test_weights_and_dead_mask():
    op = np.array([[-30.0], [0.0], [30.0], [math.log(0.004 / 0.996)], [2.0]], f32)
    sc = np.array([[-3, -3, -3], [-3, -3, -3], [-3, -3, -3], [-3, -3, -3], [-3, 1.0, -3]], f32)
    q, dead = mr.weights(op, sc, 0.005, np.log(f32(0.1) * f32(5.0)), with_dead=True)
    assert dead.tolist() == [True, False, False, True, True]         # opacity, -, -, opacity, scale
    assert q.tolist() == [0, 1 << 29, 1 << 30, 0, 0]
    q_all, none = mr.weights(op)
    assert none is None and (q_all > 0).sum() == 4 and q_all[0] == 0   # sigmoid(-30)·2^30 < 1


# ---- the growth schedule ----
def test_n_new_schedule_is_julias_float32_product():
    S = mr.Strategy
    assert mr.n_new_gaussians(S(grow_factor=1.05), 1000) == 50
    assert mr.n_new_gaussians(S(grow_factor=1.05, max_cap=1020), 1000) == 20     # clipped at max_cap
    assert mr.n_new_gaussians(S(grow_factor=1.05, max_cap=1000), 1000) == 0 and mr.n_new_gaussians(S(max_cap=900), 1000) < 0
    assert mr.n_new_gaussians(S(grow_factor=1.05), 10) == 0                      # floor(10.5) - 10
    # Float32(1.05) * Float32(n) is NOT the double product: 1.05f0 = 1.0499999523..., so n = 20 gives 20.999999 -> 20 in
    # double, but the fp32 product rounds to 21.0
    assert f32(1.05) * f32(20) == f32(21) and int(np.floor(float(f32(1.05)) * 20)) == 20
    assert mr.n_new_gaussians(S(grow_factor=1.05), 20) == 1
    n, seq = 500, []
    s = S(grow_factor=1.25, max_cap=900)
    for _ in range(4):
        n += max(mr.n_new_gaussians(s, n), 0)
        seq.append(n)
    assert seq == [625, 781, 900, 900]


def test_package_schedule_and_seeds_match(pkg):
    M = pkg.mcmc
    st = M.MCMCStrategy(grow_factor=1.25, max_cap=900, seed=9)
    for n in (1, 20, 500, 625, 781, 899, 900, 1000):
        assert M.n_new_gaussians(st, n) == mr.n_new_gaussians(mr.Strategy(grow_factor=1.25, max_cap=900), n)
    assert M.n_new_gaussians(M.MCMCStrategy(), 20) == 1
    # the reference's defaults (mcmc.jl:60-72)
    d = M.MCMCStrategy()
    assert (d.max_cap, d.start_refine, d.stop_refine, d.refine_every, d.n_max) == (2_000_000, 500, 25_000, 100, 51)
    assert (f32(d.min_opacity), f32(d.max_scale), f32(d.grow_factor), f32(d.noise_lr), f32(d.opacity_reg), f32(d.scale_reg)) == \
           (f32(0.005), f32(0.1), f32(1.05), f32(5e5), f32(0.01), f32(0.01))
    assert [d.refining(s) for s in (500, 600, 650, 24_900, 25_000)] == [False, True, False, True, False]
    # separate, advancing, checkpointable seed streams
    a, b = M.MCMCStrategy(seed=9), M.MCMCStrategy(seed=9)
    s1 = [a.next_sample_seed(), a.next_sample_seed(), a.next_noise_seed(), a.next_noise_seed()]
    assert len(set(s1)) == 4 and a.state_dict() == {"seed_base": 9, "sample_rounds": 2, "noise_steps": 2}
    b.load_state_dict(a.state_dict())
    assert (b.next_sample_seed(), b.next_noise_seed()) == (a.next_sample_seed(), a.next_noise_seed())
    assert M.MCMCStrategy(seed=10).next_noise_seed() != M.MCMCStrategy(seed=9).next_noise_seed()


def test_checkpoint_carries_the_mcmc_counters(pkg, tmp_path):
    """checkpoint.save_state(strategy=...) / load_state resume the sampling and noise sequences; a DefaultStrategy file loads into
    an MCMCStrategy without touching it (and the reverse)."""
    ck, M = pkg.checkpoint, pkg.mcmc
    n = 5
    g = pkg.ply.GaussianModel(np.zeros((n, 3), f32), np.zeros((n, 1, 3), f32), np.zeros((n, 0, 3), f32), np.zeros((n, 3), f32),
                              np.zeros((n, 4), f32), np.zeros((n, 1), f32), 0, 0)

    class _Opt:
        def __init__(self, numel): self.mu, self.nu, self.current_step = np.zeros(numel, f32), np.zeros(numel, f32), 3

    opts = lambda: {k: _Opt(int(np.asarray(getattr(g, k)).size)) for k in ck.OPTIMIZER_NAMES}  # noqa: E731
    st = M.MCMCStrategy(seed=77)
    st.next_sample_seed(); st.next_noise_seed(); st.next_noise_seed()
    path = str(tmp_path / "mcmc.safetensors")
    ck.save_state(path, g, opts(), 12, strategy=st)
    meta = ck.load_checkpoint(path).meta
    assert (meta["strategy.seed_base"], meta["strategy.sample_rounds"], meta["strategy.noise_steps"]) == ("77", "1", "2")
    st2 = M.MCMCStrategy(seed=1)
    _, step = ck.load_state(path, opts(), strategy=st2)
    assert step == 12 and st2.state_dict() == st.state_dict()
    assert st2.next_noise_seed() == st.next_noise_seed()

    import torch

    class _Default:   # what checkpoint.py reads of a densification.DefaultStrategy: its seed position and its running statistics
        def __init__(self):
            self.split_seed_base, self.split_rounds = 5, 6
            self.max_radii = torch.arange(n, dtype=torch.int32)
            self.accum_grad_means_2d, self.denom = torch.full((n,), 0.25), torch.full((n,), 2.0)

        def state_dict(self): return {"split_seed_base": self.split_seed_base, "split_rounds": self.split_rounds}
        def load_state_dict(self, d): self.split_seed_base, self.split_rounds = int(d["split_seed_base"]), int(d["split_rounds"])

    dflt = _Default()
    ck.load_state(path, opts(), strategy=dflt)            # an MCMC file: a DefaultStrategy keeps its own position
    assert (dflt.split_seed_base, dflt.split_rounds) == (5, 6)
    path2 = str(tmp_path / "default.safetensors")
    ck.save_state(path2, g, opts(), 3, strategy=dflt)
    st3 = M.MCMCStrategy(seed=2)
    assert all(f"strategy.{k}" in ck.load_checkpoint(path2) for k in ck.STRATEGY_STATS)   # the file holds the statistics ...
    ck.load_state(path2, opts(), strategy=st3)                                            # ... which an MCMCStrategy has no use for
    assert st3.state_dict() == {"seed_base": 2, "sample_rounds": 0, "noise_steps": 0}
    assert not any(hasattr(st3, k) for k in ck.STRATEGY_STATS)
    back = _Default()
    back.max_radii = back.accum_grad_means_2d = back.denom = None
    ck.load_state(path2, opts(), strategy=back)                                           # a DefaultStrategy still gets them back
    assert torch.equal(back.max_radii, dflt.max_radii) and torch.equal(back.denom, dflt.denom)


# ---- the library ----
NEW_SYMBOLS = ("gsr_mcmc_weights", "gsr_mcmc_sample_scratch_bytes", "gsr_mcmc_sample", "gsr_mcmc_split_sampled",
               "gsr_mcmc_relocation_params", "gsr_mcmc_relocate_rows", "gsr_mcmc_inject_noise",
               "gsr_mcmc_regularization_scratch_bytes", "gsr_mcmc_regularization")


def test_library_exports_the_mcmc_entry_points(pkg):
    L = pkg._lib
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert lib.gsr_abi_version() == 6
    M = pkg.mcmc   # imports without a GPU
    for f in ("MCMCStrategy", "regularization_loss", "relocate_gaussians", "add_gaussians", "split_sampled", "inject_noise",
              "post_train_step"):
        assert hasattr(M, f), f


def test_scratch_sizes_and_argument_checks(pkg):
    """Everything the entry points refuse before touching the GPU (no launch happens here)."""
    L = pkg._lib
    lib = L.load()
    E = L.GSR_E_INVALID_ARG
    assert lib.gsr_mcmc_sample_scratch_bytes(0) == 0 and lib.gsr_mcmc_sample_scratch_bytes(-3) == 0
    assert lib.gsr_mcmc_sample_scratch_bytes(1) == 16 and lib.gsr_mcmc_sample_scratch_bytes(1024) == 8 * 1025
    assert lib.gsr_mcmc_sample_scratch_bytes(1025) == 8 * (2 + 1025)
    assert lib.gsr_mcmc_regularization_scratch_bytes(0) == 0 and lib.gsr_mcmc_regularization_scratch_bytes(1) == 8
    assert lib.gsr_mcmc_regularization_scratch_bytes(683) == 16     # 3·683 = 2049 flat elements: two 2048-element chunks
    x = C.c_void_p(4096)   # a non-null address nothing reads: every call below fails in validation
    assert lib.gsr_mcmc_weights(-1, 3, x, x, 0.005, 0.0, x, x, None) == E
    assert lib.gsr_mcmc_weights(5, 2, x, x, 0.005, 0.0, x, x, None) == E and b"scale_dims" in lib.gsr_last_error_string()
    assert lib.gsr_mcmc_weights(5, 3, None, x, 0.005, 0.0, x, x, None) == E
    assert lib.gsr_mcmc_weights(0, 3, None, None, 0.005, 0.0, None, None, None) == 0
    assert lib.gsr_mcmc_sample(5, x, -1, 0, x, x, x, x, 1 << 20, None) == E
    assert lib.gsr_mcmc_sample(5, x, 3, 0, x, x, x, x, 8, None) == E and b"scratch" in lib.gsr_last_error_string()
    assert lib.gsr_mcmc_sample(5, x, 3, 0, x, x, x, C.c_void_p(4100), 1 << 20, None) == E   # misaligned scratch
    assert lib.gsr_mcmc_sample(5, None, 3, 0, x, x, x, x, 1 << 20, None) == E
    assert lib.gsr_mcmc_sample(5, None, 0, 0, None, None, None, None, 0, None) == 0            # m = 0: nothing to do
    assert lib.gsr_mcmc_split_sampled(5, 3, x, x, 0, 0.005, x, x, None) == E and b"n_max" in lib.gsr_last_error_string()
    assert lib.gsr_mcmc_split_sampled(5, 3, None, x, 51, 0.005, x, x, None) == E
    assert lib.gsr_mcmc_relocation_params(5, x, x, x, 0, 0.005, x, x, None) == E
    assert lib.gsr_mcmc_relocation_params(0, None, None, None, 51, 0.005, None, None, None) == 0
    g = (L.ComposeGroup * 2)(L.ComposeGroup(4096, 8192, 3, 0), L.ComposeGroup(None, 8192, 3, 1))
    assert lib.gsr_mcmc_relocate_rows(g, 2, 10, x, x, 4, None) == E and b"in place" in lib.gsr_last_error_string()
    assert lib.gsr_mcmc_relocate_rows(g, 25, 10, x, x, 4, None) == E
    assert lib.gsr_mcmc_relocate_rows(g, 2, 10, x, x, 0, None) == 0
    assert lib.gsr_mcmc_inject_noise(5, 3, x, x, x, C.c_void_p(4100), 1.0, 1.0, 0, None) == E and b"aligned" in lib.gsr_last_error_string()
    assert lib.gsr_mcmc_inject_noise(5, 3, None, x, x, x, 1.0, 1.0, 0, None) == E
    assert lib.gsr_mcmc_inject_noise(0, 3, None, None, None, None, 1.0, 1.0, 0, None) == 0
    assert lib.gsr_mcmc_regularization(5, 3, x, x, 0.01, 0.01, x, None, None, x, 4, None) == E and b"scratch" in lib.gsr_last_error_string()
    assert lib.gsr_mcmc_regularization(5, 3, x, x, 0.01, 0.01, None, None, None, x, 64, None) == E
    import torch
    with pytest.raises(ValueError):
        pkg.mcmc.regularization_loss(pkg.mcmc.MCMCStrategy(), torch.zeros((4, 1)), torch.zeros((4, 3)))   # no CPU path
    with pytest.raises(ValueError):
        pkg.mcmc.MCMCStrategy(n_max=0)
