"""The SH codebook k-means without a GPU: what pins tests/vq_ref.py — the restatement tests/test_gpu_vq.py
holds the kernels to — and the host side of sh_codebook (archive round trip, weights)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import vq_ref as R

f32 = np.float32

C_SRC = r"""
#include <math.h>
void fmaf_many(const float* a, const float* b, const float* c, float* out, long n) {
    for (long i = 0; i < n; i++) out[i] = fmaf(a[i], b[i], c[i]);
}
"""


@pytest.fixture(scope="module")
def c_fmaf(tmp_path_factory):
    """C `fmaf` over arrays, compiled with the oracle's compiler (oracle/Makefile: $(CC), gcc by default)."""
    d = tmp_path_factory.mktemp("fmaf")
    src, so = d / "fmaf_many.c", d / "libfmaf_many.so"
    src.write_text(C_SRC)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-std=c99", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-o", str(so), str(src), "-lm"])
    lib = ctypes.CDLL(str(so))
    lib.fmaf_many.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_long]
    lib.fmaf_many.restype = None

    def run(a, b, c):
        a, b, c = (np.ascontiguousarray(v, f32) for v in (a, b, c))
        out = np.empty_like(a)
        lib.fmaf_many(a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data, a.size)
        return out
    return run


def _same(got, want):
    """Bit for bit, a NaN for a NaN."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def test_fmaf_emulation_on_random_triples(c_fmaf):
    """4 M triples: normal-scale values, values across the whole exponent range (subnormals, overflow), raw bit patterns."""
    rng = np.random.default_rng(11)
    n = 4_000_000 // 4
    parts = [rng.normal(size=(3, n)).astype(f32),
             (rng.normal(size=(3, n)) * np.exp2(rng.integers(-30, 30, size=(3, n)))).astype(f32),
             (rng.normal(size=(3, n)) * np.exp2(rng.integers(-80, 70, size=(3, n)))).astype(f32),
             rng.integers(0, 1 << 32, size=(3, n), dtype=np.uint64).astype(np.uint32).view(f32)]
    # products that cancel against c: the sum's error term decides
    parts[0][2] = -(parts[0][0] * parts[0][1]) * f32(1 + 2.0 ** -20)
    for a, b, c in parts:
        assert _same(R.fmaf(a, b, c), c_fmaf(a, b, c))


def _midpoint_triples(n):
    """a*b + c next to an fp32 midpoint: a = 1 ± 2^-23, b = 2^-24 (1 ∓ 2^-23), c = 1 + k 2^-23."""
    rng = np.random.default_rng(12)
    s = np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
    a = (1.0 + s * 2.0 ** -23).astype(f32)
    b = (2.0 ** -24 * (1.0 - s * 2.0 ** -23)).astype(f32)
    c = (1.0 + rng.integers(0, 1 << 22, n) * 2.0 ** -23).astype(f32)
    return a, b, c


def test_fmaf_emulation_next_to_midpoints(c_fmaf):
    """1 M triples whose exact value is 2^-70 away from a midpoint of c's binade: the emulation is C fmaf, the naive float64
    evaluation rounds twice and is wrong about half the time."""
    a, b, c = _midpoint_triples(1_000_000)
    want = c_fmaf(a, b, c)
    assert _same(R.fmaf(a, b, c), want)
    wrong = int(np.count_nonzero(R.fmaf_naive(a, b, c).view(np.uint32) != want.view(np.uint32)))
    print(f"naive float32(float64(a)*b + c): wrong on {wrong} of {a.size}")
    assert 400_000 < wrong < 600_000


def test_restatement_against_float64_kmeans_on_separated_clusters():
    """K = 12 clusters, centres 10 apart, spread 0.1, dim 45: the fp32 chain and a float64 distance agree on every index, and
    three Lloyd iterations end at the float64 means to fp32 rounding."""
    rng = np.random.default_rng(13)
    K, dim, per = 12, 45, 40
    centres = (rng.integers(-3, 4, size=(K, dim)) * 10.0)
    centres[:, 0] = np.arange(K) * 10.0   # distinct
    x = (np.repeat(centres, per, axis=0) + 0.1 * rng.normal(size=(K * per, dim))).astype(f32)
    perm = rng.permutation(K * per)
    x = x[perm]
    init = (centres + 0.5 * rng.normal(size=centres.shape)).astype(f32)
    idx, err, changed = R.assign(x, init)
    d2 = ((x.astype(np.float64)[:, None, :] - init.astype(np.float64)[None]) ** 2).sum(-1)
    assert np.array_equal(idx, d2.argmin(1).astype(np.uint16)) and changed == K * per
    assert np.array_equal(idx, (np.repeat(np.arange(K), per)[perm]).astype(np.uint16))
    assert np.allclose(err, d2.min(1), rtol=1e-5)
    c, idx2, hist = R.fit(x, K, 3, init=init)
    assert np.array_equal(idx2, idx) and hist[:, 0].tolist() == [K * per, 0, 0] and hist[:, 1].tolist() == [0, 0, 0]
    means = np.stack([x[idx == j].astype(np.float64).mean(0) for j in range(K)])
    # a row's fixed point is off by at most 2^-25 (exact from |x| >= 2^-1 on), the stored float32 by half an ulp of the mean
    assert (np.abs(c - means) <= 2.0 ** -25 + 2.0 ** -24 * np.abs(means)).all()


def test_arg_rule_nan_inf_and_ties():
    t = np.array([[np.nan, 1.0, 1.0, 0.5], [np.nan, np.nan, np.nan, np.nan], [np.nan, -np.inf, -np.inf, np.nan],
                  [np.inf, np.inf, 1.0, np.nan], [-0.0, 0.0, -1.0, np.nan]], f32)
    assert R.argbest(t).tolist() == [1, 0, 1, 0, 0]


def test_integer_sums_against_python_integers_at_the_bound():
    """(2^24 - 1) rows would overflow nothing: 255 · 2^31 per row; checked on 1000 rows of ±128 and beyond with weight 255, and
    the bound itself in Python integers."""
    assert 255 * (1 << 31) * ((1 << 24) - 1) < (1 << 63)
    x = np.array([[128.0, -128.0, 1e9, -np.inf, np.nan, 2.0 ** -25, 3 * 2.0 ** -25, 0.1]] * 1000, f32)
    wq = np.full(1000, 255, np.uint8)
    sums, wsum = R.accumulate(x, np.zeros(1000, np.uint16), 2, wq)
    q = [1 << 31, -(1 << 31), 1 << 31, -(1 << 31), 0, 0, 2, int(np.rint(np.float64(f32(0.1)) * 2.0 ** 24))]   # rne: 0.5 -> 0, 1.5 -> 2
    assert sums[0].tolist() == [255 * 1000 * v for v in q] and int(wsum[0]) == 255000
    assert not sums[1].any() and int(wsum[1]) == 0
    # accumulated into, not cleared; weights None is weight 1
    sums, wsum = R.accumulate(x[:10], np.ones(10, np.uint16), 2, None, sums, wsum)
    assert sums[1].tolist() == [10 * v for v in q] and int(wsum[1]) == 10 and int(wsum[0]) == 255000
    c, empty = R.update(np.full((3, 8), 7.0, f32), np.concatenate([sums, np.zeros((1, 8), np.int64)]), np.append(wsum, np.uint64(0)))
    assert empty == 1 and (c[2] == 7.0).all() and c[0].tolist()[:4] == [128.0, -128.0, 128.0, -128.0] and c[1, 7] == f32(q[7] / 2.0 ** 24)


def test_weights_from_scores(pkg):
    s = np.array([0.0, 1e-9, 0.5, 1.0, 2.0, 0.999 * 2.0 / 255.0], np.float64)
    w = pkg.sh_codebook.weights_from_scores(torch.from_numpy(s))
    assert w.dtype == torch.uint8 and w.tolist() == [1, 1, 64, 128, 255, 1] and np.array_equal(w.numpy(), R.weights_from_scores(s))
    assert pkg.sh_codebook.weights_from_scores(torch.zeros(3, dtype=torch.float64)).tolist() == [1, 1, 1]


def test_save_load_round_trip(pkg, tmp_path):
    S = pkg.sh_codebook
    rng = np.random.default_rng(14)
    cb = torch.from_numpy(rng.normal(size=(300, 45)).astype(f32))
    idx = torch.from_numpy(rng.integers(0, 300, 1000).astype(np.int16)).view(torch.uint16)
    a = S.SHCodebook(cb, idx, (1000, 15, 3))
    assert a.nbytes == 300 * 45 * 4 + 1000 * 2 and a.n_codes == 300
    path = tmp_path / "codebook.npz"
    a.save(path)
    b = S.SHCodebook.load(path)
    assert b.shape == (1000, 15, 3) and b.indices.dtype == torch.uint16
    assert torch.equal(b.codebook.view(torch.int32), cb.view(torch.int32)) and torch.equal(b.indices.view(torch.int16), idx.view(torch.int16))
    with np.load(path) as z:
        assert sorted(z.files) == ["codebook", "indices", "shape"] and z["indices"].dtype == np.uint16
    np.savez(tmp_path / "bad.npz", codebook=cb.numpy(), indices=np.zeros(5, np.uint16), shape=np.array([1000, 15, 3]))
    with pytest.raises(ValueError):
        S.SHCodebook.load(tmp_path / "bad.npz")


def test_fit_refuses_what_needs_no_device(pkg):
    S = pkg.sh_codebook
    with pytest.raises(ValueError):
        S.fit_sh_codebook(torch.zeros((10, 15, 3)), 4)            # a CPU tensor: no CPU path
    with pytest.raises(TypeError):
        S.fit_sh_codebook(torch.zeros((10, 15, 3), dtype=torch.float64), 4)
    lib = pkg._lib.load()
    bad = pkg._lib.GSR_E_INVALID_ARG
    for n, k, d in ((-1, 4, 45), (1 << 24, 4, 45), (8, 0, 45), (8, 65537, 45), (8, 4, 0), (8, 4, 49)):
        assert lib.gsr_vq_scratch_bytes(n, k, d) == 0
        assert lib.gsr_vq_assign(n, k, d, None, None, None, None, None, None, None, 0, None) == bad
        assert lib.gsr_vq_accumulate(n, k, d, None, None, None, None, None, None) == bad
        assert lib.gsr_vq_decode(n, k, d, None, None, None, None) == bad
    assert lib.gsr_vq_update(0, 45, None, None, None, None, None) == bad and lib.gsr_vq_update(4, 45, None, None, None, None, None) == bad
    # n == 0: GSR_OK, nothing is launched, no pointer is looked at
    assert lib.gsr_vq_assign(0, 4, 45, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.gsr_vq_accumulate(0, 4, 45, None, None, None, None, None, None) == 0
    assert lib.gsr_vq_decode(0, 4, 45, None, None, None, None) == 0
    assert lib.gsr_vq_scratch_bytes(0, 4, 45) == 0 and lib.gsr_vq_scratch_bytes(1, 257, 45) == 2 * (48 * 288 + 256) * 4
    # nulls and alignment, none of which touches the device (the addresses are never dereferenced)
    A = 1 << 20
    assert lib.gsr_vq_assign(8, 4, 45, None, A, None, A, None, None, A, 1 << 20, None) == bad
    assert lib.gsr_vq_assign(8, 4, 45, A, A, None, A + 1, None, None, A, 1 << 20, None) == bad
    assert lib.gsr_vq_assign(8, 4, 45, A, A, A + 1, A, None, None, A, 1 << 20, None) == bad
    assert lib.gsr_vq_assign(8, 4, 45, A, A, None, A, None, A + 2, A, 1 << 20, None) == bad
    assert lib.gsr_vq_assign(8, 4, 45, A, A, None, A, None, None, A + 8, 1 << 20, None) == bad
    assert lib.gsr_vq_assign(8, 4, 45, A, A, None, A, None, None, A, lib.gsr_vq_scratch_bytes(8, 4, 45) - 1, None) == bad
    assert b"scratch" in lib.gsr_last_error_string()
    assert lib.gsr_vq_accumulate(8, 4, 45, A, A, None, A + 4, A, None) == bad and lib.gsr_vq_accumulate(8, 4, 45, A, A, None, A, A + 4, None) == bad
    assert lib.gsr_vq_accumulate(8, 4, 45, A, A + 1, None, A, A, None) == bad and lib.gsr_vq_accumulate(8, 4, 45, A, None, None, A, A, None) == bad
    assert lib.gsr_vq_update(4, 45, A + 4, A, A, None, None) == bad and lib.gsr_vq_update(4, 45, A, A, A, A + 2, None) == bad
    assert lib.gsr_vq_decode(8, 4, 45, A, A + 1, A, None) == bad and lib.gsr_vq_decode(8, 4, 45, A, A, None, None) == bad
