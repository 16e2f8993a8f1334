"""SH codebook fine-tuning without a GPU: what pins tests/vq_grad_ref.py — the restatement
tests/test_gpu_vq_grad.py holds the kernels to —, the host side of the four entry points and the checkpoint group."""
import types

import numpy as np
import pytest
import torch

import vq_grad_ref as R

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_radix_is_the_headers(pkg):
    assert R.RADIX == pkg._lib.VQ_SUM_RADIX == 64
    assert [R.levels(n) for n in (1, 64, 65, 4096, 4097, 262144, 262145, (1 << 24) - 1)] == [1, 1, 2, 2, 3, 3, 4, 4]


def test_group_is_the_stable_counting_sort():
    rng = np.random.default_rng(1)
    idx = rng.integers(0, 9, 300).astype(np.uint16)
    idx[::7] = 65535                                        # >= K: read as K - 1
    order, offsets = R.group(idx, 7)
    c = np.minimum(idx.astype(np.int64), 6)
    want = sorted(range(300), key=lambda i: (c[i], i))
    assert order.dtype == np.uint32 and order.tolist() == want
    assert offsets.tolist() == [int((c < j).sum()) for j in range(8)] and offsets[-1] == 300
    o1, f1 = R.group(np.zeros(5, np.uint16), 3)
    assert o1.tolist() == [0, 1, 2, 3, 4] and f1.tolist() == [0, 5, 5, 5]


@pytest.mark.parametrize("n,K,dim", [(1, 1, 1), (5, 3, 2), (64, 2, 3), (65, 2, 3), (200, 1, 2), (300, 5, 4), (4200, 3, 1)])
def test_restatement_against_the_literal_loop(n, K, dim):
    """Small cases, one of them past 4096 rows in one code (three levels): every bit of the vectorised restatement is the
    per-code, per-column, per-chunk Python loop's."""
    rng = np.random.default_rng(100 * n + K)
    g = (rng.normal(size=(n, dim)) * np.exp2(rng.integers(-10, 10, size=(n, dim)))).astype(f32)
    idx = rng.integers(0, K + 1, n).astype(np.uint16)        # K itself: clamped
    if n == 4200:
        idx[:4150] = 1
    order, offsets = R.group(idx, K)
    got = R.codebook_grad(g, order, offsets, K)
    assert np.array_equal(bits(got), bits(R.codebook_grad_literal(g, idx, K)))


def test_restatement_within_the_derived_bound_of_float64():
    """|g_codebook - exact| <= 2^-16 · Σ|g| per code and column (63 · 2^-24 per level, four levels compound to < 256 · 2^-24):
    gradients spread over e^±3, 80 % of 100 000 rows in one code."""
    rng = np.random.default_rng(2)
    n, K, dim = 100_000, 9, 45
    g = (rng.normal(size=(n, dim)) * np.exp(rng.uniform(-3, 3, size=(n, 1)))).astype(f32)
    idx = rng.integers(0, K, n).astype(np.uint16)
    idx[rng.uniform(size=n) < 0.8] = 4
    order, offsets = R.group(idx, K)
    got = R.codebook_grad(g, order, offsets, K).astype(np.float64)
    exact = np.zeros((K, dim))
    mass = np.zeros((K, dim))
    np.add.at(exact, idx.astype(np.int64), g.astype(np.float64))
    np.add.at(mass, idx.astype(np.int64), np.abs(g.astype(np.float64)))
    ratio = np.abs(got - exact) / mass
    print(f"max |err| / sum|g| = 2^{np.log2(ratio.max()):.1f}")
    assert (np.abs(got - exact) <= 2.0 ** -16 * mass).all()


def test_single_row_passes_bits_through_and_empty_is_plus_zero():
    payload = np.array([0x7FC12345, 0xFFA00001, 0x80000000, 0x7F800000], np.uint32).view(f32)   # NaNs with payloads, -0.0, +Inf
    g = np.stack([payload, np.array([1.0, -0.0, -0.0, 2.0], f32), np.array([3.0, -0.0, -0.0, 4.0], f32)])
    idx = np.array([3, 1, 1], np.uint16)
    order, offsets = R.group(idx, 5)
    out = R.codebook_grad(g, order, offsets, 5)
    assert np.array_equal(bits(out[3]), bits(payload))                     # |L| = 1: no add touched it
    assert np.array_equal(bits(out[1]), bits(np.array([4.0, -0.0, -0.0, 6.0], f32)))   # -0 + -0 = -0
    for j in (0, 2, 4):
        assert np.array_equal(bits(out[j]), np.zeros(4, np.uint32))       # empty: +0.0
    # a NaN / Inf row poisons its own code and column only
    g2 = np.ones((130, 3), f32)
    g2[70, 1] = np.nan
    g2[100, 2] = np.inf
    idx2 = np.zeros(130, np.uint16)
    idx2[100:] = 1
    out2 = R.codebook_grad(g2, *R.group(idx2, 2), 2)
    assert out2[0].tolist()[0] == 100.0 and np.isnan(out2[0, 1]) and out2[0, 2] == 100.0
    assert out2[1].tolist()[:2] == [30.0, 30.0] and np.isposinf(out2[1, 2])


def test_scratch_sizes(pkg):
    lib = pkg._lib.load()
    gs, cs = lib.gsr_vq_group_scratch_bytes, lib.gsr_vq_codebook_grad_scratch_bytes
    for n, k in ((0, 4), (-1, 4), (1 << 24, 4), (8, 0), (8, 65537)):
        assert gs(n, k) == 0 and cs(n, k, 45) == 0
    assert cs(8, 4, 0) == 0 and cs(8, 4, 49) == 0
    ns = [1, 63, 64, 65, 1024, 1025, 4096, 4097, 70_000, 262_144, 262_145, 1_000_000, (1 << 24) - 1]
    for k in (1, 256, 4096, 65536):
        g = [gs(n, k) for n in ns]
        c = [cs(n, k, 45) for n in ns]
        assert all(v > 0 and v % 16 == 0 for v in g + c)
        assert g == sorted(g) and c == sorted(c), (k, g, c)               # monotone in n
    # the documented layout: the prefixes, then floor(n / 64^l) + min(K, n) partial rows per level below the last
    a16 = lambda b: (b + 15) & ~15  # noqa: E731
    assert cs(64, 7, 45) == a16(8 * 4)
    assert cs(65, 7, 45) == a16(2 * 8 * 4) + a16((1 + 7) * 45 * 4)
    assert cs(70_000, 7, 45) == a16(3 * 8 * 4) + a16((1093 + 7) * 45 * 4) + a16((17 + 7) * 45 * 4)
    assert gs(1025, 7) == a16(1025 * 4) + a16((256 * 2 + 1) * 4) + a16(1025 * 2)


def test_error_codes_that_need_no_device(pkg):
    lib = pkg._lib.load()
    bad = pkg._lib.GSR_E_INVALID_ARG
    grp, grad = lib.gsr_vq_group, lib.gsr_vq_codebook_grad
    for n, k, d in ((-1, 4, 45), (1 << 24, 4, 45), (8, 0, 45), (8, 65537, 45), (8, 4, 0), (8, 4, 49)):
        if d == 45:
            assert grp(n, k, None, None, None, None, 0, None) == bad
        assert grad(n, k, d, None, 48, None, None, None, None, 0, None) == bad
    # n == 0: GSR_OK, nothing is launched, no pointer is looked at; but the stride is still checked
    assert grp(0, 4, None, None, None, None, 0, None) == 0
    assert grad(0, 4, 45, None, 45, None, None, None, None, 0, None) == 0
    assert grad(0, 4, 45, None, 44, None, None, None, None, 0, None) == bad
    A = 1 << 20
    nbg, nbc = lib.gsr_vq_group_scratch_bytes(8, 4), lib.gsr_vq_codebook_grad_scratch_bytes(8, 4, 45)
    # group: nulls, alignment, scratch (the addresses are never dereferenced)
    for kw in (dict(ind=None), dict(order=None), dict(off=None), dict(scr=None), dict(ind=A + 1), dict(order=A + 2), dict(off=A + 2),
               dict(scr=A + 8), dict(nb=nbg - 1)):
        a = dict(ind=A, order=A, off=A, scr=A, nb=nbg); a.update(kw)
        assert grp(8, 4, a["ind"], a["order"], a["off"], a["scr"], a["nb"], None) == bad, kw
    assert grp(8, 4, A, A, A, A, nbg - 1, None) == bad and b"scratch" in lib.gsr_last_error_string()
    for kw in (dict(g=None), dict(order=None), dict(off=None), dict(out=None), dict(scr=None), dict(g=A + 2), dict(out=A + 1),
               dict(order=A + 2), dict(off=A + 1), dict(scr=A + 8), dict(nb=nbc - 1), dict(stride=44), dict(stride=-1)):
        a = dict(g=A, stride=45, order=A, off=A, out=A, scr=A, nb=nbc); a.update(kw)
        assert grad(8, 4, 45, a["g"], a["stride"], a["order"], a["off"], a["out"], a["scr"], a["nb"], None) == bad, kw
    assert grad(8, 4, 45, A, 44, A, A, A, A, nbc, None) == bad and b"row_stride" in lib.gsr_last_error_string()
    S = pkg.sh_codebook
    sh = S.SHCodebook(torch.zeros((4, 45)), torch.zeros(8, dtype=torch.int16).view(torch.uint16), (8, 15, 3))
    with pytest.raises(ValueError):
        sh.groups()                                                      # CPU tensors: no CPU path
    with pytest.raises(ValueError):
        S.codebook_grad(torch.zeros((8, 15, 3)), sh)
    with pytest.raises(ValueError):
        S.SHCodebookFineTuner(sh)


def test_checkpoint_group_round_trip_on_host_tensors(pkg, tmp_path):
    """sh_codebook.{codebook, indices, shape} and the optimizer's moments through save_state / load_state; a file without the
    group leaves the object as built; existing callers (no keyword) write no such keys."""
    S, CK = pkg.sh_codebook, pkg.checkpoint
    rng = np.random.default_rng(3)
    K, D, n = 5, 6, 11

    def tuner(seed):
        r = np.random.default_rng(seed)
        sh = S.SHCodebook(torch.from_numpy(r.normal(size=(K, D)).astype(f32)),
                          torch.from_numpy(r.integers(0, K, n).astype(np.int16)).view(torch.uint16), (n, 2, 3))
        opt = types.SimpleNamespace(mu=torch.from_numpy(r.normal(size=K * D).astype(f32)),
                                    nu=torch.from_numpy(r.uniform(size=K * D).astype(f32)), current_step=int(r.integers(1, 99)))
        return types.SimpleNamespace(sh=sh, optimizer=opt)

    g = pkg.ply.GaussianModel(rng.normal(size=(n, 3)).astype(f32), rng.normal(size=(n, 1, 3)).astype(f32),
                              rng.normal(size=(n, 2, 3)).astype(f32), rng.normal(size=(n, 3)).astype(f32),
                              rng.normal(size=(n, 4)).astype(f32), rng.normal(size=(n, 1)).astype(f32), 1, 1)
    opts = {name: types.SimpleNamespace(mu=np.zeros(np.asarray(getattr(g, name)).size, f32),
                                        nu=np.zeros(np.asarray(getattr(g, name)).size, f32), current_step=7)
            for name in CK.OPTIMIZER_NAMES}
    a, b = tuner(10), tuner(11)
    CK.save_state(str(tmp_path / "with.safetensors"), g, opts, 7, sh_codebook=a)
    CK.save_state(str(tmp_path / "without.safetensors"), g, opts, 7)
    ck = CK.load_checkpoint(str(tmp_path / "with.safetensors"))
    assert ck.raw_tensor("sh_codebook.codebook").shape == (D, K) and ck.raw_tensor("sh_codebook.indices").dtype == np.uint16
    assert ck.tensor("sh_codebook.shape").tolist() == [n, 2, 3] and ck.meta["sh_codebook.optimizer.n_moments"] == "1"
    assert not any(k.startswith("sh_codebook") for k in CK.load_checkpoint(str(tmp_path / "without.safetensors"))._keys)
    before = (b.sh.codebook.clone(), b.sh.indices.clone(), b.optimizer.mu.clone(), b.optimizer.current_step)
    keep = b.sh.codebook
    CK.load_state(str(tmp_path / "without.safetensors"), opts, sh_codebook=b)     # no group: as built
    assert torch.equal(b.sh.codebook, before[0]) and torch.equal(b.sh.indices.view(torch.int16), before[1].view(torch.int16))
    assert torch.equal(b.optimizer.mu, before[2]) and b.optimizer.current_step == before[3]
    CK.load_state(str(tmp_path / "with.safetensors"), opts)                       # without the keyword the group is ignored
    CK.load_state(str(tmp_path / "with.safetensors"), opts, sh_codebook=b)
    assert b.sh.codebook is keep and torch.equal(b.sh.codebook.view(torch.int32), a.sh.codebook.view(torch.int32))
    assert b.sh.indices.dtype == torch.uint16 and torch.equal(b.sh.indices.view(torch.int16), a.sh.indices.view(torch.int16))
    assert b.sh.shape == (n, 2, 3) and b.optimizer.current_step == a.optimizer.current_step
    assert torch.equal(b.optimizer.mu, a.optimizer.mu) and torch.equal(b.optimizer.nu, a.optimizer.nu)
    # a bare SHCodebook: no moments in the file, and a codebook of another shape is refused
    tensors, meta = {}, {}
    CK.write_sh_codebook(tensors, meta, "sh_codebook", a.sh)
    assert sorted(tensors) == ["sh_codebook.codebook", "sh_codebook.indices", "sh_codebook.shape"] and meta == {}
    other = S.SHCodebook(torch.zeros((K + 1, D)), torch.zeros(n, dtype=torch.int16).view(torch.uint16), (n, 2, 3))
    with pytest.raises(ValueError):
        CK.read_sh_codebook(other, ck, "sh_codebook")
