"""-m gpu: SH codebook fine-tuning on the MI355X (csrc/vq_grad.hip through gsr_vq_group / gsr_vq_codebook_grad and sh_codebook;
DESIGN.md §24); every test fails on a build without the feature (no such symbols).
  1. group against numpy's stable argsort and bincount at every n, K and key pattern at which the sort takes another path:
     the wave's 64 rows, the workgroup's 1024, a second round of the histogram scan, keys that differ in one byte only;
  2. the gradient against the restatement of tests/vq_grad_ref.py, bit for bit: list lengths around every chunk and level
     boundary, alone and mixed, a 70 000-row code, every dim, a strided source, NaN / Inf / -0 rows, poisoned buffers;
  3. sh_codebook: codebook_grad, the autograd path against the raw chain, the fine-tuner against the steps by hand, a tiny
     fine-tuning run, and the checkpoint in the middle of one;
  4. the four entry points on guarded arenas with damaged order / offsets, the error codes with device pointers.
Every comparison is array_equal / torch.equal, on integers or float bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import scenes
import vq_grad_ref as R
from guarded import placements
from hip_helpers import dev
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu
f32 = np.float32
W = 1024                                    # rows per workgroup of the sort (csrc/vq_grad.hip GROUP_ROWS)
N_CASES = [1, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1, 5 * W + 3]   # the last: 6 x 256 histogram entries, two scan rounds
K_CASES = [1, 2, 255, 256, 257, 65536]
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097]


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, f32).view(np.uint32)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev_u16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).cuda().view(torch.uint16)


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def gpu_group(lib, idx, K, poison=0xFF):
    n = idx.size
    nb = int(lib.gsr_vq_group_scratch_bytes(n, K))
    scr = torch.full((nb,), poison, dtype=torch.uint8, device="cuda")
    order = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    offsets = torch.full((K + 1,), -1, dtype=torch.int32, device="cuda")
    ind = dev_u16(idx)
    rc = lib.gsr_vq_group(n, K, _ptr(ind), _ptr(order), _ptr(offsets), _ptr(scr), nb, _stream())
    assert rc == 0, lib.gsr_last_error_string().decode()
    torch.cuda.synchronize()
    return u32(order), u32(offsets)


def check_group(lib, idx, K):
    idx = np.ascontiguousarray(idx, np.uint16)
    want = R.group(idx, K)
    got = gpu_group(lib, idx, K)
    assert np.array_equal(got[1], want[1]), (idx.size, K, "offsets")
    bad = np.flatnonzero(got[0] != want[0])
    assert bad.size == 0, (idx.size, K, bad[:8], got[0][bad[:8]], want[0][bad[:8]])
    return got


def gpu_grad(lib, g, order, offsets, K, padded=False, poison=0xFF, out_fill=float("nan")):
    """g (n, dim) host rows.  padded: the rows lie 48 floats apart behind a 3-float offset, every float between them a NaN."""
    n, dim = g.shape
    if padded:
        buf = np.full((n, 48), np.nan, f32)
        buf[:, 3:3 + dim] = g
        gd, stride, base = dev(buf), 48, 12
    else:
        gd, stride, base = dev(g), dim, 0
    nb = int(lib.gsr_vq_codebook_grad_scratch_bytes(n, K, dim))
    scr = torch.full((nb,), poison, dtype=torch.uint8, device="cuda")
    out = torch.full((K, dim), out_fill, device="cuda")
    od, fd = dev_u32(order), dev_u32(offsets)   # named: a temporary's memory would be handed to the next allocation
    rc = lib.gsr_vq_codebook_grad(n, K, dim, C.c_void_p(gd.data_ptr() + base), stride, _ptr(od), _ptr(fd), _ptr(out), _ptr(scr), nb,
                                  _stream())
    assert rc == 0, lib.gsr_last_error_string().decode()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def rows_for(idx, dim, seed):
    """Gradient-like rows: magnitudes over e^±3."""
    rng = np.random.default_rng(seed)
    n = idx.size
    return (rng.normal(size=(n, dim)) * np.exp(rng.uniform(-3, 3, size=(n, 1)))).astype(f32)


def check_grad(lib, g, idx, K, **kw):
    order, offsets = R.group(idx, K)
    want = R.codebook_grad(g, order, offsets, K)
    got = gpu_grad(lib, g, order, offsets, K, **kw)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (g.shape, K, kw, bad[:6].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:6]])
    return got


# ---- 1. group ----
@pytest.mark.parametrize("n", N_CASES)
def test_group_every_row_count(pkg, n):
    lib = pkg._lib.load()
    rng = np.random.default_rng(n)
    check_group(lib, rng.integers(0, 300, n), 300)
    check_group(lib, rng.integers(0, 5, n), 3)                 # indices >= K are read as K - 1


@pytest.mark.parametrize("K", K_CASES)
def test_group_every_code_count(pkg, K):
    lib = pkg._lib.load()
    rng = np.random.default_rng(K)
    n = 2 * W + 1
    check_group(lib, rng.integers(0, K, n), K)
    check_group(lib, rng.integers(0, min(2 * K, 65536), n), K)


def test_group_keys_that_differ_in_one_byte(pkg):
    lib = pkg._lib.load()
    rng = np.random.default_rng(5)
    keys = np.array([0x0001, 0x0100, 0x0101, 0x00FF, 0xFF00, 0xFFFF], np.uint16)
    check_group(lib, keys[rng.integers(0, 6, 2 * W + 1)], 65536)
    check_group(lib, keys[rng.integers(0, 2, 130) * 2], 65536)          # 0x0001 / 0x0101: the high byte alone
    check_group(lib, keys[rng.integers(0, 2, 130) + 1], 65536)          # 0x0100 / 0x0101: the low byte alone


def test_group_one_code_descending_and_two_runs(pkg):
    lib = pkg._lib.load()
    n = 3 * W + 5
    order, offsets = check_group(lib, np.full(n, 7), 9)
    assert np.array_equal(order, np.arange(n, dtype=np.uint32))       # all rows in one code: the identity
    assert offsets.tolist() == [0] * 8 + [n, n]
    order, offsets = check_group(lib, np.arange(n - 1, -1, -1), n)      # strictly descending: the reversal
    assert np.array_equal(order, np.arange(n - 1, -1, -1, dtype=np.uint32)) and np.array_equal(offsets, np.arange(n + 1))
    idx = np.random.default_rng(6).integers(0, 700, n).astype(np.uint16)
    a, b = gpu_group(lib, idx, 600, poison=0xFF), gpu_group(lib, idx, 600, poison=0x00)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 2. the gradient, bit for bit ----
@pytest.mark.parametrize("m", LENGTHS)
def test_grad_one_code_of_every_length(pkg, m):
    """One code of m rows between two empty codes; 4097 rows take three levels.  m = 0 is n = 0: GSR_OK, nothing written."""
    lib = pkg._lib.load()
    if m == 0:
        out = torch.full((3, 45), 5.0, device="cuda")
        assert lib.gsr_vq_codebook_grad(0, 3, 45, None, 45, None, None, _ptr(out), None, 0, _stream()) == 0
        torch.cuda.synchronize()
        assert bool((out == 5.0).all())
        sh = pkg.sh_codebook.SHCodebook(torch.zeros((3, 45), device="cuda"), torch.zeros(0, dtype=torch.uint16, device="cuda"), (0, 15, 3))
        got = pkg.sh_codebook.codebook_grad(torch.zeros((0, 15, 3), device="cuda"), sh, out=out)
        assert np.array_equal(bits(got), np.zeros((3, 45), np.uint32))
        return
    idx = np.full(m, 1, np.uint16)
    assert R.levels(m) == {1: 1, 2: 1, 63: 1, 64: 1, 65: 2, 127: 2, 128: 2, 129: 2, 4095: 2, 4096: 2, 4097: 3}[m]
    got = check_grad(lib, rows_for(idx, 45, m), idx, 3)
    assert not got[0].any() and not got[2].any() and not np.signbit(got[[0, 2]]).any()    # empty: +0.0


@pytest.fixture(scope="module")
def mixed():
    """Every length of LENGTHS in one call: code 2t + 1 has LENGTHS[t] rows, the even codes are empty; rows shuffled."""
    rng = np.random.default_rng(7)
    idx = np.concatenate([np.full(m, 2 * t + 1, np.uint16) for t, m in enumerate(LENGTHS)])
    idx = idx[rng.permutation(idx.size)]
    return idx, 2 * len(LENGTHS) + 1


@pytest.mark.parametrize("dim", [1, 2, 45, 48])
def test_grad_mixed_lengths_every_dim(pkg, mixed, dim):
    idx, K = mixed
    check_grad(pkg._lib.load(), rows_for(idx, dim, dim), idx, K)


def test_grad_strided_rows_and_two_poisons(pkg, mixed):
    """row_stride = 48 behind a 3-float offset, the skipped floats NaN: never read.  Two runs on other poisons: equal bits."""
    idx, K = mixed
    lib = pkg._lib.load()
    g = rows_for(idx, 45, 8)
    a = check_grad(lib, g, idx, K, padded=True)
    b = check_grad(lib, g, idx, K, poison=0x00, out_fill=1.0e30)
    assert np.array_equal(bits(a), bits(b))
    g2 = rows_for(idx, 2, 9)
    check_grad(lib, g2, idx, K, padded=True)


def test_grad_hot_code(pkg):
    """One code of 70 000 rows (1094 -> 18 -> 1 partial rows) beside six small ones; and within the derived bound of float64."""
    lib = pkg._lib.load()
    rng = np.random.default_rng(10)
    idx = np.concatenate([np.full(70_000, 3, np.uint16), rng.integers(0, 7, 500).astype(np.uint16)])
    idx = idx[rng.permutation(idx.size)]
    g = rows_for(idx, 45, 11)
    got = check_grad(lib, g, idx, 7).astype(np.float64)
    exact, mass = np.zeros((7, 45)), np.zeros((7, 45))
    np.add.at(exact, idx.astype(np.int64), g.astype(np.float64))
    np.add.at(mass, idx.astype(np.int64), np.abs(g.astype(np.float64)))
    assert (np.abs(got - exact) <= 2.0 ** -16 * mass).all()


def test_grad_65536_codes(pkg):
    lib = pkg._lib.load()
    idx = np.random.default_rng(12).integers(0, 65536, 70).astype(np.uint16)
    idx[:5] = 65535
    idx[5:8] = 0
    check_grad(lib, rows_for(idx, 45, 13), idx, 65536)


def test_grad_nan_inf_and_negative_zero_rows(pkg):
    lib = pkg._lib.load()
    rng = np.random.default_rng(14)
    idx = rng.integers(0, 4, 700).astype(np.uint16)
    idx[:200] = 2
    g = rows_for(idx, 45, 15)
    g[17] = np.nan
    g[300, 5] = np.inf
    g[301, 6] = -np.inf
    g[idx == 3] = -0.0                                                  # rows of -0.0: the sum is -0.0
    payload = np.array([0x7FC12345], np.uint32).view(f32)[0]
    idx = np.append(idx, 5).astype(np.uint16)                           # a code of ONE row: bits pass through
    g = np.vstack([g, np.full((1, 45), payload, f32)])
    g[-1, 1] = -0.0
    got = check_grad(lib, g, idx, 6)
    j = int(idx[17])
    assert np.isnan(got[j]).all()
    for other in set(range(4)) - {j, int(idx[300]), int(idx[301]), 3}:
        assert np.isfinite(got[other]).all()
    assert np.signbit(got[3]).all() and not got[3].any()
    assert bits(got[5])[0] == 0x7FC12345 and bits(got[5])[1] == 0x80000000 and not got[4].any()


# ---- 3. sh_codebook ----
def _sh(pkg, idx, K, dim=45, seed=0, shape=None):
    rng = np.random.default_rng(seed)
    cb = dev(rng.normal(size=(K, dim)).astype(f32))
    return pkg.sh_codebook.SHCodebook(cb, dev_u16(idx), shape or (idx.size, dim // 3, 3))


def test_codebook_grad_contiguous_and_strided_view(pkg, mixed):
    S = pkg.sh_codebook
    idx, K = mixed
    n = idx.size
    sh = _sh(pkg, idx, K)
    order, offsets = sh.groups()
    assert sh.groups()[0] is order                                     # cached
    want_o, want_f = R.group(idx, K)
    assert np.array_equal(u32(order), want_o) and np.array_equal(u32(offsets), want_f)
    vshs = torch.full((n, 16, 3), float("nan"), device="cuda")
    g = rows_for(idx, 45, 16)
    vshs[:, 1:, :] = dev(g).view(n, 15, 3)
    want = R.codebook_grad(g, want_o, want_f, K)
    view = vshs[:, 1:, :]
    assert not view.is_contiguous()
    assert np.array_equal(bits(S.codebook_grad(view, sh)), bits(want))                       # in place: the NaN column is not read
    assert np.array_equal(bits(S.codebook_grad(dev(g).view(n, 15, 3), sh)), bits(want))
    out = torch.full((K, 45), float("nan"), device="cuda")
    assert S.codebook_grad(dev(g), sh, out=out) is out and np.array_equal(bits(out), bits(want))
    # indices replaced: the groups are built again
    idx2 = np.roll(idx, 3)
    sh.indices = dev_u16(idx2)
    assert sh.groups()[0] is not order
    assert np.array_equal(bits(S.codebook_grad(dev(g), sh)), bits(R.codebook_grad(g, *R.group(idx2, K), K)))
    with pytest.raises(ValueError):
        S.codebook_grad(dev(g)[:, :44], sh)
    with pytest.raises(ValueError):
        S.codebook_grad(dev(g), sh, out=torch.zeros((K, 44), device="cuda"))


@pytest.fixture(scope="module")
def grid(pkg):
    """The 64-Gaussian grid scene at SH degree 3 with random features_rest, its render, and a K = 8 codebook of them."""
    model, cam = scenes.grid_scene_rgbdn()
    n = model["means"].shape[0]
    rest = (0.2 * np.random.default_rng(20).normal(size=(n, 15, 3))).astype(f32)
    camera = pkg.Camera(cam.width, cam.height, tuple(cam.focal))
    rast = pkg.rasterizer.GaussianRasterizer(cam.width, cam.height, mode="rgb", device="cuda:0")
    t = dict(means=dev(model["means"]), dc=dev(model["shs"]), opac=dev(model["opac"].reshape(-1, 1)), scales=dev(model["scales"]),
             rots=dev(model["rots"]))

    def forward(rest_t):
        shs = torch.cat([t["dc"], rest_t], dim=1).contiguous()
        return shs, rast.forward_raw(t["means"], shs, t["opac"], t["scales"], t["rots"], camera, 3, (0.0, 0.0, 0.0))

    target = forward(dev(rest))[1].clone()
    sh = pkg.sh_codebook.fit_sh_codebook(dev(rest), 8, iters=3)
    torch.cuda.synchronize()
    return t, camera, rast, forward, target, sh


def _l1_cotangent(img, target):
    leaf = img.detach().clone().requires_grad_(True)
    loss = (leaf - target).abs().mean()
    return loss.detach(), torch.autograd.grad(loss, leaf)[0].contiguous()


def _raw_grad(grid, rest_t):
    t, camera, rast, forward, target, sh = grid
    shs, img = forward(rest_t)
    loss, vpix = _l1_cotangent(img, target)
    vshs = rast.backward_raw(vpix, t["means"], shs, t["opac"], t["scales"], t["rots"], camera, 3, (0.0, 0.0, 0.0))[1]
    return loss, vshs


def test_autograd_path_equals_the_raw_chain(pkg, grid):
    S = pkg.sh_codebook
    t, camera, rast, forward, target, sh = grid
    cb = sh.codebook.clone().requires_grad_(True)
    rest = S.decode_features_rest(cb, sh)
    assert torch.equal(rest, sh.decode()) and rest.requires_grad
    shs = torch.cat([t["dc"], rest], dim=1)
    img = pkg.rasterizer.rasterize(t["means"], shs, t["opac"], t["scales"], t["rots"], rast=rast, camera=camera, sh_degree=3)
    loss = (img - target).abs().mean()
    loss.backward()
    torch.cuda.synchronize()
    raw_loss, vshs = _raw_grad(grid, sh.decode())
    want = S.codebook_grad(vshs[:, 1:, :], sh)
    assert torch.equal(loss.detach(), raw_loss)
    assert float(want.abs().max()) > 0 and torch.equal(cb.grad, want)
    assert np.array_equal(bits(want), bits(R.codebook_grad(vshs[:, 1:, :].reshape(-1, 45).cpu().numpy(), *map(u32, sh.groups()), 8)))


def test_fine_tuner_step_equals_the_steps_by_hand(pkg, mixed):
    S = pkg.sh_codebook
    idx, K = mixed
    a, b = _sh(pkg, idx, K, seed=21), _sh(pkg, idx, K, seed=21)
    tuner = S.SHCodebookFineTuner(a)
    assert tuner.codebook is a.codebook and tuner.optimizer.lr == 25e-4 / 20 and tuner.optimizer.eps == 1e-15
    opt = pkg.optim.Adam(b.codebook, 25e-4 / 20, eps=1e-15)
    for step in range(3):
        g = dev(rows_for(idx, 45, 30 + step) * f32(1e-3)).view(-1, 15, 3)
        tuner.step(g)
        opt.step(b.codebook, S.codebook_grad(g, b))
    torch.cuda.synchronize()
    assert tuner.optimizer.current_step == 3 and not torch.equal(a.codebook, _sh(pkg, idx, K, seed=21).codebook)
    assert torch.equal(a.codebook, b.codebook) and torch.equal(tuner.optimizer.mu, opt.mu) and torch.equal(tuner.optimizer.nu, opt.nu)
    assert torch.equal(tuner.features_rest(), b.decode())


def test_fine_tuning_lowers_the_loss(pkg, grid):
    """K = 8 codes for 64 Gaussians: the decoded render differs from the original; 40 steps of the code rows alone against the
    original render (backward_raw + SHCodebookFineTuner.step, lr 2e-3) must lower the L1.  Deterministic: the same figures in
    every run."""
    S = pkg.sh_codebook
    t, camera, rast, forward, target, fitted = grid
    sh = S.SHCodebook(fitted.codebook.clone(), fitted.indices, fitted.shape)
    tuner = S.SHCodebookFineTuner(sh, lr=2e-3)
    before = float(_raw_grad(grid, tuner.features_rest())[0])
    assert before > 0
    for _ in range(40):
        tuner.step(_raw_grad(grid, tuner.features_rest())[1][:, 1:, :])
    after = float(_raw_grad(grid, tuner.features_rest())[0])
    print(f"L1 against the original render: {before:.6f} before, {after:.6f} after 40 steps")
    assert after < before


def test_checkpoint_in_the_middle_of_a_run(pkg, mixed, tmp_path):
    """Two steps, save, load into a tuner built from other values, one more step: the uninterrupted run's bits."""
    S, CK = pkg.sh_codebook, pkg.checkpoint
    idx, K = mixed
    gs = [dev(rows_for(idx, 45, 40 + s) * f32(1e-3)) for s in range(3)]
    whole = S.SHCodebookFineTuner(_sh(pkg, idx, K, seed=22))
    for g in gs:
        whole.step(g)
    first = S.SHCodebookFineTuner(_sh(pkg, idx, K, seed=22))
    for g in gs[:2]:
        first.step(g)
    tensors, meta = {}, {}
    CK.write_sh_codebook(tensors, meta, "sh_codebook", first)
    CK.save_checkpoint(str(tmp_path / "mid.safetensors"), tensors, meta)
    resumed = S.SHCodebookFineTuner(_sh(pkg, np.zeros_like(idx), K, seed=23))
    resumed.sh.groups()                                                   # built for the other indices: must not survive the load
    CK.read_sh_codebook(resumed, CK.load_checkpoint(str(tmp_path / "mid.safetensors")), "sh_codebook")
    assert resumed.optimizer.current_step == 2 and resumed.codebook is resumed.sh.codebook
    resumed.step(gs[2])
    torch.cuda.synchronize()
    assert torch.equal(resumed.codebook, whole.codebook) and torch.equal(resumed.optimizer.mu, whole.optimizer.mu)
    assert torch.equal(resumed.optimizer.nu, whole.optimizer.nu) and resumed.optimizer.current_step == 3


# ---- 4. guarded arenas, error codes ----
def _guarded_calls(lib, P, tag):
    n, K, dim = 2 * W + 1, 257, 45
    rng = np.random.default_rng(50)
    idx = rng.integers(0, 300, n).astype(np.uint16)                     # some >= K
    idx[:900] = 11                                                      # a code of two levels
    g = rows_for(idx, dim, 51)
    want_o, want_f = R.group(idx, K)
    want = R.codebook_grad(g, want_o, want_f, K)
    I16, I32, U8 = torch.int16, torch.int32, torch.uint8
    padded = np.full((n, 48), np.nan, f32)
    padded[:, 3:] = g
    nbg, nbc = int(lib.gsr_vq_group_scratch_bytes(n, K)), int(lib.gsr_vq_codebook_grad_scratch_bytes(n, K, dim))
    ind = P.place("indices", idx.view(np.int16), guard=(0, K - 1))
    order = P.place("order", (n,), I32, guard=(0, n - 1))
    offsets = P.place("offsets", (K + 1,), I32, guard=(0, n))
    sg = P.place("group scratch", (nbg,), U8, align=16, role="scratch")
    rows, rows48 = P.place("g_rows", g), P.place("g_rows, stride 48", padded)
    out, out48, out_bad = P.place("g_codebook", (K, dim)), P.place("g_codebook, stride 48", (K, dim)), P.place("g_codebook, damaged", (K, dim))
    sc = P.place("grad scratch", (nbc,), U8, align=16, role="scratch")
    bad_o, bad_f = want_o.copy(), want_f.copy()
    bad_o[::5] = n + 7
    bad_o[3::11] = 0xFFFFFFFF
    bad_f[3], bad_f[10], bad_f[20], bad_f[21], bad_f[K] = n + 100, 0xFFFFFFFF, 2000, 5, 0
    order_bad = P.place("order, damaged", bad_o.view(np.int32), guard=(0, n - 1))
    offsets_bad = P.place("offsets, damaged", bad_f.view(np.int32), guard=(0, n))
    if P.skew == "worst":
        assert rows.data_ptr() % 16 == 4 and ind.data_ptr() % 16 == 2 and order.data_ptr() % 16 == 4 and sc.data_ptr() % 32 == 16
    for t in (order, offsets, sg, out, out48, out_bad, sc):
        t.view(-1).view(U8).fill_(0xFF)
    st = _stream()
    grad = lib.gsr_vq_codebook_grad
    rcs = [lib.gsr_vq_group(n, K, _ptr(ind), _ptr(order), _ptr(offsets), _ptr(sg), nbg, st),
           grad(n, K, dim, _ptr(rows), dim, _ptr(order), _ptr(offsets), _ptr(out), _ptr(sc), nbc, st),
           grad(n, K, dim, C.c_void_p(rows48.data_ptr() + 12), 48, _ptr(order), _ptr(offsets), _ptr(out48), _ptr(sc), nbc, st),
           grad(n, K, dim, _ptr(rows), dim, _ptr(order_bad), _ptr(offsets_bad), _ptr(out_bad), _ptr(sc), nbc, st),
           grad(n, K, dim, _ptr(rows), dim, _ptr(order_bad), _ptr(offsets), _ptr(out_bad), _ptr(sc), nbc, st)]
    assert rcs == [0] * 5, (tag, rcs, lib.gsr_last_error_string().decode())
    torch.cuda.synchronize()
    assert P.check() == [], (tag, P.check())
    P.assert_inputs_unchanged()
    assert np.array_equal(u32(order), want_o) and np.array_equal(u32(offsets), want_f), tag
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(bits(out48), bits(want)), tag


def test_entry_points_on_guarded_buffers(pkg):
    """n = 2049, K = 257, dim = 45 on the five placements: no guard word changes, the inputs are unchanged, poisoned outputs and
    scratch reach no result.  Under skew "worst" the floats and the uint32 arrays start at 4 mod 16, the indices at 2 mod 16,
    the scratch at 16 mod 32.  Two more calls read an `order` with entries >= n and `offsets` with entries > n, out of order
    and short of n: wrong numbers, no access outside the arrays.  The integer guards are in range for a row and a position."""
    lib = pkg._lib.load()
    for P in placements(1 << 22, "cuda"):
        _guarded_calls(lib, P, f"{P.skew}/{P.fill}")


def test_error_codes(pkg):
    L = pkg._lib
    lib, bad, st = L.load(), L.GSR_E_INVALID_ARG, _stream()
    n, K, dim = 65, 33, 9
    idx = np.random.default_rng(60).integers(0, K, n).astype(np.uint16)
    ind = dev_u16(idx)
    order, offsets = torch.zeros(n + 1, dtype=torch.int32, device="cuda"), torch.zeros(K + 2, dtype=torch.int32, device="cuda")
    nbg, nbc = int(lib.gsr_vq_group_scratch_bytes(n, K)), int(lib.gsr_vq_codebook_grad_scratch_bytes(n, K, dim))
    sg, sc = torch.zeros(nbg + 16, dtype=torch.uint8, device="cuda"), torch.zeros(nbc + 16, dtype=torch.uint8, device="cuda")
    g, out = dev(rows_for(idx, dim, 61)), torch.zeros((K, dim), device="cuda")

    def group(n=n, K=K, ind=ind.data_ptr(), order=order.data_ptr(), off=offsets.data_ptr(), scr=sg.data_ptr(), nb=nbg):
        return lib.gsr_vq_group(n, K, ind, order, off, scr, nb, st)
    assert group() == 0
    for kw in (dict(n=-1), dict(n=1 << 24), dict(K=0), dict(K=65537), dict(ind=None), dict(order=None), dict(off=None), dict(scr=None),
               dict(nb=nbg - 1), dict(scr=sg.data_ptr() + 8), dict(ind=ind.data_ptr() + 1), dict(order=order.data_ptr() + 2),
               dict(off=offsets.data_ptr() + 1)):
        assert group(**kw) == bad, kw
    assert group(n=0, ind=None, order=None, off=None, scr=None, nb=0) == 0

    def grad(n=n, K=K, dim=dim, g=g.data_ptr(), stride=dim, order=order.data_ptr(), off=offsets.data_ptr(), out=out.data_ptr(),
             scr=sc.data_ptr(), nb=nbc):
        return lib.gsr_vq_codebook_grad(n, K, dim, g, stride, order, off, out, scr, nb, st)
    assert grad() == 0
    for kw in (dict(n=-1), dict(n=1 << 24), dict(K=0), dict(K=65537), dict(dim=0), dict(dim=49), dict(stride=dim - 1), dict(g=None),
               dict(order=None), dict(off=None), dict(out=None), dict(scr=None), dict(nb=nbc - 1), dict(scr=sc.data_ptr() + 8),
               dict(g=g.data_ptr() + 2), dict(out=out.data_ptr() + 1), dict(order=order.data_ptr() + 2), dict(off=offsets.data_ptr() + 2)):
        assert grad(**kw) == bad, kw
    assert grad(n=0, g=None, order=None, off=None, out=None, scr=None, nb=0) == 0
    torch.cuda.synchronize()
    want = R.codebook_grad(g.cpu().numpy(), *R.group(idx, K), K)
    assert np.array_equal(bits(out), bits(want))
    S = pkg.sh_codebook
    with pytest.raises(ValueError):
        S.codebook_grad(torch.zeros((n, dim), device="cuda", dtype=torch.float64), _sh(pkg, idx, K, dim=dim))
    with pytest.raises(ValueError):
        S.codebook_grad(torch.zeros((n + 1, dim), device="cuda"), _sh(pkg, idx, K, dim=dim))
