"""-m gpu: the SH codebook k-means on the MI355X (csrc/vq.hip through gsr_vq_* and sh_codebook); every test fails on a build without the feature (no sh_codebook in the package, no gsr_vq_* in the library).
  1. assign against the fp32 restatement of tests/vq_ref.py — indices, err bits and `changed` — at every n, K and dim at which
     the kernel takes another path: the 32-wide tiles, the workgroup's 512 rows, the 256-code LDS chunk, the padded columns;
  2. ties (a code duplicated in another register, half-wave, tile and chunk; duplicate points): the lowest index wins;
  3. hand rows: a NaN row, ±Inf, subnormals, a NaN code; two runs;
  4. accumulate and update against numpy int64: one hot code with weight 255, clamping, an empty code, NULL weights, arrays
     accumulated into;  5. decode with an index >= K;
  6. fit_sh_codebook against the restatement's chain, the lossless round trip and its render;
  7. the five entry points on guarded arenas, the error codes with device pointers.
Every comparison is array_equal, on bits or integers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import scenes
import vq_ref as R
from guarded import placements
from hip_helpers import dev
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu
f32 = np.float32
WG, CH = 512, 256   # rows per workgroup, codes per LDS chunk (csrc/vq.hip)
N_CASES = [1, 31, 32, 33, 63, 64, 65, WG - 1, WG, WG + 1, 2 * WG + 1]
K_CASES = [1, 2, 31, 32, 33, 64, 65, 100, CH - 1, CH, CH + 1]
DIM_CASES = [1, 2, 9, 24, 45, 48]


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, f32).view(np.int32)


def u16(t):
    """A device uint16 tensor as a numpy uint16 array."""
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def dev_u16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).cuda().view(torch.uint16)


@functools.lru_cache(maxsize=None)
def case(n, K, dim, seed=0):
    """Rows, a codebook drawn from near the rows (so that codes compete), a previous assignment; and the restatement's answer."""
    rng = np.random.default_rng(1000 * seed + 7 * n + 13 * K + dim)
    x = rng.normal(size=(n, dim)).astype(f32)
    cb = (x[rng.integers(0, n, K)] + 0.3 * rng.normal(size=(K, dim))).astype(f32)
    prev = rng.integers(0, K, n).astype(np.uint16)
    idx, err, _ = R.assign(x, cb)
    prev[::3] = idx[::3]
    return x, cb, prev, idx, err, int(np.count_nonzero(idx != prev))


def gpu_assign(lib, x, cb, prev=None, want_err=True, want_changed=True, in_place=False):
    n, dim = x.shape
    K = cb.shape[0]
    xd, cd = dev(x), dev(cb)
    nb = int(lib.gsr_vq_scratch_bytes(n, K, dim))
    scr = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    idx = torch.full((n,), -1, dtype=torch.int16, device="cuda").view(torch.uint16)
    pd = None if prev is None else dev_u16(prev)
    if in_place:
        idx = pd
    err = torch.full((n,), float("nan"), device="cuda") if want_err else None
    ch = torch.full((1,), -1, dtype=torch.int32, device="cuda") if want_changed else None
    rc = lib.gsr_vq_assign(n, K, dim, _ptr(xd), _ptr(cd), _ptr(pd), _ptr(idx), _ptr(err), _ptr(ch), _ptr(scr), nb, _stream())
    assert rc == 0, lib.gsr_last_error_string().decode()
    torch.cuda.synchronize()
    return u16(idx), None if err is None else err.cpu().numpy(), None if ch is None else int(ch.item()) & 0xFFFFFFFF


def check_assign(lib, n, K, dim):
    x, cb, prev, idx, err, changed = case(n, K, dim)
    got = gpu_assign(lib, x, cb, prev)
    bad = np.flatnonzero(got[0] != idx)
    assert bad.size == 0, ((n, K, dim), bad[:8], got[0][bad[:8]], idx[bad[:8]])
    assert np.array_equal(bits(got[1]), bits(err)), (n, K, dim)
    assert got[2] == changed, ((n, K, dim), got[2], changed)
    return got


# ---- 1. assign, bit for bit ----
@pytest.mark.parametrize("n", N_CASES)
def test_assign_every_row_count(pkg, n):
    lib = pkg._lib.load()
    check_assign(lib, n, 100, 45)
    check_assign(lib, n, CH + 1, 9)


@pytest.mark.parametrize("K", K_CASES)
def test_assign_every_code_count(pkg, K):
    lib = pkg._lib.load()
    check_assign(lib, 65, K, 45)
    check_assign(lib, WG + 1, K, 24)


@pytest.mark.parametrize("dim", DIM_CASES)
def test_assign_every_dim(pkg, dim):
    """The odd-dim pad (1, 9, 45), the columns padded to a multiple of eight, the largest dim; prev NULL, prev == indices."""
    lib = pkg._lib.load()
    check_assign(lib, 33, 33, dim)
    got = check_assign(lib, WG + 1, CH + 1, dim)
    x, cb, prev, idx, err, changed = case(WG + 1, CH + 1, dim)
    none = gpu_assign(lib, x, cb, None)
    assert np.array_equal(none[0], idx) and none[2] == WG + 1            # prev NULL: every row counts
    inpl = gpu_assign(lib, x, cb, prev, in_place=True)
    assert np.array_equal(inpl[0], idx) and inpl[2] == changed            # prev is indices itself
    bare = gpu_assign(lib, x, cb, None, want_err=False, want_changed=False)
    assert np.array_equal(bare[0], got[0])


def test_assign_65536_codes(pkg):
    check_assign(pkg._lib.load(), 70, 65536, 9)


# ---- 2. ties ----
def test_ties_take_the_lowest_index(pkg):
    """K = 700 (three chunks), dim 45.  The code at j is duplicated at j + 1, j + 4, j + 8, j + 32 and j + 256 — another
    register of the lane, the other half-wave, another register group, another tile, another chunk — for j at the start of a
    tile, in its middle, and where the copies cross a tile and a chunk boundary.  Every point IS one of those codes (and each
    twice: duplicate points), so the copies tie for the maximum exactly."""
    lib = pkg._lib.load()
    rng = np.random.default_rng(5)
    K, dim = 700, 45
    cb = rng.normal(size=(K, dim)).astype(f32)
    groups = []
    for j, offs in ((0, (1, 4, 8, 32, 256)), (40, (1,)), (50, (4,)), (77, (8,)), (100, (32,)), (130, (256,)), (250, (1, 4, 8, 32, 256)),
                    (300, (32, 256)), (420, (4, 256))):
        for o in offs:
            cb[j + o] = cb[j]
        groups.append(j)
    x = np.repeat(cb[groups], 2, axis=0)
    x = np.concatenate([x, rng.normal(size=(40, dim)).astype(f32)])
    idx, err, _ = R.assign(x, cb)
    assert idx[:2 * len(groups)].tolist() == [j for j in groups for _ in range(2)]   # the restatement takes the lowest
    got = gpu_assign(lib, x, cb)
    assert np.array_equal(got[0], idx) and np.array_equal(bits(got[1]), bits(err))
    # the whole codebook one row: index 0 for everybody
    same = np.tile(cb[:1], (CH + 40, 1))
    assert not gpu_assign(lib, x, same)[0].any()


# ---- 3. hand rows ----
def test_hand_rows(pkg):
    """Rows: NaN in one column (every t is NaN: index 0), +Inf and -Inf columns, subnormals, an ordinary row, a zero row.
    Codes: ordinary ones, one of NaN (never chosen), one of subnormals, one with an Inf."""
    lib = pkg._lib.load()
    rng = np.random.default_rng(6)
    dim, K = 9, 40
    cb = rng.normal(size=(K, dim)).astype(f32)
    cb[0] = np.nan                      # never chosen, though it is the lowest index
    cb[7] = f32(1e-41)                  # subnormal
    cb[9, 2] = np.inf
    x = rng.normal(size=(12, dim)).astype(f32)
    x[0, 3] = np.nan
    x[1, 0] = np.inf
    x[2, 0] = -np.inf
    x[3, 2] = np.inf                    # meets the Inf of code 9: Inf - Inf/… whatever the chain says
    x[4] = f32(3e-42)
    x[5] = 0.0
    x[6] = -cb[9]
    idx, err, _ = R.assign(x, cb)
    assert idx[0] == 0 and (idx[1:] != 0).all()
    a, b = gpu_assign(lib, x, cb), gpu_assign(lib, x, cb)
    assert np.array_equal(a[0], idx), (a[0], idx)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2] == 12
    nan = np.isnan(err)
    assert np.array_equal(np.isnan(a[1]), nan) and np.array_equal(bits(a[1])[~nan], bits(err)[~nan])
    # a codebook of NaN only: index 0 everywhere
    assert not gpu_assign(lib, x, np.full((70, dim), np.nan, f32))[0].any()


# ---- 4. accumulate and update ----
def gpu_accumulate(lib, x, idx, K, wq=None, sums=None, wsum=None):
    n, dim = x.shape
    sums = torch.zeros((K, dim), dtype=torch.int64, device="cuda") if sums is None else sums
    wsum = torch.zeros(K, dtype=torch.int64, device="cuda") if wsum is None else wsum
    wd = None if wq is None else torch.from_numpy(np.ascontiguousarray(wq, np.uint8)).cuda()
    xd, idd = dev(x), dev_u16(idx)   # named: a temporary's memory would be handed to the next allocation
    rc = lib.gsr_vq_accumulate(n, K, dim, _ptr(xd), _ptr(idd), _ptr(wd), _ptr(sums), _ptr(wsum), _stream())
    assert rc == 0, lib.gsr_last_error_string().decode()
    torch.cuda.synchronize()
    return sums, wsum


def gpu_update(lib, cb, sums, wsum):
    K, dim = cb.shape
    cd = dev(cb)
    empty = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    assert lib.gsr_vq_update(K, dim, _ptr(sums), _ptr(wsum), _ptr(cd), _ptr(empty), _stream()) == 0
    torch.cuda.synchronize()
    return cd.cpu().numpy(), int(empty.item())


def test_accumulate_one_hot_code_at_weight_255(pkg):
    """70 000 rows, ALL on code 3 of 5, weight 255, values at ±128, beyond (clamped), NaN (0) and ordinary: against numpy
    int64.  Code 0, 1, 2, 4 stay empty: their rows keep their bits, `empty` counts 4."""
    lib = pkg._lib.load()
    rng = np.random.default_rng(7)
    n, K, dim = 70_000, 5, 45
    x = (rng.normal(size=(n, dim)) * 40).astype(f32)
    x[:, 0], x[:, 1], x[:, 2], x[:, 3], x[::7, 4] = 128.0, -128.0, 1e30, -np.inf, np.nan
    idx = np.full(n, 3, np.uint16)
    wq = np.full(n, 255, np.uint8)
    want_s, want_w = R.accumulate(x, idx, K, wq)
    assert want_s[3, 0] == 255 * n * (1 << 31) and want_s[3, 3] == -255 * n * (1 << 31)
    sums, wsum = gpu_accumulate(lib, x, idx, K, wq)
    assert np.array_equal(sums.cpu().numpy(), want_s) and np.array_equal(wsum.cpu().numpy().view(np.uint64), want_w)
    cb = rng.normal(size=(K, dim)).astype(f32)
    want_c, want_e = R.update(cb, want_s, want_w)
    got_c, got_e = gpu_update(lib, cb, sums, wsum)
    assert got_e == want_e == 4 and np.array_equal(bits(got_c), bits(want_c))
    assert np.array_equal(bits(got_c[[0, 1, 2, 4]]), bits(cb[[0, 1, 2, 4]])) and got_c[3, 0] == 128.0 and got_c[3, 3] == -128.0


def test_accumulate_weights_runs_and_accumulation(pkg):
    """n = 1025 rows over K = 70 codes (one of them unused) with random weights, rows sorted by code in one half (long runs of
    equal codes within a wave) and shuffled in the other; NULL weights == all-ones weights; a second call adds to the first."""
    lib = pkg._lib.load()
    rng = np.random.default_rng(8)
    n, K, dim = 1025, 70, 45
    x = rng.normal(size=(n, dim)).astype(f32)
    idx = rng.integers(0, K - 1, n).astype(np.uint16)   # code 69 is empty
    idx[:512] = np.sort(idx[:512])
    wq = rng.integers(0, 256, n).astype(np.uint8)        # weight 0 among them
    want_s, want_w = R.accumulate(x, idx, K, wq)
    sums, wsum = gpu_accumulate(lib, x, idx, K, wq)
    assert np.array_equal(sums.cpu().numpy(), want_s) and np.array_equal(wsum.cpu().numpy().view(np.uint64), want_w)
    ones = gpu_accumulate(lib, x, idx, K, np.ones(n, np.uint8))
    null = gpu_accumulate(lib, x, idx, K, None)
    assert torch.equal(ones[0], null[0]) and torch.equal(ones[1], null[1])
    assert np.array_equal(null[0].cpu().numpy(), R.accumulate(x, idx, K)[0])
    # accumulated into, not cleared
    sums2, wsum2 = gpu_accumulate(lib, x, idx, K, None, sums, wsum)
    assert np.array_equal(sums2.cpu().numpy(), want_s + null[0].cpu().numpy()) and np.array_equal(wsum2.cpu().numpy(), want_w.view(np.int64) + null[1].cpu().numpy())
    cb = rng.normal(size=(K, dim)).astype(f32)
    want_c, want_e = R.update(cb, want_s + null[0].cpu().numpy(), (want_w.view(np.int64) + null[1].cpu().numpy()).view(np.uint64))
    got_c, got_e = gpu_update(lib, cb, sums2, wsum2)
    assert got_e == want_e and want_e >= 1 and np.array_equal(bits(got_c), bits(want_c))
    # other row lengths: the lanes past dim, the weight lane
    wide = np.concatenate([x, x[:, :3]], axis=1)
    for d in (1, 2, 48):
        xd = np.ascontiguousarray(wide[:, :d])
        s, w = gpu_accumulate(lib, xd, idx, K, wq)
        ws, ww = R.accumulate(xd, idx, K, wq)
        assert np.array_equal(s.cpu().numpy(), ws) and np.array_equal(w.cpu().numpy().view(np.uint64), ww), d


# ---- 5. decode ----
def test_decode_clamps_an_index_past_the_codebook(pkg):
    lib = pkg._lib.load()
    rng = np.random.default_rng(9)
    n, K, dim = 1027, 70, 45
    cb = rng.normal(size=(K, dim)).astype(f32)
    idx = rng.integers(0, K, n).astype(np.uint16)
    idx[5], idx[6], idx[n - 1] = K, 65535, K - 1
    out = torch.full((n, dim), float("nan"), device="cuda")
    cd, idd = dev(cb), dev_u16(idx)
    assert lib.gsr_vq_decode(n, K, dim, _ptr(cd), _ptr(idd), _ptr(out), _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), bits(cb[np.minimum(idx.astype(np.int64), K - 1)]))


# ---- 6. fit_sh_codebook ----
def test_fit_is_the_restatements_chain(pkg):
    """Five iterations at n = 3000, K = 70, dim = 45: codebook bits, indices and history equal the restatement's chain."""
    S = pkg.sh_codebook
    rng = np.random.default_rng(10)
    fr = (rng.normal(size=(3000, 15, 3)) * rng.uniform(0.05, 1.0, size=(1, 15, 1))).astype(f32)
    want_c, want_i, want_h = R.fit(fr.reshape(3000, 45), 70, 5)
    got = S.fit_sh_codebook(dev(fr), 70, iters=5)
    assert got.indices.dtype == torch.uint16 and got.history.dtype == torch.uint32 and tuple(got.history.shape) == (5, 2)
    assert np.array_equal(got.history.view(torch.int32).numpy().view(np.uint32), want_h), (got.history, want_h)
    assert np.array_equal(u16(got.indices), want_i)
    assert np.array_equal(bits(got.codebook), bits(want_c))
    assert want_h[0, 0] == 3000 and 0 < want_h[-1, 0] < want_h[1, 0]
    assert got.nbytes == 70 * 45 * 4 + 3000 * 2 and tuple(got.decode().shape) == (3000, 15, 3)
    assert np.array_equal(bits(got.decode()).reshape(3000, 45), bits(want_c[want_i.astype(np.int64)]))


def test_fit_with_weights_and_early_stop(pkg):
    S = pkg.sh_codebook
    rng = np.random.default_rng(11)
    x = rng.normal(size=(1100, 9)).astype(f32)
    score = rng.uniform(size=1100) ** 4
    score[::5] = 0.0
    wq = S.weights_from_scores(torch.from_numpy(score).cuda())
    assert np.array_equal(wq.cpu().numpy(), R.weights_from_scores(score)) and int(wq.min()) == 1 and int(wq.max()) == 255
    want_c, want_i, want_h = R.fit(x, 33, 2, wq=wq.cpu().numpy())
    got = S.fit_sh_codebook(dev(x), 33, iters=2, weights=wq)
    assert np.array_equal(bits(got.codebook), bits(want_c)) and np.array_equal(u16(got.indices), want_i)
    assert np.array_equal(got.history.view(torch.int32).numpy().view(np.uint32), want_h)
    # separated clusters settle: the early stop cuts the history where nothing changed, with the same codebook
    cl = (np.repeat(np.arange(6)[:, None] * 10.0, 50, axis=0) + 0.1 * rng.normal(size=(300, 9))).astype(f32)
    full = S.fit_sh_codebook(dev(cl), 6, iters=6)
    early = S.fit_sh_codebook(dev(cl), 6, iters=6, stop_when_unchanged=True)
    h = full.history.view(torch.int32).numpy()
    assert h[0, 0] == 300 and (h[2:, 0] == 0).all()
    assert early.history.shape[0] < 6 and torch.equal(early.codebook, full.codebook) and torch.equal(early.indices.view(torch.int16), full.indices.view(torch.int16))


@pytest.fixture(scope="module")
def lossless(pkg):
    """The 64-Gaussian grid scene of tests/scenes.py at SH degree 3, its features_rest drawn from 7 distinct rows; the codebook
    with K = 7 and init = those rows, zero iterations and two.  The rows are multiples of 2^-24 (what an update stores: the
    sums are fixed point), so the two iterations reproduce them as well."""
    S = pkg.sh_codebook
    model, cam = scenes.grid_scene_rgbdn()
    n = model["means"].shape[0]
    rng = np.random.default_rng(12)
    distinct = (np.rint(0.2 * rng.normal(size=(7, 15, 3)) * 2.0 ** 24) / 2.0 ** 24).astype(f32)
    pick = rng.integers(0, 7, n)
    pick[:7] = np.arange(7)
    rest = distinct[pick]
    fits = [S.fit_sh_codebook(dev(rest), 7, iters=it, init=dev(distinct.reshape(7, 45))) for it in (0, 2)]
    return model, cam, rest, pick, fits


def test_lossless_round_trip(pkg, lossless):
    model, cam, rest, pick, fits = lossless
    for cbk in fits:
        assert np.array_equal(u16(cbk.indices), pick.astype(np.uint16))
        assert np.array_equal(bits(cbk.decode()), bits(rest)) and tuple(cbk.decode().shape) == rest.shape
    assert fits[1].history.view(torch.int32)[:, 1].tolist() == [0, 0] and fits[1].history.view(torch.int32)[:, 0].tolist() == [64, 0]
    # the one-call form, on rows off the 2^-24 grid: without an update the codes are the rows as given
    off = (rest * f32(1.0 / 3.0)).astype(f32)
    one = pkg.sh_codebook.compress_features_rest(dev(off), 7, iters=0, init=dev(off[:7].reshape(7, 45)))
    assert np.array_equal(bits(one.decode()), bits(off)) and np.array_equal(u16(one.indices), pick.astype(np.uint16))


def test_lossless_render_is_the_originals(pkg, lossless):
    model, cam, rest, pick, fits = lossless
    camera = pkg.Camera(cam.width, cam.height, tuple(cam.focal))
    rast = pkg.rasterizer.GaussianRasterizer(cam.width, cam.height, mode="rgb", device="cuda:0")

    def render(rest_t):
        shs = torch.cat([dev(model["shs"]), rest_t], dim=1).contiguous()
        img = rast.forward_raw(dev(model["means"]), shs, dev(model["opac"].reshape(-1, 1)), dev(model["scales"]), dev(model["rots"]),
                               camera, 3, (0.0, 0.0, 0.0)).clone()
        torch.cuda.synchronize()
        return img

    ref = render(dev(rest))
    assert float(ref.abs().max()) > 0.1
    assert torch.equal(render(fits[1].decode()), ref)
    assert not torch.equal(render(torch.zeros_like(dev(rest))), ref)   # the scene sees features_rest


# ---- 7. guarded arenas, error codes ----
def _guarded_calls(lib, P, tag):
    n, K, dim = 2 * WG + 1, CH + 1, 45
    x, cb, prev, idx, err, changed = case(n, K, dim)
    I16, I64, U8 = torch.int16, torch.int64, torch.uint8
    rng = np.random.default_rng(13)
    wq_h = rng.integers(0, 256, n).astype(np.uint8)
    nb = int(lib.gsr_vq_scratch_bytes(n, K, dim))
    rows, code = P.place("rows", x), P.place("codebook", cb)
    pv = P.place("prev", prev.view(np.int16), guard=(0, K - 1))
    ind = P.place("indices", (n,), I16, guard=(0, K - 1))
    er, ch = P.place("err", (n,)), P.place("changed", (1,), torch.int32)
    scr = P.place("scratch", (nb,), U8, align=16, role="scratch")
    inpl = P.place("indices in place of prev", prev.view(np.int16), role="inout", guard=(0, K - 1))
    wq = P.place("wq", wq_h)
    sums, wsum = P.place("sums", (K, dim), I64), P.place("wsum", (K,), I64)
    cb2, empty = P.place("codebook, updated", cb, role="inout"), P.place("empty", (1,), torch.int32)
    dec = P.place("decoded", (n, dim))
    if P.skew == "worst":
        assert rows.data_ptr() % 16 == 4 and code.data_ptr() % 16 == 4 and ind.data_ptr() % 16 == 2 and scr.data_ptr() % 32 == 16
        assert sums.data_ptr() % 16 == 8 and wq.data_ptr() % 2 == 1
    for t in (ind, er, ch, scr, empty, dec):
        t.view(-1).view(U8).fill_(0xFF)
    st = _stream()
    rcs = [lib.gsr_vq_assign(n, K, dim, _ptr(rows), _ptr(code), _ptr(pv), _ptr(ind), _ptr(er), _ptr(ch), _ptr(scr), nb, st),
           lib.gsr_vq_assign(n, K, dim, _ptr(rows), _ptr(code), _ptr(inpl), _ptr(inpl), None, None, _ptr(scr), nb, st),
           lib.gsr_vq_accumulate(n, K, dim, _ptr(rows), _ptr(ind), _ptr(wq), _ptr(sums), _ptr(wsum), st),
           lib.gsr_vq_update(K, dim, _ptr(sums), _ptr(wsum), _ptr(cb2), _ptr(empty), st),
           lib.gsr_vq_decode(n, K, dim, _ptr(cb2), _ptr(ind), _ptr(dec), st)]
    assert rcs == [0] * 5, (tag, rcs, lib.gsr_last_error_string().decode())
    torch.cuda.synchronize()
    assert P.check() == [], (tag, P.check())
    P.assert_inputs_unchanged()
    assert np.array_equal(ind.cpu().numpy().view(np.uint16), idx) and np.array_equal(inpl.cpu().numpy().view(np.uint16), idx), tag
    assert np.array_equal(bits(er), bits(err)) and int(ch.item()) == changed, tag
    ws, ww = R.accumulate(x, idx, K, wq_h)
    assert np.array_equal(sums.cpu().numpy(), ws) and np.array_equal(wsum.cpu().numpy().view(np.uint64), ww), tag
    wc, we = R.update(cb, ws, ww)
    assert np.array_equal(bits(cb2), bits(wc)) and int(empty.item()) == we, tag
    assert np.array_equal(bits(dec), bits(wc[idx.astype(np.int64)])), tag


def test_entry_points_on_guarded_buffers(pkg):
    """n = 1025, K = 257, dim = 45 on the five placements: no guard word changes, the inputs are unchanged, poisoned outputs
    and scratch reach no result, the restatement's bits everywhere.  Under skew "worst" the float arrays start at 4 mod 16, the
    indices at 2 mod 16, the sums at 8 mod 16, the scratch at 16 mod 32: the entry points may not ask for more.  The integer
    guards are in range for an index."""
    lib = pkg._lib.load()
    for P in placements(1 << 21, "cuda"):
        _guarded_calls(lib, P, f"{P.skew}/{P.fill}")


def test_error_codes(pkg):
    L = pkg._lib
    lib, bad, st = L.load(), L.GSR_E_INVALID_ARG, _stream()
    n, K, dim = 65, 33, 9
    x, cb, prev, idx, err, changed = case(n, K, dim)
    xd, cd, pd = dev(x), dev(cb), dev_u16(prev)
    nb = int(lib.gsr_vq_scratch_bytes(n, K, dim))
    assert nb == (16 * 288 + 256) * 4   # one chunk, dim 9 padded to 16 columns
    scr = torch.zeros(nb + 16, dtype=torch.uint8, device="cuda")
    ind = torch.full((n + 1,), 77, dtype=torch.int16, device="cuda")
    sums, wsum = torch.zeros((K, dim), dtype=torch.int64, device="cuda"), torch.zeros(K + 1, dtype=torch.int64, device="cuda")
    out = torch.zeros((n, dim), device="cuda")

    def assign(n=n, K=K, dim=dim, rows=xd, code=cd, prev=pd.data_ptr(), ind=ind.data_ptr(), err=None, ch=None, scr=scr.data_ptr(), nb=nb):
        return lib.gsr_vq_assign(n, K, dim, _ptr(rows), _ptr(code), prev, ind, err, ch, scr, nb, st)
    assert assign() == 0
    for kw in (dict(n=-1), dict(n=1 << 24), dict(K=0), dict(K=65537), dict(dim=0), dict(dim=49), dict(rows=None), dict(code=None),
               dict(ind=None), dict(scr=None), dict(nb=nb - 1), dict(scr=scr.data_ptr() + 8), dict(ind=ind.data_ptr() + 1),
               dict(prev=pd.data_ptr() + 1), dict(ch=wsum.data_ptr() + 2)):
        assert assign(**kw) == bad, kw
    assert assign(n=0, rows=None, code=None, ind=None, scr=None, nb=0) == 0
    acc = lib.gsr_vq_accumulate
    assert acc(n, K, dim, _ptr(xd), ind.data_ptr(), None, _ptr(sums), _ptr(wsum), st) == 0
    assert acc(n, K, dim, None, ind.data_ptr(), None, _ptr(sums), _ptr(wsum), st) == bad
    assert acc(n, K, dim, _ptr(xd), None, None, _ptr(sums), _ptr(wsum), st) == bad
    assert acc(n, K, dim, _ptr(xd), ind.data_ptr(), None, None, _ptr(wsum), st) == bad
    assert acc(n, K, dim, _ptr(xd), ind.data_ptr(), None, _ptr(sums), None, st) == bad
    assert acc(n, K, dim, _ptr(xd), ind.data_ptr(), None, sums.data_ptr() + 4, _ptr(wsum), st) == bad
    assert acc(n, K, 49, _ptr(xd), ind.data_ptr(), None, _ptr(sums), _ptr(wsum), st) == bad
    assert acc(0, K, dim, None, None, None, None, None, st) == 0
    upd = lib.gsr_vq_update
    assert upd(K, dim, _ptr(sums), _ptr(wsum), _ptr(cd), None, st) == 0
    assert upd(K, dim, None, _ptr(wsum), _ptr(cd), None, st) == bad and upd(K, dim, _ptr(sums), None, _ptr(cd), None, st) == bad
    assert upd(K, dim, _ptr(sums), _ptr(wsum), None, None, st) == bad and upd(0, dim, _ptr(sums), _ptr(wsum), _ptr(cd), None, st) == bad
    assert upd(K, dim, _ptr(sums), wsum.data_ptr() + 4, _ptr(cd), None, st) == bad
    decode = lib.gsr_vq_decode
    assert decode(n, K, dim, _ptr(cd), ind.data_ptr(), _ptr(out), st) == 0
    assert decode(n, K, dim, None, ind.data_ptr(), _ptr(out), st) == bad and decode(n, K, dim, _ptr(cd), None, _ptr(out), st) == bad
    assert decode(n, K, dim, _ptr(cd), ind.data_ptr(), None, st) == bad and decode(n, 65537, dim, _ptr(cd), ind.data_ptr(), _ptr(out), st) == bad
    assert decode(0, K, dim, None, None, None, st) == 0
    torch.cuda.synchronize()
    S = pkg.sh_codebook
    with pytest.raises(ValueError):
        S.fit_sh_codebook(xd, 0)
    with pytest.raises(ValueError):
        S.fit_sh_codebook(xd, 4, weights=torch.ones(n, device="cuda"))
    with pytest.raises(ValueError):
        S.fit_sh_codebook(xd, 4, init=torch.zeros((4, dim + 1), device="cuda"))
    with pytest.raises(ValueError):
        S.fit_sh_codebook(torch.zeros((5, 49), device="cuda"), 4)
