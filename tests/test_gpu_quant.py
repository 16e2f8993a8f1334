"""The quantised model container on the device (csrc/quant.hip) against the numpy restatement tests/quant_ref.py:
every comparison is array_equal on integers or on float bits.

Sizes: the range kernels take 1024 rows per workgroup in the one-block form and one block per workgroup otherwise, the other
kernels 256 rows per workgroup and 64 per wave — so n runs over 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, and 70 000
for the integer atomics across 69 workgroups.  cols 1, 3, 4 take the row-per-lane path (4: the vector accesses), 45 and 48 the
column-per-lane path; bits 1, 8 / 9, 16 the two code widths."""
import ctypes as C

import numpy as np
import pytest
import torch

import quant_ref as R
import scenes
from guarded import placements
from hip_helpers import dev
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN, INF = f32(np.nan), f32(np.inf)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, f32).view(np.uint32)


def host_codes(t):
    t = t.detach().cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype in (torch.uint16, torch.int16) else t.numpy()


def dev_codes(a, nbits):
    a = np.ascontiguousarray(a)
    if nbits <= 8:
        return torch.from_numpy(a.astype(np.uint8)).cuda()
    return torch.from_numpy(a.astype(np.uint16).view(np.int16)).cuda()      # int16 storage of the uint16 words


def ok(lib, rc):
    assert rc == 0, lib.gsr_last_error_string().decode()


def poisoned(shape, dtype, poison):
    """A device tensor whose every byte is 0xFF ("nan": NaN floats, the last code) or 0x7F ("big": 3.4e38, codes 127 / 32639)."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(-1).view(torch.uint8).fill_(0x7F if poison == "big" else 0xFF)
    return t


def g_ranges(lib, x, br, poison="nan"):
    n, cols = x.shape
    xd = dev(x) if n else torch.empty((0, cols), device="cuda")
    out = poisoned((R.n_blocks(n, br), 2, cols), torch.float32, poison)
    ok(lib, lib.gsr_quant_ranges(n, cols, _ptr(xd) if n else None, br, _ptr(out), _stream()))
    return out


def g_encode(lib, x, nbits, rg, br, kind=0, poison="nan"):
    n, cols = x.shape
    out = poisoned((n, cols), torch.uint8 if nbits <= 8 else torch.int16, poison)
    ok(lib, lib.gsr_quant_encode(n, cols, nbits, kind, _ptr(dev(x)), br, _ptr(rg), _ptr(out), _stream()))
    return out


def g_decode(lib, codes, nbits, rg, br, kind=0, poison="nan"):
    n, cols = codes.shape
    out = poisoned((n, cols), torch.float32, poison)
    ok(lib, lib.gsr_quant_decode(n, cols, nbits, kind, _ptr(codes), br, _ptr(rg), _ptr(out), _stream()))
    return out


def g_fake(L, groups, n, in_place=False, poison="nan"):
    """groups: (device rows, bits, kind, block_rows, device ranges or None) -> the outputs."""
    lib = L.load()
    arr = (L.QuantGroup * len(groups))()
    outs = []
    for i, (x, nbits, kind, br, rg) in enumerate(groups):
        o = x if in_place else poisoned(tuple(x.shape), torch.float32, poison)
        outs.append(o)
        arr[i] = L.QuantGroup(x.data_ptr(), o.data_ptr(), int(x.shape[1]), nbits, kind, br, rg.data_ptr() if rg is not None else None)
    ok(lib, lib.gsr_quant_fake(arr, len(groups), n, _stream()))
    return outs


def data(n, cols, seed, specials=True):
    """Columns of different centres and widths; NaN, Inf and -0 sprinkled in (never a whole column)."""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(n, cols)) * 10.0 ** rng.uniform(-3, 2, size=cols) + rng.normal(size=cols) * 3).astype(f32)
    if specials and n >= 8:
        for v in (NAN, INF, -INF, f32(-0.0), f32(0.0)):
            x[rng.integers(0, n, max(1, n // 50)), rng.integers(0, cols, max(1, n // 50))] = v
    return x


def check_all(pkg, x, nbits, br, poison="nan"):
    """ranges, encode, decode and the one-group fake pass of `x` against the restatement."""
    L = pkg._lib
    lib = L.load()
    n, cols = x.shape
    want_rg = R.ranges(x, br)
    rg = g_ranges(lib, x, br, poison)
    assert np.array_equal(bits(rg), bits(want_rg)), "ranges"
    want_q = R.encode(x, nbits, want_rg, br)
    q = g_encode(lib, x, nbits, rg, br, 0, poison)
    assert np.array_equal(host_codes(q), want_q), "codes"
    want_y = R.decode(want_q, nbits, want_rg, br)
    assert np.array_equal(bits(g_decode(lib, q, nbits, rg, br, 0, poison)), bits(want_y)), "decode"
    assert np.array_equal(bits(g_fake(L, [(dev(x), nbits, 0, br, rg)], n, poison=poison)[0]), bits(want_y)), "fake"
    torch.cuda.synchronize()


# ---- 1. against the restatement: a sparse walk through the cross product ----
CASES = [  # n, cols, bits, block_rows
    (1, 1, 1, 0), (1, 48, 16, 64), (63, 3, 8, 64), (63, 45, 9, 0), (64, 4, 16, 64), (64, 48, 1, 0), (65, 1, 9, 64), (65, 45, 8, 64),
    (255, 3, 16, 256), (255, 48, 8, 0), (256, 4, 1, 256), (256, 45, 16, 256), (257, 3, 9, 256), (257, 48, 9, 64), (1023, 1, 8, 1024),
    (1023, 45, 1, 1024), (1024, 4, 8, 0), (1024, 48, 16, 1024), (1025, 3, 1, 0), (1025, 4, 9, 1024), (1025, 45, 8, 0),
    (2049, 1, 16, 0), (2049, 3, 8, 256), (2049, 4, 16, 1024), (2049, 45, 9, 256), (2049, 48, 8, 64)]


@pytest.mark.parametrize("n,cols,nbits,br", CASES)
def test_against_the_restatement(pkg, n, cols, nbits, br):
    check_all(pkg, data(n, cols, 1000 * cols + n), nbits, br)


@pytest.mark.parametrize("cols,nbits", [(3, 16), (4, 8), (45, 8)])
def test_one_block_across_many_workgroups(pkg, cols, nbits):
    """n = 70 000: 69 workgroups meet in the integer min / max atomics; each column's extremes lie in different workgroups."""
    x = data(70000, cols, 7 + cols)
    x[69999, 0], x[1024, cols - 1], x[35000, cols // 2] = f32(-1e6), f32(1e6), f32(-2e6)
    check_all(pkg, x, nbits, 0)


# ---- 2. where an extreme sits ----
@pytest.mark.parametrize("cols", [1, 3, 4, 45, 48])
def test_extremes_on_block_edges_and_last_lanes_ragged_last_block(pkg, cols):
    """Blocks of 64 over 200 rows (the last block has 8): every column's maximum on the first row of a block and its minimum on
    the last row (lane 63 of the row-per-lane wave) or the other way round; the last column is the column-per-lane path's last
    lane.  The one-block form over 2049 rows: the extremes on rows 0, 1023, 1024 and 2048."""
    rng = np.random.default_rng(cols)
    x = rng.uniform(-1, 1, size=(200, cols)).astype(f32)
    for b, (r0, r1) in enumerate(((0, 63), (64, 127), (128, 191), (192, 199))):
        x[r0, :], x[r1, :] = (f32(5 + b), f32(-7 - b)) if b % 2 == 0 else (f32(-5 - b), f32(7 + b))
        x[r1, cols - 1] *= f32(2)
    for br in (64, 0):
        check_all(pkg, x, 8, br)
    want = R.ranges(x, 64)
    assert want[1, 0, 0] == -6 and want[1, 1, cols - 1] == 16 and want[3, 0, 0] == -8
    y = rng.uniform(-1, 1, size=(2049, cols)).astype(f32)
    for c in range(cols):
        lo_row, hi_row = ((0, 2048), (1023, 1024), (2048, 0), (1024, 1023))[c % 4]
        y[lo_row, c], y[hi_row, c] = f32(-9), f32(9)
    check_all(pkg, y, 16, 0)
    assert np.abs(R.ranges(y, 0)).min() == 9


# ---- 3. the hand values of tests/test_quant_cpu.py, on the device ----
def test_hand_values_on_the_device(pkg):
    lib = pkg._lib.load()
    rg = dev(np.array([[[0.0], [1.0]]], f32))
    x = np.array([[NAN], [INF], [-INF], [0.25], [2.0], [-1.0]], f32)
    for nbits, want in ((8, [0, 255, 0, 64, 255, 0]), (16, [0, 65535, 0, 16384, 65535, 0]), (1, [0, 1, 0, 0, 1, 0])):
        assert host_codes(g_encode(lib, x, nbits, rg, 0)).reshape(-1).tolist() == want
    c = np.full((5, 1), 3.25, f32)                                            # a constant column
    rc = g_ranges(lib, c, 0)
    assert rc.reshape(-1).tolist() == [3.25, 3.25] and not host_codes(g_encode(lib, c, 8, rc, 0)).any()
    assert np.array_equal(bits(g_decode(lib, dev_codes(np.full((5, 1), 200), 8), 8, rc, 0)), bits(c))
    big = dev(np.array([[[-3e38], [3e38]]], f32))                             # the span overflows
    assert not host_codes(g_encode(lib, np.array([[0.0], [3e38]], f32), 8, big, 0)).any()
    assert bits(g_decode(lib, dev_codes([[7]], 8), 8, big, 0)).tolist() == [[bits(f32(-3e38)).item()]]
    for lo, hi in ((NAN, 1.0), (0.0, NAN), (NAN, NAN), (1.0, 0.0), (-INF, 0.0), (0.0, INF)):   # ranges that are not ok
        bad = dev(np.array([[[lo], [hi]]], f32))
        assert not host_codes(g_encode(lib, np.array([[0.5]], f32), 8, bad, 0)).any()
        assert bits(g_decode(lib, dev_codes([[9]], 8), 8, bad, 0)).tolist() == [[bits(f32(lo)).item()]]
    z = np.array([[0.0, -0.0, NAN, 5.0], [-0.0, 0.0, INF, NAN], [0.0, 0.0, -INF, -5.0]], f32)   # -0 < +0; not finite: skipped
    for br in (0, 64):
        got = bits(g_ranges(lib, z, br))
        assert got[0, 0].tolist() == [0x80000000, 0x80000000, 0, bits(f32(-5.0)).item()]
        assert got[0, 1].tolist() == [0, 0, 0, bits(f32(5.0)).item()]
    assert bits(g_ranges(lib, np.zeros((0, 3), f32), 0)).tolist() == [[[0, 0, 0], [0, 0, 0]]]   # n = 0: the one block, +0
    tiny = f32(1e-45)                                                         # subnormals are kept
    srg_host = (np.array([[[0.0], [255.0]]], f32) * tiny).astype(f32)         # 255 subnormal steps
    srg = dev(srg_host)
    sx = (np.arange(256, dtype=f32) * tiny).astype(f32).reshape(-1, 1)
    assert host_codes(g_encode(lib, sx, 8, srg, 0)).reshape(-1).tolist() == [0] + [255] * 255
    assert np.array_equal(bits(g_decode(lib, dev_codes(np.arange(256).reshape(-1, 1), 8), 8, srg, 0)), bits(sx))
    assert np.array_equal(bits(g_ranges(lib, sx, 0)), bits(srg_host))
    srg2 = dev(np.array([[[0.0], [2.0 ** -127]]], f32))
    sx2 = np.array([[0.0], [2.0 ** -127], [2.0 ** -128], [3 * 2.0 ** -129], [2.0 ** -149]], f32)
    assert host_codes(g_encode(lib, sx2, 1, srg2, 0)).reshape(-1).tolist() == [0, 1, 0, 1, 0]
    trg = dev(np.array([[[0.0], [255.0]]], f32))                              # rintf ties go to even
    tx = np.array([[0.5], [1.5], [2.5], [3.5], [254.5], [0.49999997], [2.5000002]], f32)
    assert host_codes(g_encode(lib, tx, 8, trg, 0)).reshape(-1).tolist() == [0, 2, 2, 4, 254, 0, 3]
    torch.cuda.synchronize()


# ---- 4. poisons, twice ----
def test_poisoned_outputs_and_two_runs(pkg):
    """Outputs and ranges pre-filled with 0xFF bytes (NaN) and with 0x7F bytes (3.4e38, codes 127 / 32639): the same results,
    and a second run of everything gives the first run's bits."""
    for n, cols, nbits, br in ((2049, 3, 16, 256), (2049, 45, 8, 0), (1025, 4, 9, 0)):
        x = data(n, cols, 77 + cols)
        for poison in ("nan", "big"):
            check_all(pkg, x, nbits, br, poison)
        lib = pkg._lib.load()
        runs = []
        for _ in range(2):
            rg = g_ranges(lib, x, br, "big")
            q = g_encode(lib, x, nbits, rg, br, 0, "big")
            runs.append((rg, q, g_decode(lib, q, nbits, rg, br, 0, "big")))
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8)) for a, b in zip(*runs))


# ---- 5. the one-launch fake pass ----
def _six_groups(n, seed=5):
    shapes = (("points", 3, 16, 0, 256), ("features_dc", 3, 8, 0, 0), ("features_rest", 45, 8, 0, 0), ("opacities", 1, 8, 0, 0),
              ("scales", 3, 8, 0, 0), ("rotations", 4, 8, 1, 0))
    return [(data(n, cols, seed + i, specials=(kind == 0)), nbits, kind, br) for i, (_, cols, nbits, kind, br) in enumerate(shapes)]


@pytest.mark.parametrize("n", [257, 2049])
def test_fake_six_groups_in_one_launch_equal_six_encode_decode_pairs(pkg, n):
    L = pkg._lib
    lib = L.load()
    groups, want = [], []
    for x, nbits, kind, br in _six_groups(n):
        rg = None if kind else g_ranges(lib, x, br)
        q = g_encode(lib, x, nbits, rg, br, kind)
        want.append(g_decode(lib, q, nbits, rg, br, kind))
        groups.append((dev(x), nbits, kind, br, rg))
        ref_rg = None if kind else R.ranges(x, br)
        assert np.array_equal(bits(want[-1]), bits(R.fake(x, nbits, ref_rg, br, kind)))
    out = g_fake(L, groups, n)
    torch.cuda.synchronize()
    for o, w in zip(out, want):
        assert torch.equal(o.view(torch.int32), w.view(torch.int32))
    # in place equals out of place; a launch of ONE group equals its part of the six
    copies = [(x.clone(), nbits, kind, br, rg) for x, nbits, kind, br, rg in groups]
    for o, w in zip(g_fake(L, copies, n, in_place=True), want):
        assert torch.equal(o.view(torch.int32), w.view(torch.int32))
    for i in (0, 2, 5):
        assert torch.equal(g_fake(L, [groups[i]], n)[0].view(torch.int32), want[i].view(torch.int32))
    assert not any(torch.equal(c[0], g[0]) for c, g in zip(copies, groups))   # (the copies were overwritten, the inputs not)


# ---- 6. unit quaternions ----
def test_unit_quaternion_rows(pkg):
    lib = pkg._lib.load()
    rng = np.random.default_rng(6)
    q = (rng.normal(size=(1025, 4)) * rng.uniform(0.01, 100, size=(1025, 1))).astype(f32)
    q[:8] = np.array([[2, 0, 0, 0], [-1, 1, 0, 0], [0, 0, 0, 0], [NAN, 1, 0, 0], [3e38, 3e38, 0, 0], [1e-30, 0, 0, 0], [0, 0, -5, 0],
                      [INF, 0, 0, 0]], f32)
    q[8:16] = f32(1e-20) * q[16:24]                                           # squares that are subnormal or underflow
    for nbits in (1, 8, 9, 16):
        codes = g_encode(lib, q, nbits, None, 0, 1)
        assert np.array_equal(host_codes(codes), R.encode(q, nbits, None, 0, R.UNIT_QUAT)), nbits
        assert np.array_equal(bits(g_decode(lib, codes, nbits, None, 0, 1)), bits(R.decode(host_codes(codes), nbits, None, 0, R.UNIT_QUAT)))
    c8 = host_codes(g_encode(lib, q, 8, None, 0, 1))
    assert c8[0].tolist() == [255, 128, 128, 128] and c8[1].tolist() == [218, 37, 128, 128] and c8[2].tolist() == [255, 128, 128, 128]
    assert c8[3].tolist() == c8[4].tolist() == c8[5].tolist() == c8[7].tolist() == [255, 128, 128, 128] and c8[6].tolist() == [128, 128, 0, 128]
    torch.cuda.synchronize()


# ---- 7. damaged codes ----
@pytest.mark.parametrize("nbits", [1, 9])
def test_codes_above_the_last_level_read_as_the_last_level(pkg, nbits):
    lib = pkg._lib.load()
    rng = np.random.default_rng(nbits)
    for cols in (3, 4, 45):
        x = data(300, cols, 70 + cols, specials=False)
        rg = R.ranges(x, 64)
        codes = rng.integers(0, 256 if nbits <= 8 else 65536, size=(300, cols))
        codes[0, :] = 255 if nbits <= 8 else 65535
        assert (codes > (1 << nbits) - 1).mean() > 0.4
        got = g_decode(lib, dev_codes(codes, nbits), nbits, dev(rg), 64)
        assert np.array_equal(bits(got), bits(R.decode(np.minimum(codes, (1 << nbits) - 1), nbits, rg, 64)))
    qc = rng.integers(0, 256 if nbits <= 8 else 65536, size=(300, 4))
    assert np.array_equal(bits(g_decode(lib, dev_codes(qc, nbits), nbits, None, 0, 1)), bits(R.decode(qc, nbits, None, 0, R.UNIT_QUAT)))
    torch.cuda.synchronize()


# ---- 8. pack_model / unpack on the grid scene ----
def _u16(t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _raw_model(pkg, seed=0, rest_scale=0.2, staggered=False):
    """The 64-Gaussian grid scene as a GaussianModel of RAW parameters at SH degree 3, ids 0 .. 63.  `staggered`: the depths
    3.0, 3.015, ... in a shuffled order instead of 3.0 sixty-four times."""
    m, cam = scenes.grid_scene_rgbdn()
    n = m["means"].shape[0]
    rng = np.random.default_rng(seed)
    if staggered:
        m["means"][:, 2] += f32(0.015) * np.random.default_rng(seed + 1).permutation(n).astype(f32)
    rest = (rest_scale * rng.normal(size=(n, 15, 3))).astype(f32)
    rots = rng.normal(size=(n, 4)).astype(f32)
    op = np.log(m["opac"] / (1 - m["opac"])).astype(f32).reshape(-1, 1) + rng.normal(size=(n, 1)).astype(f32) * f32(0.3)
    model = pkg.densification.GaussianModel(dev(m["means"]), dev(m["shs"]), dev(rest), dev(np.log(m["scales"])), dev(rots), dev(op),
                                            ids=torch.arange(n, dtype=torch.int32, device="cuda"))
    return model, cam


def _render(pkg, rast, camera, model):
    shs, oa, sa = pkg.rasterizer.prologue_forward(model.features_dc, model.features_rest, model.opacities, model.scales)
    return rast.forward_raw(model.points, shs, oa, sa, model.rotations, camera, 3, (0.0, 0.0, 0.0))


@pytest.fixture(scope="module")
def grid(pkg):
    model, cam = _raw_model(pkg)
    camera = pkg.Camera(cam.width, cam.height, tuple(cam.focal))
    rast = pkg.rasterizer.GaussianRasterizer(cam.width, cam.height, mode="rgb", device="cuda:0")
    sh = pkg.sh_codebook.fit_sh_codebook(model.features_rest, 8, iters=3)
    torch.cuda.synchronize()
    return model, camera, rast, sh


def _same_container(a, b):
    assert a.codes.keys() == b.codes.keys() and a.shapes == b.shapes and a.n == b.n and a.spec == b.spec
    for g in a.codes:
        assert torch.equal(_u16(a.codes[g]), _u16(b.codes[g])), g
        assert (a.ranges[g] is None) == (b.ranges.get(g) is None)
        if a.ranges[g] is not None:
            assert torch.equal(a.ranges[g].view(torch.int32), b.ranges[g].view(torch.int32)), g
    assert (a.sh is None) == (b.sh is None)
    if a.sh is not None:
        assert torch.equal(_u16(a.sh.indices), _u16(b.sh.indices)) and torch.equal(a.sh.codebook, b.sh.codebook) and a.sh.shape == b.sh.shape
    assert (a.ids is None) == (b.ids is None) and (a.ids is None or torch.equal(a.ids, b.ids))


@pytest.mark.parametrize("with_sh", [True, False])
def test_pack_applies_the_morton_permutation_to_every_array(pkg, grid, with_sh):
    Q, S, D = pkg.quantised_model, pkg.sh_codebook, pkg.densification
    model, camera, rast, sh = grid
    sh = sh if with_sh else None
    spec = Q.QuantSpec(points=(16, 64))
    packed = Q.pack_model(model, sh, spec)
    perm = packed.permutation
    assert perm is not None and perm.dtype == torch.int32 and sorted(perm.tolist()) == list(range(64)) and perm.tolist() != list(range(64))
    assert torch.equal(packed.ids, perm)                                      # ids were 0 .. 63: they ARE the permutation
    p = perm.long()
    by_hand = D.GaussianModel(*[getattr(model, k)[p].contiguous() for k in D.PARAMS], ids=model.ids[p].contiguous())
    sh_hand = S.SHCodebook(sh.codebook, sh.indices.view(torch.int16)[p].contiguous().view(torch.uint16), sh.shape) if with_sh else None
    kept = Q.pack_model(by_hand, sh_hand, spec, order=None)
    assert kept.permutation is None
    _same_container(packed, kept)
    assert ("features_rest" in packed.codes) == (not with_sh)
    # ... and every group is the restatement's codes of the permuted rows
    for g in packed.codes:
        nbits, br = getattr(spec, g)
        rows = getattr(by_hand, g).reshape(64, -1).cpu().numpy()
        rg = None if g == "rotations" else R.ranges(rows, br)
        assert np.array_equal(host_codes(packed.codes[g]), R.encode(rows, nbits, rg, br, int(g == "rotations"))), g
    un = packed.unpack()
    assert len(un) == 64 and un.features_rest.shape == (64, 15, 3) and torch.equal(un.ids, perm)
    if with_sh:
        assert torch.equal(un.features_rest, sh_hand.decode())
    # a sanity check of the whole chain, not a measurement (the bits are held above): against the model with the same
    # features_rest, the 8- and 16-bit attributes move a colour by 0.004 and a disc's edge by a tenth of a pixel
    same_rest = D.GaussianModel(model.points, model.features_dc, un.features_rest[torch.argsort(p)].contiguous(), model.scales, model.rotations,
                                model.opacities)
    assert float((_render(pkg, rast, camera, un) - _render(pkg, rast, camera, same_rest)).abs().mean()) < 0.02
    assert packed.nbytes == sum(c.numel() * c.element_size() for c in packed.codes.values()) + 4 * 2 * (3 + 3 + 1 + 3 + (0 if with_sh else 45)) + (
        sh.nbytes if with_sh else 0)


def _stable_rotation_codes(n, seed):
    """Rows of 8-bit unit-quaternion codes that decode and encode to themselves under the restatement: the decoded vector is not
    of unit length, so encode normalises it again — most rows move by a code; fixed points are found by iterating."""
    rng = np.random.default_rng(seed)
    c = R.encode(rng.normal(size=(16 * n, 4)).astype(f32), 8, None, 0, R.UNIT_QUAT)
    for _ in range(8):
        c = R.encode(R.decode(c, 8, None, 0, R.UNIT_QUAT), 8, None, 0, R.UNIT_QUAT)
    fixed = (R.encode(R.decode(c, 8, None, 0, R.UNIT_QUAT), 8, None, 0, R.UNIT_QUAT) == c).all(axis=1)
    assert fixed.sum() >= n
    return c[fixed][:n]


def _grid_container(pkg, sh, n=64):
    """A container made by hand whose ranges have power-of-two steps, so that every operation of decode and of encoding the
    decoded value again is exact — the idempotence condition of §25 with room to spare (step = 2^13 ulp or more); every (block,
    column) holds code 0 and the last code, so the ranges of the unpacked model are these ranges."""
    Q = pkg.quantised_model
    rng = np.random.default_rng(11)
    spec = Q.QuantSpec(points=(16, 64))
    lo_step = dict(points=([-1.0, -1.0, 2.0], 2.0 ** -15), features_dc=([-2.0] * 3, 2.0 ** -6), opacities=([0.0], 2.0 ** -5),
                   scales=([-5.0] * 3, 2.0 ** -7), features_rest=([-0.5] * 45, 2.0 ** -9))
    shapes = dict(points=(n, 3), features_dc=(n, 1, 3), features_rest=(n, 15, 3), opacities=(n, 1), scales=(n, 3), rotations=(n, 4))
    codes, ranges = {}, {}
    for g, (lo, step) in lo_step.items():
        if g == "features_rest" and sh is not None:
            continue
        nbits = getattr(spec, g)[0]
        last = (1 << nbits) - 1
        c = rng.integers(0, last + 1, size=(n, len(lo)))
        for col in range(len(lo)):
            a, b = rng.choice(n, 2, replace=False)
            c[a, col], c[b, col] = 0, last
        codes[g] = dev_codes(c, nbits).view(torch.uint16) if nbits > 8 else dev_codes(c, nbits)
        lo = np.asarray(lo, f32)
        ranges[g] = dev(np.stack([lo, (lo + f32(last) * f32(step)).astype(f32)])[None])
    codes["rotations"], ranges["rotations"] = dev_codes(_stable_rotation_codes(n, 12), 8), None
    return Q.QuantisedModel(n, spec, codes, ranges, {g: shapes[g] for g in codes}, sh=sh)


@pytest.mark.parametrize("with_sh", [True, False])
def test_a_model_on_the_grid_packs_to_itself_bit_for_bit(pkg, grid, tmp_path, with_sh):
    Q = pkg.quantised_model
    _, camera, rast, sh = grid
    hand = _grid_container(pkg, sh if with_sh else None)
    on_grid = hand.unpack()
    again = Q.pack_model(on_grid, hand.sh, hand.spec, order=None)
    _same_container(hand, again)                                              # the codes AND the ranges come back
    back = again.unpack()
    for k in pkg.densification.PARAMS:
        assert torch.equal(getattr(back, k).view(torch.int32), getattr(on_grid, k).view(torch.int32)), k
    img = _render(pkg, rast, camera, on_grid)
    assert float(img.abs().sum()) > 0 and torch.equal(_render(pkg, rast, camera, back), img)
    # the Morton order permutes the rows and nothing else
    sorted_ = Q.pack_model(on_grid, hand.sh, hand.spec)
    p = sorted_.permutation.long()
    assert torch.equal(sorted_.unpack().points.view(torch.int32), on_grid.points[p].view(torch.int32))
    # save -> load -> unpack equals unpack
    for compressed in (True, False):
        path = str(tmp_path / f"grid_{int(compressed)}.npz")
        again.save(path, compressed=compressed)
        loaded = Q.QuantisedModel.load(path, device="cuda")
        _same_container(again, loaded)
        lm = loaded.unpack()
        for k in pkg.densification.PARAMS:
            assert torch.equal(getattr(lm, k).view(torch.int32), getattr(back, k).view(torch.int32)), k


# ---- 9. FakeQuantizer ----
def test_fake_quantizer_apply_equals_the_chain_by_hand(pkg, grid):
    Q = pkg.quantised_model
    model, _, _, sh = grid
    spec = Q.QuantSpec(points=(16, 64), scales=(6, 0))
    fq = Q.FakeQuantizer(spec)
    with pytest.raises(RuntimeError):
        fq.apply(model)
    fq.refresh(model)
    with torch.no_grad():
        out = fq.apply(model)
        out_sh = fq.apply(model, sh_codebook=sh)
        out_tuner = fq.apply(model, sh_codebook=pkg.sh_codebook.SHCodebookFineTuner(sh))
    assert len(out) == 6
    for g, o, o2 in zip(Q.GROUPS, out, out_sh):
        x = getattr(model, g)
        rows = x.reshape(64, -1)
        nbits, br = getattr(spec, g)
        kind = spec.kind(g)
        rg = None if kind else Q.quant_ranges(rows, br)
        want = Q.quant_decode(Q.quant_encode(rows, nbits, rg, br, kind), nbits, rg, br, kind).view(x.shape)
        assert o.shape == x.shape and torch.equal(o.view(torch.int32), want.view(torch.int32)), g
        assert g not in ("points", "features_dc", "rotations") or not torch.equal(o, x)
        assert torch.equal(o2, sh.decode() if g == "features_rest" else o), g
    assert torch.equal(out_tuner[2], sh.decode())


def test_fake_quantizer_gradient_is_the_incoming_gradient(pkg, grid):
    Q, D = pkg.quantised_model, pkg.densification
    model, _, _, _ = grid
    leaves = {k: getattr(model, k).clone().requires_grad_(True) for k in D.PARAMS}
    m = D.GaussianModel(**leaves)
    fq = Q.FakeQuantizer(Q.QuantSpec(points=(16, 64), opacities=(2, 0)))          # 2 bits: most values are far from their level
    fq.refresh(m)
    out = fq.apply(m)
    gen = torch.Generator(device="cuda").manual_seed(3)
    ws = [torch.randn(o.shape, device="cuda", generator=gen) for o in out]
    assert all(o.requires_grad for o in out)
    sum((o * w).sum() for o, w in zip(out, ws)).backward()
    for g, w in zip(Q.GROUPS, ws):
        assert torch.equal(leaves[g].grad, w), g


def test_positive_w_rotations_keeps_the_codes(pkg, grid):
    Q = pkg.quantised_model
    model, _, _, _ = grid
    rot = model.rotations.clone()
    adam = pkg.optim.Adam(rot, 1e-3)
    adam.mu.copy_(torch.arange(256, device="cuda", dtype=torch.float32) + 1)
    mu = adam.mu.clone().view(64, 4)
    before = Q.quant_encode(model.rotations, 8, None, 0, Q.UNIT_QUAT)
    flip = Q.positive_w_rotations_(rot, adam)
    assert torch.equal(flip, model.rotations[:, :1] < 0) and 0 < int(flip.sum()) < 64
    assert torch.equal(rot, torch.where(flip, -model.rotations, model.rotations)) and torch.equal(adam.mu.view(64, 4), torch.where(flip, -mu, mu))
    assert torch.equal(Q.quant_encode(rot, 8, None, 0, Q.UNIT_QUAT), before)   # -q is the same rotation and the same code
    assert not bool(Q.positive_w_rotations_(rot).any())


def _l1_cotangent(img, target):
    leaf = img.detach().clone().requires_grad_(True)
    loss = (leaf - target).abs().mean()
    return loss.detach(), torch.autograd.grad(loss, leaf)[0].contiguous()


def test_forty_quantisation_aware_steps_lower_the_quantised_l1(pkg, grid):
    """The step without autograd of FakeQuantizer's docstring, 40 times, on the grid scene: the target is the render of the
    original model, the run starts from that model with its colours and opacities disturbed, all six groups are stepped, and
    what is measured is the L1 of the render of the QUANTISED model (default spec, positions in blocks of 64; ranges refreshed
    every 10 steps).  Lower at the end than at the start; no other threshold.  Deterministic.  Measured: DESIGN.md §25.

    Two properties of the scene that have nothing to do with the quantiser, both measured before this test was written
    (§25): the grid's 64 discs overlap and all sit at depth 3.0 exactly, so the first position step of ANY size re-sorts them
    and doubles the L1 with or without the fake pass — here the depths are staggered by 0.015, more than twice what 40 position
    steps can move; and half of the random rotations have w < 0, where the straight-through identity points uphill —
    positive_w_rotations_ flips them first, as its docstring asks."""
    Q, D, O, RZ = pkg.quantised_model, pkg.densification, pkg.optim, pkg.rasterizer
    _, camera, rast, _ = grid
    model, _ = _raw_model(pkg, staggered=True)
    target = _render(pkg, rast, camera, model).clone()
    rng = np.random.default_rng(40)
    m = D.GaussianModel(**{k: getattr(model, k).clone() for k in D.PARAMS})
    m.features_dc += dev(0.5 * rng.normal(size=(64, 1, 3)).astype(f32))
    m.opacities -= 1.0
    fq = Q.FakeQuantizer(Q.QuantSpec(points=(16, 64)))
    lrs = dict(points=1.6e-4, features_dc=2e-2, features_rest=2.5e-3 / 20, opacities=5e-2, scales=5e-3, rotations=1e-3)
    raw = [getattr(m, g) for g in Q.GROUPS]
    opts = [O.Adam(t, lrs[g], eps=1e-15) for g, t in zip(Q.GROUPS, raw)]
    flipped = Q.positive_w_rotations_(m.rotations, opts[5])
    assert 0 < int(flipped.sum()) < 64 and bool((m.rotations[:, 0] >= 0).all())
    bg = (0.0, 0.0, 0.0)

    def quantised_pass():
        with torch.no_grad():
            pts, dc, rest, op, sc, rot = fq.apply(m)
        shs, oa, sa = RZ.prologue_forward(dc, rest, op, sc)
        img = rast.forward_raw(pts, shs, oa, sa, rot, camera, 3, bg)
        return (pts, shs, oa, sa, rot), img

    fq.refresh(m)
    before = float(_l1_cotangent(quantised_pass()[1], target)[0])
    for step in range(40):
        if step % 10 == 0:
            fq.refresh(m)
        (pts, shs, oa, sa, rot), img = quantised_pass()
        _, vpix = _l1_cotangent(img, target)
        vm, vshs, vo, vsc, vr = rast.backward_raw(vpix, pts, shs, oa, sa, rot, camera, 3, bg)[:5]
        vdc, vrest, vo_raw, vs_raw = RZ.prologue_backward(oa, sa, vshs, vo.view(-1, 1), vsc, scale_dims=3)
        O.step_all(opts, raw, [vm, vdc, vrest, vo_raw, vs_raw, vr])
    fq.refresh(m)
    after = float(_l1_cotangent(quantised_pass()[1], target)[0])
    print(f"L1 of the quantised model's render against the target: {before:.6f} before, {after:.6f} after 40 steps")
    assert before > 0 and after < before


# ---- 10. guarded arenas ----
def _guarded_calls(L, P, tag):
    lib = L.load()
    n = 2049
    I16, U8 = torch.int16, torch.uint8
    st = _stream()
    rng = np.random.default_rng(90)
    rcs, checks = [], []
    for cols, nbits, br in ((3, 16, 256), (4, 8, 0), (45, 8, 64), (1, 9, 0)):
        x = data(n, cols, 91 + cols)
        want_rg = R.ranges(x, br)
        rows = P.place(f"rows {cols}", x)
        rg = P.place(f"ranges {cols}", tuple(want_rg.shape))
        ct = U8 if nbits <= 8 else I16
        codes = P.place(f"codes {cols}", (n, cols), ct)
        out, out_f = P.place(f"decoded {cols}", (n, cols)), P.place(f"fake {cols}", (n, cols))
        inout = P.place(f"in place {cols}", x, role="inout")
        # damaged ranges (NaN, inverted, infinite, huge) and damaged codes (every value of the code type)
        bad_rg = want_rg.copy()
        bad_rg.reshape(-1)[::3] = NAN
        bad_rg.reshape(-1)[1::7] = f32(3e38)
        bad_rg[:, 0, -1], bad_rg[:, 1, -1] = INF, -INF
        bad_c = rng.integers(0, 256 if nbits <= 8 else 65536, size=(n, cols))
        rg_bad = P.place(f"ranges, damaged {cols}", bad_rg)
        c_bad = P.place(f"codes, damaged {cols}", bad_c.astype(np.uint8) if nbits <= 8 else bad_c.astype(np.uint16).view(np.int16))
        o_bad, c_out_bad = P.place(f"decoded, damaged {cols}", (n, cols)), P.place(f"codes of damaged ranges {cols}", (n, cols), ct)
        if P.skew == "worst":
            assert rows.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4 and codes.data_ptr() % 16 == (1 if nbits <= 8 else 2)
        elif P.skew == "aligned":
            assert rows.data_ptr() % 16 == 0 and codes.data_ptr() % 16 == 0
        for t in (rg, codes, out, out_f, o_bad, c_out_bad):
            t.view(-1).view(U8).fill_(0xFF)
        one = lambda a, b, r: (L.QuantGroup * 1)(L.QuantGroup(a.data_ptr(), b.data_ptr(), cols, nbits, 0, br, r.data_ptr()))  # noqa: E731
        rcs += [lib.gsr_quant_ranges(n, cols, _ptr(rows), br, _ptr(rg), st),
                lib.gsr_quant_encode(n, cols, nbits, 0, _ptr(rows), br, _ptr(rg), _ptr(codes), st),
                lib.gsr_quant_decode(n, cols, nbits, 0, _ptr(codes), br, _ptr(rg), _ptr(out), st),
                lib.gsr_quant_fake(one(rows, out_f, rg), 1, n, st),
                lib.gsr_quant_fake(one(inout, inout, rg), 1, n, st),
                lib.gsr_quant_encode(n, cols, nbits, 0, _ptr(rows), br, _ptr(rg_bad), _ptr(c_out_bad), st),
                lib.gsr_quant_decode(n, cols, nbits, 0, _ptr(c_bad), br, _ptr(rg_bad), _ptr(o_bad), st)]
        want_q = R.encode(x, nbits, want_rg, br)
        checks.append((cols, rg, want_rg, codes, want_q, out, out_f, inout, R.decode(want_q, nbits, want_rg, br),
                       c_out_bad, R.encode(x, nbits, bad_rg, br), o_bad, R.decode(bad_c, nbits, bad_rg, br)))
    q = data(n, 4, 99, specials=False)
    qrows, qcodes, qout = P.place("quaternions", q), P.place("quaternion codes", (n, 4), U8), P.place("quaternions decoded", (n, 4))
    qbad = P.place("quaternion codes, damaged", rng.integers(0, 65536, size=(n, 4)).astype(np.uint16).view(np.int16))
    qbad_out = P.place("quaternions decoded, damaged", (n, 4))
    rcs += [lib.gsr_quant_encode(n, 4, 8, 1, _ptr(qrows), 0, None, _ptr(qcodes), st),
            lib.gsr_quant_decode(n, 4, 8, 1, _ptr(qcodes), 0, None, _ptr(qout), st),
            lib.gsr_quant_decode(n, 4, 9, 1, _ptr(qbad), 0, None, _ptr(qbad_out), st)]
    assert rcs == [0] * len(rcs), (tag, rcs, lib.gsr_last_error_string().decode())
    torch.cuda.synchronize()
    assert P.check() == [], (tag, P.check())
    P.assert_inputs_unchanged()
    for cols, rg, want_rg, codes, want_q, out, out_f, inout, want_y, c_out_bad, want_cb, o_bad, want_ob in checks:
        assert np.array_equal(bits(rg), bits(want_rg)) and np.array_equal(host_codes(codes), want_q), (tag, cols)
        assert np.array_equal(bits(out), bits(want_y)) and np.array_equal(bits(out_f), bits(want_y)) and np.array_equal(bits(inout), bits(want_y)), (tag, cols)
        assert np.array_equal(host_codes(c_out_bad), want_cb) and np.array_equal(bits(o_bad), bits(want_ob)), (tag, cols)
    assert np.array_equal(host_codes(qcodes), R.encode(q, 8, None, 0, R.UNIT_QUAT)), tag
    assert np.array_equal(bits(qout), bits(R.decode(host_codes(qcodes), 8, None, 0, R.UNIT_QUAT))), tag
    assert np.array_equal(bits(qbad_out), bits(R.decode(host_codes(qbad), 9, None, 0, R.UNIT_QUAT))), tag


def test_entry_points_on_guarded_buffers(pkg):
    """n = 2049 rows of 3, 4, 45 and 1 columns on the five placements: no guard word changes, the const inputs are unchanged, the
    poisoned outputs reach no result.  Under skew "worst" the floats start at 4 mod 16 (no vector access may be taken), the
    uint8 codes at an odd address and the uint16 codes at 2 mod 16; under "aligned" the cols = 4 vector paths run.  Two more
    calls per group read ranges with NaN, infinities, 3e38 and inverted ends, and codes of every value: wrong numbers — the
    restatement's — and no access outside the arrays."""
    for P in placements(1 << 23, "cuda"):
        _guarded_calls(pkg._lib, P, f"{P.skew}/{P.fill}")


# ---- 11. error codes ----
def test_error_codes(pkg):
    L, Q = pkg._lib, pkg.quantised_model
    lib, bad, st = L.load(), L.GSR_E_INVALID_ARG, _stream()
    n = 130
    x = torch.zeros((n + 1, 4), device="cuda")
    rg = torch.zeros((3, 2, 4), device="cuda")
    codes = torch.zeros((n + 1) * 4 + 8, dtype=torch.int16, device="cuda")
    X, RG, CO = x.data_ptr(), rg.data_ptr(), codes.data_ptr()

    def ranges(n=n, cols=4, rows=X, br=64, out=RG):
        return lib.gsr_quant_ranges(n, cols, rows, br, out, st)
    assert ranges() == 0
    for kw in (dict(n=-1), dict(n=1 << 31), dict(cols=0), dict(cols=49), dict(br=63), dict(br=32), dict(br=1088), dict(br=-64), dict(rows=None),
               dict(out=None), dict(rows=X + 2), dict(out=RG + 1)):
        assert ranges(**kw) == bad, kw
    assert ranges(n=0, rows=None, out=None) == 0 and ranges(n=0, rows=None, br=0) == 0 and ranges(n=0, rows=None, br=0, out=None) == bad

    def encode(n=n, cols=4, nbits=8, kind=0, rows=X, br=64, r=RG, out=CO):
        return lib.gsr_quant_encode(n, cols, nbits, kind, rows, br, r, out, st)

    def decode(n=n, cols=4, nbits=8, kind=0, c=CO, br=64, r=RG, out=X):
        return lib.gsr_quant_decode(n, cols, nbits, kind, c, br, r, out, st)
    assert encode() == 0 and decode() == 0 and encode(kind=1, r=None, br=0) == 0 and decode(kind=1, r=None, br=0) == 0
    assert encode(nbits=16) == 0 and decode(nbits=16) == 0 and encode(out=CO + 1) == 0 and decode(c=CO + 1) == 0   # uint8 codes: any address
    for f in (encode, decode):
        for kw in (dict(n=-1), dict(n=1 << 31), dict(cols=0), dict(cols=49), dict(nbits=0), dict(nbits=17), dict(kind=2), dict(kind=-1),
                   dict(kind=1, cols=3), dict(br=100), dict(br=2048), dict(r=None), dict(r=RG + 2), dict(out=None), dict(nbits=9, **{"out" if f is encode else "c": CO + 1})):
            assert f(**kw) == bad, (f.__name__, kw)
    assert encode(rows=None) == bad and encode(rows=X + 1) == bad and decode(c=None) == bad and decode(out=X + 2) == bad
    assert encode(n=0, rows=None, r=None, out=None) == 0 and decode(n=0, c=None, r=None, out=None) == 0

    outs = torch.zeros((L.QUANT_MAX_GROUPS + 1, n + 1, 4), device="cuda")

    def fake(count=1, n=n, **kw):
        f = dict(rows_in=X, cols=4, nbits=8, kind=0, br=64, r=RG)
        f.update(kw)
        m = max(count, 1)
        arr = (L.QuantGroup * m)(*[L.QuantGroup(f["rows_in"], f.get("rows_out", outs[i].data_ptr()), f["cols"], f["nbits"], f["kind"], f["br"], f["r"])
                                   for i in range(m)])
        return lib.gsr_quant_fake(arr, count, n, st)
    assert fake() == 0 and fake(count=L.QUANT_MAX_GROUPS) == 0 and fake(count=0) == 0 and fake(kind=1, r=None, br=0) == 0
    assert fake(count=L.QUANT_MAX_GROUPS + 1) == bad and fake(count=-1) == bad and lib.gsr_quant_fake(None, 1, n, st) == bad
    for kw in (dict(n=-1), dict(n=1 << 31), dict(cols=0), dict(cols=49), dict(nbits=0), dict(nbits=17), dict(kind=2), dict(kind=1, cols=3),
               dict(br=100), dict(r=None), dict(rows_in=None), dict(rows_out=None), dict(rows_in=X + 1), dict(rows_out=X + 2), dict(r=RG + 1)):
        assert fake(**kw) == bad, kw
    assert fake(n=0, rows_in=None, rows_out=None, r=None) == 0
    torch.cuda.synchronize()
    # the wrappers
    with pytest.raises(ValueError):
        Q.quant_encode(x, 8, rg[:1], 64)
    with pytest.raises(ValueError):
        Q.quant_encode(x[:, :3].contiguous(), 8, None, 0, Q.UNIT_QUAT)
    with pytest.raises(ValueError):
        Q.quant_ranges(x, 100)
    with pytest.raises(TypeError):
        Q.quant_decode(torch.zeros((4, 4), dtype=torch.uint8, device="cuda"), 12, rg[:1])
    with pytest.raises(ValueError):
        Q.pack_model(None, order="hilbert")
    assert lib.gsr_abi_version() == 6
