"""The quantised model container without a device: the numpy restatement tests/quant_ref.py against a literal
per-element loop, the derived error bound and idempotence condition, the hand values of the definition, the unit quaternions,
the archive, the nbytes arithmetic, and every error code that needs no device."""
import math
import struct

import numpy as np
import pytest
import torch

import quant_ref as R
from vq_ref import fmaf

f32, f64 = np.float32, np.float64
INF, NAN = f32(np.inf), f32(np.nan)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- 1. the restatement against a literal loop ----
def _key(x):
    b = struct.unpack("<I", struct.pack("<f", x))[0]
    return (~b & 0xFFFFFFFF) if b >> 31 else b ^ 0x80000000


def _loop_ranges(x, block_rows):
    n, cols = x.shape
    nb = R.n_blocks(n, block_rows)
    out = np.zeros((nb, 2, cols), f32)
    for b in range(nb):
        r0, r1 = (0, n) if block_rows == 0 else (b * block_rows, min(n, (b + 1) * block_rows))
        for c in range(cols):
            fin = [x[r, c] for r in range(r0, r1) if math.isfinite(x[r, c])]
            if fin:
                out[b, 0, c] = min(fin, key=_key)
                out[b, 1, c] = max(fin, key=_key)
    return out


def _loop_encode_decode(x, nbits, rg, block_rows):
    n, cols = x.shape
    q = np.zeros((n, cols), np.int64)
    y = np.zeros((n, cols), f32)
    L = (1 << nbits) - 1
    with np.errstate(all="ignore"):
        for r in range(n):
            b = r // block_rows if block_rows else 0
            for c in range(cols):
                lo, hi = rg[b, 0, c], rg[b, 1, c]
                span = f32(hi - lo)
                ok = bool(span > 0 and span < INF)
                inv, step = f32(f32(L) / span), f32(span / f32(L))
                t = f32(f32(x[r, c] - lo) * inv)
                t = f32(0) if math.isnan(t) else min(max(t, f32(0)), f32(L))
                q[r, c] = int(np.rint(t)) if ok else 0
                y[r, c] = fmaf(f32(q[r, c]), step, lo).reshape(()) if ok else lo
    return q, y


@pytest.mark.parametrize("nbits,block_rows", [(1, 0), (8, 64), (9, 0), (16, 64)])
def test_restatement_against_a_literal_loop(nbits, block_rows):
    rng = np.random.default_rng(nbits)
    x = (rng.normal(size=(150, 3)) * [1e-3, 1.0, 300.0] + [0.0, 5.0, -100.0]).astype(f32)
    x[7, 0], x[8, 1], x[9, 2], x[70, 1] = NAN, INF, -INF, f32(-0.0)
    x[128:, 2] = f32(4.5)                                   # a constant (block, column) in the blocked form
    rg = R.ranges(x, block_rows)
    assert np.array_equal(bits(rg), bits(_loop_ranges(x, block_rows)))
    q, y = _loop_encode_decode(x, nbits, rg, block_rows)
    codes = R.encode(x, nbits, rg, block_rows)
    assert codes.dtype == (np.uint8 if nbits <= 8 else np.uint16) and np.array_equal(codes, q)
    assert np.array_equal(bits(R.decode(codes, nbits, rg, block_rows)), bits(y))
    assert np.array_equal(bits(R.fake(x, nbits, rg, block_rows)), bits(y))


# ---- 2. the end points, the derived error bound, idempotence ----
def _columns(seed, count, rows=64):
    """Random columns as in §25's prototype: bits 1..16, centres 1e-3 .. 1e3 of either sign, widths 1e-4 .. 1e3."""
    rng = np.random.default_rng(seed)
    for i in range(count):
        nbits = 1 + i % 16
        centre = f32(10.0 ** rng.uniform(-3, 3) * rng.choice([-1.0, 1.0]))
        width = f32(10.0 ** rng.uniform(-4, 3))
        yield nbits, (centre + width * rng.uniform(-0.5, 0.5, size=(rows, 1))).astype(f32)


def test_lo_is_code_0_and_hi_the_last_code():
    for nbits, x in _columns(1, 320):
        rg = R.ranges(x)
        if not rg[0, 1, 0] > rg[0, 0, 0]:
            continue
        q = R.encode(rg[0], nbits, rg)
        assert q[0, 0] == 0 and q[1, 0] == (1 << nbits) - 1, (nbits, rg)


def test_decode_error_within_the_derived_bound():
    """|decode(encode(x)) - x| <= step/2 + 9 ulp(max(|lo|, |hi|)) for finite x in [lo, hi] (the rounding of
    x - lo and of the final fmaf, one ulp(M) each at most; the three roundings of inv, t and step, 2^-24 each on a product of at
    most 2M, less than 6 ulp(M) together; one more for the second-order terms; |rint(t) - t| <= 1/2 is the step/2).  The
    bound is derived, not fitted: the prototype's worst case over such columns was step/2 + 3.1 ulp."""
    worst = 0.0
    for nbits, x in _columns(2, 3400, rows=32):
        rg = R.ranges(x)
        lo, hi = f64(rg[0, 0, 0]), f64(rg[0, 1, 0])
        if not hi > lo:
            continue
        step = f64(R.params(rg[0, 0], rg[0, 1], nbits)[3][0])
        u = float(R.ulp(max(abs(lo), abs(hi))))
        err = np.abs(R.fake(x, nbits, rg).astype(f64) - x.astype(f64)).max()
        worst = max(worst, (err - step / 2) / u)
        assert err <= step / 2 + R.ERROR_ULPS * u, (nbits, lo, hi, err, step, u)
    print(f"worst (error - step/2) / ulp over the columns: {worst:.2f}")


def test_every_code_survives_decode_and_encode():
    """encode(decode(q)) == q for every code of a column with step >= 8 ulp(max(|lo|, |hi|)).  The true condition (§25): the
    decoded value is q·step + lo within one ulp(M), the difference to lo costs at most another, so t = q(1 + 3·2^-24) +- 2 ulp(M)
    / step, and rint(t) = q as long as 2 ulp(M) / step + 3 (2^bits - 1) 2^-24 < 1/2: step > 4.1 ulp(M) suffices at every width.
    Every column below is built to satisfy the asserted condition."""
    rng = np.random.default_rng(3)
    tried = 0
    for i in range(400):
        nbits = 1 + i % 16
        L = (1 << nbits) - 1
        centre = 10.0 ** rng.uniform(-3, 3) * rng.choice([-1.0, 1.0])
        u = float(R.ulp(abs(centre))) * 2                    # the range's end may lie in the next binade
        width = max(10.0 ** rng.uniform(-4, 3), 2.5 * R.IDEMPOTENT_ULPS * u * L)
        rg = np.array([[[centre - width / 2], [centre + width / 2]]], f32)
        step = float(R.params(rg[0, 0], rg[0, 1], nbits)[3][0])
        assert step >= R.IDEMPOTENT_ULPS * float(R.ulp(np.abs(rg).max()))
        q = np.arange(L + 1, dtype=np.uint16 if nbits > 8 else np.uint8).reshape(-1, 1)
        assert np.array_equal(R.encode(R.decode(q, nbits, rg), nbits, rg), q), (nbits, rg)
        tried += 1
    assert tried == 400


# ---- 3. hand values ----
def test_hand_values():
    rg = np.array([[[0.0], [1.0]]], f32)
    x = np.array([[NAN], [INF], [-INF], [0.25], [2.0], [-1.0]], f32)
    assert R.encode(x, 8, rg).reshape(-1).tolist() == [0, 255, 0, 64, 255, 0]
    assert R.encode(x, 16, rg).reshape(-1).tolist() == [0, 65535, 0, 16384, 65535, 0]
    assert R.encode(x, 1, rg).reshape(-1).tolist() == [0, 1, 0, 0, 1, 0]
    # a constant column: span 0, code 0, decodes to lo
    c = np.full((5, 1), 3.25, f32)
    rc = R.ranges(c)
    assert rc.reshape(-1).tolist() == [3.25, 3.25] and not R.encode(c, 8, rc).any()
    assert np.array_equal(bits(R.decode(np.full((5, 1), 200, np.uint8), 8, rc)), bits(c))
    # the span overflows: not ok, code 0, decode gives lo
    big = np.array([[[-3e38], [3e38]]], f32)
    assert not R.encode(np.array([[0.0], [3e38]], f32), 8, big).any()
    assert bits(R.decode(np.array([[7]], np.uint8), 8, big)).tolist() == [[bits(f32(-3e38)).item()]]
    # NaN ranges: not ok; the decode returns lo as it is
    for lo, hi in ((NAN, 1.0), (0.0, NAN), (NAN, NAN), (1.0, 0.0), (-INF, 0.0), (0.0, INF)):
        bad = np.array([[[lo], [hi]]], f32)
        assert not R.encode(np.array([[0.5]], f32), 8, bad).any()
        assert bits(R.decode(np.array([[9]], np.uint8), 8, bad)).tolist() == [[bits(f32(lo)).item()]]
    # codes above 2^bits - 1 read as 2^bits - 1
    assert np.array_equal(bits(R.decode(np.array([[1], [255]], np.uint8), 1, rg)), bits(np.array([[1.0], [1.0]], f32)))
    assert np.array_equal(bits(R.decode(np.array([[511], [65535]], np.uint16), 9, rg)), bits(np.array([[1.0], [1.0]], f32)))


def test_ranges_order_zeros_by_sign_and_skip_what_is_not_finite():
    x = np.array([[0.0, -0.0, NAN, 5.0], [-0.0, 0.0, INF, NAN], [0.0, 0.0, -INF, -5.0]], f32)
    rg = R.ranges(x)
    assert bits(rg[0, 0]).tolist() == [0x80000000, 0x80000000, 0, bits(f32(-5.0))]
    assert bits(rg[0, 1]).tolist() == [0, 0, 0, bits(f32(5.0))]
    # blocked: a ragged last block, an empty array
    y = np.arange(130, dtype=f32).reshape(-1, 1)
    assert R.ranges(y, 64).reshape(-1).tolist() == [0, 63, 64, 127, 128, 129]
    assert R.ranges(np.zeros((0, 2), f32), 64).shape == (0, 2, 2) and R.ranges(np.zeros((0, 2), f32), 0).tolist() == [[[0, 0], [0, 0]]]


def test_subnormals_are_kept():
    tiny = f32(1e-45)                                        # the smallest subnormal
    rg = (np.array([[[0.0], [255.0]]], f32) * tiny).astype(f32)   # 255 subnormal steps
    x = (np.arange(256, dtype=f32) * tiny).astype(f32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        step = R.params(rg[0, 0], rg[0, 1], 8)[3][0]
    assert step == tiny                                      # span / 255 is exact
    # inv = 255 / span overflows to +Inf: t = Inf for x > lo, NaN (0 x Inf) for x = lo -> the codes 0, 255, 255, ...
    assert R.encode(x, 8, rg).reshape(-1).tolist() == [0] + [255] * 255
    assert np.array_equal(bits(R.decode(np.arange(256, dtype=np.uint8).reshape(-1, 1), 8, rg)), bits(x))
    # a subnormal span with a finite inverse (bits = 1: inv = 2^127): subnormal inputs are told apart, the tie goes to even
    rg2 = np.array([[[0.0], [2.0 ** -127]]], f32)
    x2 = np.array([[0.0], [2.0 ** -127], [2.0 ** -128], [3 * 2.0 ** -129], [2.0 ** -149]], f32)
    assert R.encode(x2, 1, rg2).reshape(-1).tolist() == [0, 1, 0, 1, 0]
    assert np.array_equal(bits(R.decode(np.array([[0], [1]], np.uint8), 1, rg2)), bits(rg2[0]))


def test_rint_ties_go_to_even():
    rg = np.array([[[0.0], [255.0]]], f32)                   # inv = step = 1
    x = np.array([[0.5], [1.5], [2.5], [3.5], [254.5], [0.49999997], [2.5000002]], f32)
    assert R.encode(x, 8, rg).reshape(-1).tolist() == [0, 2, 2, 4, 254, 0, 3]


# ---- 4. unit quaternions ----
def test_unit_quaternion_rows():
    q = np.array([[2, 0, 0, 0], [-1, 1, 0, 0], [0, 0, 0, 0], [NAN, 1, 0, 0], [3e38, 3e38, 0, 0], [1e-30, 0, 0, 0], [0, 0, -5, 0],
                  [INF, 0, 0, 0]], f32)
    u = R.unit_quat(q)
    s = f32(1) / np.sqrt(f32(2), dtype=f32)
    want = np.array([[1, 0, 0, 0], [s, -s, -0.0, -0.0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [0, 0, -1, 0],
                     [1, 0, 0, 0]], f32)
    # (1e-30)^2 underflows to 0: not > 0, the identity; (3e38)^2 overflows: not finite, the identity
    assert np.array_equal(u, want), u
    codes = R.encode(q, 8, None, 0, R.UNIT_QUAT)
    assert codes[0].tolist() == [255, 128, 128, 128] and codes[2].tolist() == [255, 128, 128, 128]
    assert codes[1].tolist() == [218, 37, 128, 128] and codes[6].tolist() == [128, 128, 0, 128]


def _rot_angle(a, b):
    a, b = a.astype(f64), b.astype(f64)
    d = np.abs((a * b).sum(1)) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return 2 * np.arccos(np.minimum(d, 1.0))


@pytest.mark.parametrize("nbits", [6, 8, 12, 16])
def test_decoded_rotation_within_the_derived_angle(nbits):
    """Each component of the unit quaternion u moves by at most e = step/2 + 9 ulp(1) = 1/(2^bits - 1) + 9·2^-23 (the bound of
    the linear groups on [-1, 1]), plus the normalisation's own rounding (3 ulp(1) per component), so the decoded u' has
    |u' - u| <= 2 e' with e' = e + 3·2^-23.  For a unit u and any u' the angle between them as 4-vectors satisfies
    sin(angle) <= |u' - u|, and the rotation's angle is twice that: at most 2 asin(2 e')."""
    rng = np.random.default_rng(nbits)
    q = rng.normal(size=(4096, 4)).astype(f32) * rng.uniform(0.1, 10, size=(4096, 1)).astype(f32)
    dec = R.fake(q, nbits, None, 0, R.UNIT_QUAT)
    e = 1.0 / ((1 << nbits) - 1) + 12 * 2.0 ** -23
    bound = 2 * math.asin(2 * e)
    worst = _rot_angle(q, dec).max()
    print(f"bits {nbits}: worst angle {worst:.3e} rad, bound {bound:.3e} rad")
    assert worst <= bound
    assert (dec[:, 0] >= -e).all()                           # w >= 0 up to the quantisation


# ---- 5. the archive, nbytes, what needs no device ----
def _container(pkg, n=300, with_sh=True, seed=0, spec=None):
    Q, S = pkg.quantised_model, pkg.sh_codebook
    rng = np.random.default_rng(seed)
    spec = Q.QuantSpec() if spec is None else spec
    shapes = dict(points=(n, 3), features_dc=(n, 1, 3), features_rest=(n, 15, 3), opacities=(n, 1), scales=(n, 3), rotations=(n, 4))
    codes, ranges = {}, {}
    for g in Q.GROUPS:
        if g == "features_rest" and with_sh:
            continue
        nbits, block_rows = getattr(spec, g)
        cols = int(np.prod(shapes[g][1:]))
        c = rng.integers(0, 1 << nbits, size=(n, cols))
        codes[g] = torch.from_numpy(c.astype(np.uint8)) if nbits <= 8 else torch.from_numpy(c.astype(np.uint16).view(np.int16)).view(torch.uint16)
        ranges[g] = None if g == "rotations" else torch.from_numpy(np.sort(rng.normal(size=(Q.n_blocks(n, block_rows), 2, cols)), axis=1).astype(f32))
    sh = None
    if with_sh:
        idx = torch.from_numpy(rng.integers(0, 4096, n).astype(np.uint16).view(np.int16)).view(torch.uint16)
        sh = S.SHCodebook(torch.from_numpy(rng.normal(size=(4096, 45)).astype(f32)), idx, (n, 15, 3))
    ids = torch.arange(n, dtype=torch.int32)
    return Q.QuantisedModel(n, spec, codes, ranges, {g: shapes[g] for g in codes}, sh=sh, ids=ids)


def _same(a, b):
    v = lambda t: t.view(torch.int16) if t.dtype == torch.uint16 else t   # noqa: E731
    assert a.n == b.n and a.spec == b.spec and a.codes.keys() == b.codes.keys() and a.shapes == b.shapes
    for g in a.codes:
        assert a.codes[g].dtype == b.codes[g].dtype and torch.equal(v(a.codes[g]), v(b.codes[g])), g
        assert (a.ranges[g] is None) == (b.ranges.get(g) is None)
        if a.ranges[g] is not None:
            assert torch.equal(a.ranges[g].view(torch.int32), b.ranges[g].view(torch.int32)), g
    assert (a.sh is None) == (b.sh is None) and torch.equal(a.ids, b.ids)
    if a.sh is not None:
        assert torch.equal(a.sh.codebook, b.sh.codebook) and torch.equal(v(a.sh.indices), v(b.sh.indices)) and a.sh.shape == b.sh.shape


@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("with_sh", [True, False])
def test_archive_round_trip(pkg, tmp_path, compressed, with_sh):
    Q = pkg.quantised_model
    spec = Q.QuantSpec(points=(16, 64), scales=(7, 0), features_rest=(8, 128))
    m = _container(pkg, with_sh=with_sh, spec=spec)
    m.permutation = torch.arange(m.n, dtype=torch.int32)
    path = str(tmp_path / "model.npz")
    m.save(path, compressed=compressed)
    back = Q.QuantisedModel.load(path)
    _same(m, back)
    assert back.permutation is None and back.nbytes == m.nbytes
    with np.load(path, allow_pickle=False) as z:
        assert int(z["format_version"]) == Q.FORMAT_VERSION and z["spec"].tolist() == spec.as_array().tolist()
        assert ("sh_codebook" in z.files) == with_sh and ("features_rest_codes" in z.files) == (not with_sh)


def test_malformed_archives(pkg, tmp_path):
    Q = pkg.quantised_model
    m = _container(pkg, n=70)
    good = str(tmp_path / "good.npz")
    m.save(good)
    with np.load(good) as f:
        z = {k: f[k] for k in f.files}
    junk = tmp_path / "junk.npz"
    junk.write_bytes(b"not an archive at all")
    cut = tmp_path / "cut.npz"
    cut.write_bytes(open(good, "rb").read()[:200])
    for p in (junk, cut):
        with pytest.raises(ValueError):
            Q.QuantisedModel.load(str(p))

    def broken(**change):
        d = {k: v for k, v in {**z, **change}.items() if v is not None}
        p = str(tmp_path / "bad.npz")
        np.savez(p, **d)
        with pytest.raises(ValueError):
            Q.QuantisedModel.load(p)
    broken(format_version=np.asarray(2, np.int64))
    broken(format_version=None)
    broken(spec=z["spec"][:5])
    broken(spec=np.where(z["spec"] == 16, 17, z["spec"]))
    broken(spec=z["spec"].astype(f64))
    broken(n=np.asarray(71, np.int64))
    broken(n=np.asarray(-1, np.int64))
    broken(points_codes=z["points_codes"].astype(np.uint8))
    broken(points_codes=z["points_codes"][:-1])
    broken(points_codes=None)
    broken(points_shape=None)
    broken(points_ranges=z["points_ranges"][:, :1])
    broken(points_ranges=z["points_ranges"].astype(f64))
    broken(opacities_ranges=None)
    broken(rotations_codes=z["rotations_codes"][:, :3])
    broken(sh_indices=z["sh_indices"][:-1])
    broken(sh_indices=z["sh_indices"].astype(np.int32))
    broken(sh_codebook=z["sh_codebook"][:, :44])
    broken(sh_shape=None)
    broken(ids=z["ids"].astype(np.int64))
    broken(features_rest_codes=np.zeros((70, 45), np.uint8), features_rest_shape=np.asarray((70, 15, 3)),
           features_rest_ranges=np.zeros((1, 2, 45), f32))               # both a codebook and the 8-bit group
    with pytest.raises(FileNotFoundError):
        Q.QuantisedModel.load(str(tmp_path / "missing.npz"))
    Q.QuantisedModel.load(good)


def test_nbytes_is_19_bytes_per_gaussian_plus_ranges_and_codebook(pkg):
    n = 1000
    m = _container(pkg, n=n)
    blocks = -(-n // 256)
    ranges = 4 * 2 * (blocks * 3 + 3 + 1 + 3)                # points in blocks of 256; dc, opacity, scales one block; rotations none
    assert m.nbytes == 19 * n + ranges + 4096 * 45 * 4
    assert m.sh.nbytes == 2 * n + 4096 * 45 * 4
    iso = _container(pkg, n=n, with_sh=False)
    assert iso.nbytes == (6 + 3 + 45 + 1 + 3 + 4) * n + ranges + 4 * 2 * 45


def test_spec_and_wrappers_refuse_what_needs_no_device(pkg):
    Q = pkg.quantised_model
    assert Q.QuantSpec().as_array().tolist() == [[16, 256], [8, 0], [8, 0], [8, 0], [8, 0], [8, 0]]
    assert Q.QuantSpec.from_array(Q.QuantSpec(points=(12, 1024)).as_array()) == Q.QuantSpec(points=(12, 1024))
    for kw in (dict(points=(0, 0)), dict(points=(17, 0)), dict(scales=(8, 32)), dict(scales=(8, 96)), dict(scales=(8, 1088)),
               dict(rotations=(8, 64))):
        with pytest.raises(ValueError):
            Q.QuantSpec(**kw)
    x = torch.zeros((4, 3))
    with pytest.raises(ValueError):
        Q.quant_ranges(x)                                    # no CPU path
    with pytest.raises(TypeError):
        Q.quant_ranges(x.double())
    with pytest.raises(ValueError):
        Q.quant_encode(x, 8, torch.zeros((1, 2, 3)))
    with pytest.raises(TypeError):
        Q.quant_decode(torch.zeros((4, 3), dtype=torch.uint8), 9, torch.zeros((1, 2, 3)))
    with pytest.raises(RuntimeError):
        Q.FakeQuantizer().apply(None)
    assert pkg._lib.QUANT_MAX_GROUPS == 8
    assert pkg.quantised_model is Q


def test_error_codes_that_need_no_device(pkg):
    L = pkg._lib
    lib, bad = L.load(), L.GSR_E_INVALID_ARG
    A = 1 << 20                                              # an aligned, never dereferenced address
    rng_ = lib.gsr_quant_ranges
    enc, dec, fake = lib.gsr_quant_encode, lib.gsr_quant_decode, lib.gsr_quant_fake
    for n, cols, br in ((-1, 3, 0), (1 << 31, 3, 0), (8, 0, 0), (8, 49, 0), (8, 3, 32), (8, 3, 63), (8, 3, 96), (8, 3, 1088), (8, 3, -64)):
        assert rng_(n, cols, A, br, A, None) == bad, (n, cols, br)
        assert enc(n, cols, 8, 0, A, br, A, A, None) == bad and dec(n, cols, 8, 0, A, br, A, A, None) == bad, (n, cols, br)
    assert rng_(8, 3, None, 0, A, None) == bad and rng_(8, 3, A, 0, None, None) == bad
    assert rng_(8, 3, A + 2, 0, A, None) == bad and rng_(8, 3, A, 0, A + 1, None) == bad
    assert rng_(0, 3, None, 64, None, None) == 0            # no block: nothing to write
    for nbits, kind, cols in ((0, 0, 3), (17, 0, 3), (8, 2, 3), (8, -1, 3), (8, 1, 3)):
        assert enc(8, cols, nbits, kind, A, 0, A, A, None) == bad and dec(8, cols, nbits, kind, A, 0, A, A, None) == bad
    assert enc(8, 3, 8, 0, None, 0, A, A, None) == bad and enc(8, 3, 8, 0, A, 0, None, A, None) == bad and enc(8, 3, 8, 0, A, 0, A, None, None) == bad
    assert enc(8, 3, 8, 0, A + 1, 0, A, A, None) == bad and enc(8, 3, 8, 0, A, 0, A + 2, A, None) == bad and enc(8, 3, 9, 0, A, 0, A, A + 1, None) == bad
    assert dec(8, 3, 8, 0, None, 0, A, A, None) == bad and dec(8, 3, 8, 0, A, 0, None, A, None) == bad and dec(8, 3, 8, 0, A, 0, A, None, None) == bad
    assert dec(8, 3, 8, 0, A, 0, A, A + 2, None) == bad and dec(8, 3, 16, 0, A + 1, 0, A, A, None) == bad
    assert b"2-byte" in lib.gsr_last_error_string()
    assert enc(0, 3, 8, 0, None, 0, None, None, None) == 0 and dec(0, 4, 8, 1, None, 0, None, None, None) == 0

    def group(rows_in=A, rows_out=A, cols=3, nbits=8, kind=0, br=0, ranges=A):
        return L.QuantGroup(rows_in, rows_out, cols, nbits, kind, br, ranges)
    one = (L.QuantGroup * 1)
    assert fake(None, 1, 8, None) == bad and fake(one(group()), -1, 8, None) == bad
    assert fake((L.QuantGroup * 9)(*[group()] * 9), 9, 8, None) == bad and b"[0, 8]" in lib.gsr_last_error_string()
    for kw in (dict(rows_in=None), dict(rows_out=None), dict(ranges=None), dict(cols=0), dict(cols=49), dict(nbits=0), dict(nbits=17),
               dict(kind=2), dict(kind=1), dict(br=100), dict(rows_in=A + 1), dict(rows_out=A + 2), dict(ranges=A + 3)):
        assert fake(one(group(**kw)), 1, 8, None) == bad, kw
    assert fake(one(group()), 1, -1, None) == bad and fake(one(group()), 1, 1 << 31, None) == bad
    assert fake(one(group(rows_in=None, rows_out=None, ranges=None)), 1, 0, None) == 0 and fake(None, 0, 8, None) == 0
    assert lib.gsr_abi_version() == 6
