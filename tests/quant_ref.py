"""numpy restatement of the quantised model container (csrc/quant.hip, include/gsr.h gsr_quant_*): every
operation one rounded fp32 operation with subnormals kept, the decode's fused operation through the exact `fmaf` emulation of
tests/vq_ref.py.  tests/test_quant_cpu.py holds this file to a literal per-element loop; tests/test_gpu_quant.py holds the
kernels to this file with array_equal on integers and float bits."""
import numpy as np

from vq_ref import fmaf

f32, f64, u32 = np.float32, np.float64, np.uint32
LINEAR, UNIT_QUAT = 0, 1


def keys(x):
    """The monotone integer key of the bits: unsigned order = -Inf < ... < -0 < +0 < ... < +Inf."""
    b = np.ascontiguousarray(x, f32).view(u32)
    return np.where(b >> 31 != 0, ~b, b ^ u32(0x80000000)).astype(u32)


def unkeys(k):
    k = np.asarray(k, u32)
    return np.where(k >> 31 != 0, k ^ u32(0x80000000), ~k).astype(u32).view(f32)


def n_blocks(n, block_rows):
    return 1 if block_rows == 0 else -(-n // block_rows)


def ranges(rows, block_rows=0):
    """(n_blocks, 2, cols): lo / hi over the finite values of every (block, column) in key order; none: +0, +0."""
    x = np.ascontiguousarray(rows, f32)
    n, cols = x.shape
    nb = n_blocks(n, block_rows)
    out = np.zeros((nb, 2, cols), f32)
    step = block_rows if block_rows else max(n, 1)
    for b in range(nb):
        blk = x[b * step:(b + 1) * step]
        if blk.shape[0] == 0:
            continue
        k, fin = keys(blk), np.isfinite(blk)
        kmin = np.where(fin, k, u32(0xFFFFFFFF)).min(axis=0)
        kmax = np.where(fin, k, u32(0)).max(axis=0)
        any_ = fin.any(axis=0)
        out[b, 0] = np.where(any_, unkeys(kmin), f32(0))
        out[b, 1] = np.where(any_, unkeys(kmax), f32(0))
    return out


def _expand(rg, n, cols, block_rows, kind):
    """lo, hi as (n, cols) arrays."""
    if kind == UNIT_QUAT:
        return np.full((n, cols), -1, f32), np.full((n, cols), 1, f32)
    rg = np.asarray(rg, f32)
    b = np.arange(n) // block_rows if block_rows else np.zeros(n, np.int64)
    return rg[b, 0, :], rg[b, 1, :]


def params(lo, hi, bits):
    """-> ok, Lf, inv, step (float32 arrays of lo's shape)."""
    with np.errstate(all="ignore"):
        span = (np.asarray(hi, f32) - np.asarray(lo, f32)).astype(f32)
        ok = (span > 0) & (span < np.inf)
        Lf = f32((1 << bits) - 1)
        inv = (Lf / span).astype(f32)
        step = (span / Lf).astype(f32)
    return ok, Lf, inv, step


def unit_quat(rows):
    """Rows (w, x, y, z) normalised with w >= 0; a row whose squared norm is not > 0 or not finite becomes (1, 0, 0, 0)."""
    q = np.ascontiguousarray(rows, f32)
    with np.errstate(all="ignore"):
        w, x, y, z = (q[:, k] for k in range(4))
        n2 = ((((w * w).astype(f32) + (x * x).astype(f32)).astype(f32) + (y * y).astype(f32)).astype(f32) + (z * z).astype(f32)).astype(f32)
        good = (n2 > 0) & (n2 < np.inf)
        inv = (f32(1) / np.sqrt(n2, dtype=f32)).astype(f32)
        s = np.where(w < 0, -inv, inv).astype(f32)
        u = (q * s[:, None]).astype(f32)
    ident = np.array([1, 0, 0, 0], f32)
    return np.where(good[:, None], u, ident).astype(f32)


def encode(rows, bits, rg=None, block_rows=0, kind=LINEAR):
    x = np.ascontiguousarray(rows, f32)
    n, cols = x.shape
    if kind == UNIT_QUAT:
        x = unit_quat(x)
    lo, hi = _expand(rg, n, cols, block_rows, kind)
    ok, Lf, inv, _ = params(lo, hi, bits)
    with np.errstate(all="ignore"):
        t = ((x - lo).astype(f32) * inv).astype(f32)
        t = np.where(np.isnan(t), f32(0), np.fmin(np.fmax(t, f32(0)), Lf)).astype(f32)
        q = np.rint(t).astype(np.int64)
    return np.where(ok, q, 0).astype(np.uint8 if bits <= 8 else np.uint16)


def decode(codes, bits, rg=None, block_rows=0, kind=LINEAR):
    q = np.asarray(codes)
    n, cols = q.shape
    lo, hi = _expand(rg, n, cols, block_rows, kind)
    ok, _, _, step = params(lo, hi, bits)
    qf = np.minimum(q.astype(np.int64), (1 << bits) - 1).astype(f32)
    return np.where(ok, fmaf(qf, step, lo), lo).astype(f32)


def fake(rows, bits, rg=None, block_rows=0, kind=LINEAR):
    return decode(encode(rows, bits, rg, block_rows, kind), bits, rg, block_rows, kind)


def ulp(x):
    """The spacing of float32 at |x| (float64), of the smallest normal's binade below it."""
    a = np.maximum(np.abs(np.asarray(x, f64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


ERROR_ULPS = 9       # |decode(encode(x)) - x| <= step / 2 + ERROR_ULPS * ulp(max(|lo|, |hi|))   
IDEMPOTENT_ULPS = 8  # encode(decode(q)) == q is asserted where step >= IDEMPOTENT_ULPS * ulp(max(|lo|, |hi|))
