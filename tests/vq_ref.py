"""numpy restatement of the SH codebook k-means (csrc/vq.hip, include/gsr.h gsr_vq_*): every operation one rounded
fp32 operation, the fused ones through an exact emulation of C `fmaf`.  tests/test_vq_cpu.py pins the emulation to a compiled
`fmaf`; tests/test_gpu_vq.py holds the kernels to this file with array_equal.

fmaf without an fma: the product of two float32 is exact in float64 (48 significant bits), the float64 sum with c rounds once,
TwoSum gives that rounding's error e, and where e != 0 and the sum's last mantissa bit is even the sum is stepped one bit
pattern towards e: the float64 is now the exact value rounded to ODD, and rounding that to float32 (29 bits fewer) is the
correct single rounding of a*b + c.  The naive float32(float64(a)*b + c) rounds twice and is wrong next to fp32 midpoints."""
import numpy as np

f32, f64 = np.float32, np.float64
ONE = float(1 << 24)   # the fixed point of the sums: q = rne(clamp(x, -128, 128) * 2^24)


def fmaf(a, b, c):
    """C fmaf(a, b, c) on float32 arrays (broadcasting), bit for bit."""
    a, b, c = np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32)
    with np.errstate(all="ignore"):
        p = a.astype(f64) * b.astype(f64)
        c64 = c.astype(f64)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)
        bits = np.atleast_1d(s).view(np.int64).copy()
        fix = np.atleast_1d(np.isfinite(s) & np.isfinite(e) & (e != 0)) & ((bits & 1) == 0)
        # towards e: the magnitude's bit pattern grows when e has the sign of s
        step = np.where(np.atleast_1d((e > 0) == (s > 0)), 1, -1)
        bits = np.where(fix, bits + step, bits)
        out = bits.view(f64).reshape(np.shape(s)).astype(f32)
    return out


def fmaf_naive(a, b, c):
    a, b, c = np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32)
    with np.errstate(all="ignore"):
        return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def half_norms(codebook):
    """h_j = 0.5f * n2_j, n2_j = fmaf(c_jd, c_jd, n2_j), d ascending from 0."""
    c = np.asarray(codebook, f32)
    n2 = np.zeros(c.shape[0], f32)
    for d in range(c.shape[1]):
        n2 = fmaf(c[:, d], c[:, d], n2)
    return (f32(0.5) * n2).astype(f32)


def scores(rows, codebook):
    """t_ij (n, K): fmaf(x_id, c_jd, t_ij), d ascending, from -h_j."""
    x, c = np.asarray(rows, f32), np.asarray(codebook, f32)
    t = np.broadcast_to(-half_norms(c), (x.shape[0], c.shape[0])).astype(f32)
    for d in range(x.shape[1]):
        t = fmaf(x[:, d:d + 1], c[None, :, d], t)
    return t


def argbest(t):
    """The lowest j whose t_ij is not NaN and is >= every non-NaN t_ik; 0 when every t_ik is NaN."""
    valid = ~np.isnan(t)
    with np.errstate(all="ignore"):
        m = np.max(np.where(valid, t, -np.inf), axis=1)
    cand = valid & (t == m[:, None])
    return np.argmax(cand, axis=1).astype(np.uint16)   # the first True; 0 when there is none


def residual(rows, codebook, indices):
    """err_i: r = x_id - c_jd ; err = fmaf(r, r, err), d ascending from 0."""
    x, c = np.asarray(rows, f32), np.asarray(codebook, f32)[np.asarray(indices, np.int64)]
    err = np.zeros(x.shape[0], f32)
    with np.errstate(all="ignore"):
        for d in range(x.shape[1]):
            r = (x[:, d] - c[:, d]).astype(f32)
            err = fmaf(r, r, err)
    return err


def assign(rows, codebook, prev=None, chunk=4096):
    """-> (indices uint16 (n,), err float32 (n,), changed int).  prev None: every row counts as changed."""
    x = np.asarray(rows, f32)
    idx = np.zeros(x.shape[0], np.uint16)
    for a in range(0, x.shape[0], chunk):
        idx[a:a + chunk] = argbest(scores(x[a:a + chunk], codebook))
    changed = x.shape[0] if prev is None else int(np.count_nonzero(idx != np.asarray(prev, np.uint16)))
    return idx, residual(x, codebook, idx), changed


def quantise(rows):
    """rne(clamp(x, -128, 128) * 2^24) as int64; NaN counts as 0."""
    x = np.asarray(rows, f32)
    with np.errstate(all="ignore"):
        q = np.rint(np.clip(x, f32(-128), f32(128)).astype(f32) * f32(ONE))
    return np.where(np.isnan(x), 0, q).astype(np.int64)


def accumulate(rows, indices, n_codes, wq=None, sums=None, wsum=None):
    """sums (K, dim) int64 += wq_i * q(x_i), wsum (K,) uint64 += wq_i; both accumulated into (new zero arrays when None)."""
    q = quantise(rows)
    n, dim = q.shape
    w = np.ones(n, np.int64) if wq is None else np.asarray(wq, np.uint8).astype(np.int64)
    sums = np.zeros((n_codes, dim), np.int64) if sums is None else sums
    wsum = np.zeros(n_codes, np.uint64) if wsum is None else wsum
    j = np.minimum(np.asarray(indices, np.int64), n_codes - 1)
    np.add.at(sums, j, q * w[:, None])
    ws = wsum.view(np.int64)
    np.add.at(ws, j, w)
    return sums, wsum


def update(codebook, sums, wsum):
    """-> (new codebook, empty): c_jd = float32(float64(sums) / (float64(wsum) * 2^24)) where wsum > 0, else the old row."""
    c = np.asarray(codebook, f32).copy()
    live = wsum > 0
    with np.errstate(all="ignore"):
        new = (sums.astype(f64) / (wsum.astype(f64)[:, None] * ONE)).astype(f32)
    c[live] = new[live]
    return c, int(np.count_nonzero(~live))


def default_init(rows, n_codes):
    n = rows.shape[0]
    return np.asarray(rows, f32)[(np.arange(n_codes, dtype=np.int64) * n) // n_codes].copy()


def fit(rows, n_codes, iters, wq=None, init=None):
    """The chain of fit_sh_codebook: per iteration assign, clear, accumulate, update; a last assign.
    -> (codebook, indices, history (iters, 2) uint32: changed, empty)."""
    x = np.asarray(rows, f32)
    c = default_init(x, n_codes) if init is None else np.asarray(init, f32).copy()
    hist = np.zeros((iters, 2), np.uint32)
    prev = None
    for it in range(iters):
        idx, _, changed = assign(x, c, prev)
        sums, wsum = accumulate(x, idx, n_codes, wq)
        c, empty = update(c, sums, wsum)
        hist[it] = (changed, empty)
        prev = idx
    idx, _, _ = assign(x, c, prev)
    return c, idx, hist


def weights_from_scores(weight_sum):
    """uint8: max(1, ceil(255 * s / max s)); all ones when max s is 0."""
    s = np.asarray(weight_sum, f64)
    m = s.max() if s.size else 0.0
    if not m > 0:
        return np.ones(s.shape, np.uint8)
    return np.maximum(1, np.ceil(255.0 * s / m)).astype(np.uint8)
