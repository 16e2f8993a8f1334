"""numpy restatement of gsr_vq_group / gsr_vq_codebook_grad (include/gsr.h): the stable grouping of the rows by
code and the fixed-order per-code gradient sums.  Plain float32 adds, one rounding each; no product code, no torch."""
import re
import os

import numpy as np

f32 = np.float32
_HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gsr.h")
RADIX = int(re.search(r"#define\s+GSR_VQ_SUM_RADIX\s+(\d+)", open(_HDR).read()).group(1))   # the header's, the one constant


def group(indices, n_codes):
    """(order, offsets): c_i = min(indices[i], K - 1); order = the rows sorted by (c_i, i); offsets[j] = #{i : c_i < j}."""
    c = np.minimum(np.asarray(indices).astype(np.int64), n_codes - 1)
    order = np.argsort(c, kind="stable").astype(np.uint32)
    counts = np.bincount(c, minlength=n_codes)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return order, offsets


def _chunk_sums(vals, seg):
    """One level: `vals` (m, dim) float32 are the lists of all codes back to back, `seg` (K + 1) their bounds.  Returns the
    chunk sums back to back and their bounds.  A list of one entry passes through untouched (a chunk of one is that value)."""
    K = seg.size - 1
    lens = np.diff(seg)
    n_chunks = -(-lens // RADIX)
    new_seg = np.concatenate([[0], np.cumsum(n_chunks)]).astype(np.int64)
    total = int(new_seg[-1])
    code = np.repeat(np.arange(K), n_chunks)                       # the code of every chunk
    first = seg[:-1][code] + RADIX * (np.arange(total) - new_seg[:-1][code])
    length = np.minimum(RADIX, seg[1:][code] - first)
    out = vals[first].copy() if total else np.zeros((0, vals.shape[1]), f32)
    for t in range(1, RADIX):                                      # s = s + L[t], ascending, one rounded add each
        live = np.flatnonzero(length > t)
        if live.size == 0:
            break
        out[live] = out[live] + vals[first[live] + t]
    return out, new_seg


def codebook_grad(g_rows, order, offsets, n_codes):
    """g_codebook (K, dim) float32 of the definition; g_rows (n, dim) float32."""
    g = np.ascontiguousarray(g_rows, f32)
    n, dim = g.shape
    seg = np.minimum(np.asarray(offsets).astype(np.int64), n)
    vals = g[np.minimum(np.asarray(order).astype(np.int64), max(n - 1, 0))] if n else g
    out = np.zeros((n_codes, dim), f32)                            # an empty code: +0.0
    with np.errstate(all="ignore"):
        while True:
            lens = np.diff(seg)
            if (lens <= 1).all():
                break
            vals, seg = _chunk_sums(vals, seg)
    one = np.flatnonzero(np.diff(seg) == 1)
    out[one] = vals[seg[:-1][one]]
    return out


def codebook_grad_literal(g_rows, indices, n_codes):
    """The definition as a Python loop per code, column and chunk — for small cases."""
    g = np.ascontiguousarray(g_rows, f32)
    n, dim = g.shape
    c = [min(int(v), n_codes - 1) for v in indices]
    out = np.zeros((n_codes, dim), f32)

    def reduce(L):
        if len(L) == 1:
            return L[0]
        chunks = []
        for c0 in range(0, len(L), RADIX):
            s = L[c0]
            for v in L[c0 + 1:c0 + RADIX]:
                s = f32(s + v)
            chunks.append(s)
        return reduce(chunks)

    with np.errstate(all="ignore"):
        for j in range(n_codes):
            rows = [i for i in range(n) if c[i] == j]
            for d in range(dim):
                if rows:
                    out[j, d] = reduce([g[i, d] for i in rows])
    return out


def levels(n):
    """The number of levels the library launches for n rows: ceil(log_R n), at least one."""
    l, span = 1, RADIX
    while span < n:
        l, span = l + 1, span * RADIX
    return l
