"""SH codebook compression: features_rest vector-quantised by an exact k-means on the device (include/gsr.h gsr_vq_*;
csrc/vq.hip).  No reference counterpart.  It is the step that follows pruning by contribution scores
(contribution.py) in LightGaussian (Fan et al. 2023), Compact3D (Navaneet et al. 2023) and "Compressed 3D Gaussian Splatting"
(Niedermayr et al. 2024): at SH degree 3, 45 of a Gaussian's 59 floats are features_rest.

  fit_sh_codebook(features_rest, n_codes, iters=10, weights=None, init=None)  -> SHCodebook
  weights_from_scores(weight_sum)        uint8 weights from ContributionScores.weight_sum
  SHCodebook.decode() / save(path) / load(path) / nbytes
  compress_features_rest(model_or_tensor, n_codes, ...)   the one-call form
  SHCodebook.groups() / codebook_grad(g, sh) / decode_features_rest(codebook, sh) / SHCodebookFineTuner(sh)
                                         fine-tuning through the codebook (csrc/vq_grad.hip)

features_rest (N, K-1, 3) is, row by row, the (n, dim) matrix of gsr_vq_* with dim = 3·(K-1).  The nearest-code search runs on
the f32 matrix cores and is bit for bit the fp32 definition of the header; the sums are integers: a fit is the same bits in
every run.  Seeding is deterministic (rows (j·n) // K) — k-means++ is out of scope."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import optim

MAX_DIM, MAX_CODES, MAX_ROWS = 48, 65536, (1 << 24) - 1


def weights_from_scores(weight_sum: torch.Tensor) -> torch.Tensor:
    """uint8 weights of gsr_vq_accumulate from §22's weight_sum: max(1, ceil(255·s / max s)) — a Gaussian no view uses still
    needs a code, so nothing weighs 0.  All ones when no score is positive.  Elementwise torch on the scores' device, no
    read-back."""
    s = weight_sum.to(torch.float64)
    if s.numel() == 0:
        return torch.empty(0, dtype=torch.uint8, device=s.device)
    m = s.max()
    w = torch.ceil(255.0 * s / torch.where(m > 0, m, torch.ones_like(m)))
    return torch.where(m > 0, w.clamp(min=1.0, max=255.0), torch.ones_like(w)).to(torch.uint8)


def _rows_of(features_rest: torch.Tensor):
    if not isinstance(features_rest, torch.Tensor) or features_rest.dtype != torch.float32:
        raise TypeError("features_rest must be a float32 tensor")
    if features_rest.device.type != "cuda":
        raise ValueError("the codebook is fitted on the HIP device (no CPU path)")
    if features_rest.dim() < 2:
        raise ValueError("features_rest must be (N, K-1, 3) or (n, dim)")
    shape = tuple(int(v) for v in features_rest.shape)
    n = shape[0]
    dim = int(np.prod(shape[1:]))
    if not 1 <= dim <= MAX_DIM:
        raise ValueError(f"row length {dim}: 1 .. {MAX_DIM}")
    if n > MAX_ROWS:
        raise ValueError(f"{n} rows: at most {MAX_ROWS}")
    return features_rest.contiguous().view(n, dim), shape


class SHCodebook:
    """A fitted codebook: `codebook` (K, D) float32, `indices` (n,) torch.uint16, `shape` of the features_rest it stands for,
    `history` (iterations, 2) uint32 host tensor — per Lloyd iteration the rows that changed code and the empty codes."""

    def __init__(self, codebook, indices, shape, history=None):
        self.codebook, self.indices, self.shape = codebook, indices, tuple(int(v) for v in shape)
        self.history = history if history is not None else torch.zeros((0, 2), dtype=torch.uint32)

    @property
    def n_codes(self) -> int:
        return int(self.codebook.shape[0])

    @property
    def nbytes(self) -> int:
        """Bytes of the compressed form: the codebook's floats and the uint16 indices."""
        return self.codebook.numel() * 4 + self.indices.numel() * 2

    def decode(self, codebook=None) -> torch.Tensor:
        """features_rest in the model's layout: row i is codebook[indices[i]] (gsr_vq_decode).  `codebook`: other code rows
        of the same shape in place of the object's own."""
        cb = self.codebook if codebook is None else codebook
        if codebook is not None and not (cb.dtype == torch.float32 and cb.is_contiguous() and cb.shape == self.codebook.shape
                                         and cb.device == self.indices.device):
            raise ValueError(f"codebook must be a contiguous float32 {tuple(self.codebook.shape)} tensor on the indices' device")
        n, dim = int(self.indices.shape[0]), int(cb.shape[1])
        out = torch.empty((n, dim), dtype=torch.float32, device=cb.device)
        if n:
            with torch.cuda.device(cb.device):
                L.check(L.load().gsr_vq_decode(n, self.n_codes, dim, L.ptr(cb), L.ptr(self.indices), L.ptr(out), L.stream()))
        return out.view(self.shape)

    def groups(self):
        """(order, offsets) of gsr_vq_group, int32 device tensors holding the uint32 words: the rows sorted by (code, row) and
        the first position of every code, n and K + 1 entries.  Built once and kept; built again when `indices` is replaced
        by another tensor (an in-place change of the indices needs `invalidate_groups()`)."""
        cached = getattr(self, "_groups", None)
        if cached is not None and cached[0] is self.indices:
            return cached[1], cached[2]
        idx = self.indices
        if idx.device.type != "cuda":
            raise ValueError("the rows are grouped on the HIP device (no CPU path)")
        n, K = int(idx.shape[0]), self.n_codes
        order = torch.empty(n, dtype=torch.int32, device=idx.device)
        offsets = torch.zeros(K + 1, dtype=torch.int32, device=idx.device)
        if n:
            lib = L.load()
            nb = int(lib.gsr_vq_group_scratch_bytes(n, K))
            scratch = torch.empty(nb, dtype=torch.uint8, device=idx.device)
            with torch.cuda.device(idx.device):
                L.check(lib.gsr_vq_group(n, K, L.ptr(idx), L.ptr(order), L.ptr(offsets), L.ptr(scratch), nb, L.stream()))
        self._groups = (idx, order, offsets)
        self._grad_scratch = None
        return order, offsets

    def invalidate_groups(self) -> None:
        self._groups = None

    def save(self, path) -> None:
        """A numpy.savez archive: codebook float32 (K, D), indices uint16 (n,), shape int64."""
        np.savez(path, codebook=self.codebook.detach().cpu().numpy(), indices=self.indices.cpu().view(torch.int16).numpy().view(np.uint16),
                 shape=np.asarray(self.shape, np.int64))

    @classmethod
    def load(cls, path, device="cpu") -> "SHCodebook":
        with np.load(path) as z:
            cb, idx, shape = z["codebook"], z["indices"], z["shape"]
        if cb.dtype != np.float32 or cb.ndim != 2 or idx.dtype != np.uint16 or idx.ndim != 1:
            raise ValueError("not an SH codebook archive")
        if idx.size != int(shape[0]) or int(np.prod(shape[1:])) != cb.shape[1]:
            raise ValueError("archive shape does not match its codebook and indices")
        indices = torch.from_numpy(idx.view(np.int16).copy()).view(torch.uint16)
        return cls(torch.from_numpy(cb.copy()).to(device), indices.to(device), shape)


def fit_sh_codebook(features_rest: torch.Tensor, n_codes: int, iters: int = 10, weights=None, init=None,
                    stop_when_unchanged: bool = False) -> SHCodebook:
    """Lloyd's k-means of the rows of `features_rest` on the device.  One iteration is gsr_vq_assign, clearing the sums,
    gsr_vq_accumulate, gsr_vq_update, in that order; a last assign follows the final update, so `indices` belongs to
    `codebook`.  `weights`: uint8 (n) or None (all 1).  `init`: (n_codes, dim) float32 or None — the rows (j·n) // n_codes.
    The `changed` / `empty` counters of all iterations land in ONE device tensor that is read back once at the end: no
    per-iteration synchronisation, unless `stop_when_unchanged` (one word read per iteration; stops at the first iteration
    whose assign changes nothing, and `history` is cut there)."""
    rows, shape = _rows_of(features_rest)
    n, dim = rows.shape
    n_codes, iters = int(n_codes), int(iters)
    if not 1 <= n_codes <= MAX_CODES:
        raise ValueError(f"n_codes = {n_codes}: 1 .. {MAX_CODES}")
    if iters < 0:
        raise ValueError("negative iters")
    if n == 0:
        raise ValueError("no rows to fit")
    dev = rows.device
    if init is None:
        pick = (torch.arange(n_codes, dtype=torch.int64, device=dev) * n) // n_codes
        codebook = rows[pick].contiguous()
    else:
        if tuple(init.shape) != (n_codes, dim) or init.dtype != torch.float32:
            raise ValueError(f"init must be float32 ({n_codes}, {dim})")
        codebook = init.to(dev).contiguous().clone()
    if weights is not None:
        if weights.dtype != torch.uint8 or tuple(weights.shape) != (n,):
            raise ValueError(f"weights must be uint8 ({n},)")
        weights = weights.to(dev).contiguous()
    lib = L.load()
    indices = torch.zeros(n, dtype=torch.uint16, device=dev)
    sums = torch.empty((n_codes, dim), dtype=torch.int64, device=dev)
    wsum = torch.empty(n_codes, dtype=torch.int64, device=dev)
    hist = torch.zeros((max(iters, 1), 2), dtype=torch.int32, device=dev)   # uint32 words: [it, 0] changed, [it, 1] empty
    nb = int(lib.gsr_vq_scratch_bytes(n, n_codes, dim))
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    done = 0
    with torch.cuda.device(dev):
        st = L.stream()

        def assign(prev, changed):
            L.check(lib.gsr_vq_assign(n, n_codes, dim, L.ptr(rows), L.ptr(codebook), prev, L.ptr(indices), None, changed,
                                      L.ptr(scratch), nb, st))

        for it in range(iters):
            word = hist.data_ptr() + 8 * it
            assign(L.ptr(indices) if it else None, word)
            if stop_when_unchanged and it and int(hist[it, 0]) == 0:
                break
            sums.zero_(); wsum.zero_()
            L.check(lib.gsr_vq_accumulate(n, n_codes, dim, L.ptr(rows), L.ptr(indices), L.ptr(weights), L.ptr(sums), L.ptr(wsum), st))
            L.check(lib.gsr_vq_update(n_codes, dim, L.ptr(sums), L.ptr(wsum), L.ptr(codebook), word + 4, st))
            done = it + 1
        else:
            assign(L.ptr(indices) if iters else None, None)
    history = hist[:done].cpu().view(torch.uint32)   # the one read-back
    return SHCodebook(codebook, indices, shape, history)


def compress_features_rest(model_or_tensor, n_codes: int, iters: int = 10, weights=None, scores=None, **kw) -> SHCodebook:
    """fit_sh_codebook of a model's `features_rest` (or of the tensor itself).  `scores`: a ContributionScores of this model —
    its weight_sum becomes the weights (weights_from_scores).  The model is not changed: `model.features_rest =
    result.decode()` puts the quantised values in place.  Out of scope: the other attributes, and rendering from indices."""
    fr = getattr(model_or_tensor, "features_rest", model_or_tensor)
    if scores is not None:
        if weights is not None:
            raise ValueError("give weights or scores, not both")
        if scores.n != int(fr.shape[0]):
            raise ValueError(f"scores of {scores.n} Gaussians on a model of {int(fr.shape[0])}")
        weights = weights_from_scores(scores.weight_sum)
    return fit_sh_codebook(fr, n_codes, iters=iters, weights=weights, **kw)


# ---- fine-tuning through the codebook ----
def _grad_rows(g: torch.Tensor, n: int, dim: int):
    """(tensor to keep alive, row stride in floats) of a gradient of features_rest: contiguous, or a view whose rows are
    contiguous and lie stride(0) >= dim floats apart — `vshs[:, 1:, :]` of the (N, K, 3) gradient — read in place."""
    if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.device.type != "cuda":
        raise ValueError("the gradient must be a float32 HIP device tensor")
    if g.dim() < 2 or int(g.shape[0]) != n or int(np.prod(g.shape[1:])) != dim:
        raise ValueError(f"gradient of shape {tuple(g.shape)} for {n} rows of {dim}")
    if n == 0 or g.is_contiguous():
        return g, dim
    inner = g[0]
    if inner.is_contiguous() and g.stride(0) >= dim:
        return g, int(g.stride(0))
    return g.contiguous(), dim


def codebook_grad(g_features_rest: torch.Tensor, sh: SHCodebook, out=None) -> torch.Tensor:
    """∇codebook (K, D) of `features_rest = sh.decode()`: row j is the sum of the gradient rows of code j's Gaussians in the
    fixed order of include/gsr.h (gsr_vq_codebook_grad) — the same bits in every run, no float atomics.  The gradient is the
    contiguous (N, K-1, 3) array or the strided view `vshs[:, 1:, :]` of gsr_backward's (N, K, 3) gradient, read in place.
    `out`: a contiguous float32 (K, D) tensor, fully overwritten.  No synchronisation."""
    n, K, dim = int(sh.indices.shape[0]), sh.n_codes, int(sh.codebook.shape[1])
    g, stride = _grad_rows(g_features_rest, n, dim)
    if out is None:
        out = torch.empty((K, dim), dtype=torch.float32, device=sh.codebook.device)
    elif not (out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (K, dim) and out.device == g.device):
        raise ValueError(f"out must be a contiguous float32 ({K}, {dim}) tensor on the gradient's device")
    if n == 0:
        return out.zero_()
    order, offsets = sh.groups()
    lib = L.load()
    scratch = getattr(sh, "_grad_scratch", None)
    if scratch is None:
        scratch = sh._grad_scratch = torch.empty(int(lib.gsr_vq_codebook_grad_scratch_bytes(n, K, dim)), dtype=torch.uint8,
                                                 device=order.device)
    with torch.cuda.device(order.device):
        L.check(lib.gsr_vq_codebook_grad(n, K, dim, L.ptr(g), stride, L.ptr(order), L.ptr(offsets), L.ptr(out), L.ptr(scratch),
                                         scratch.numel(), L.stream()))
    return out


class _DecodeFeaturesRest(torch.autograd.Function):
    @staticmethod
    def forward(ctx, codebook, sh):
        ctx.sh = sh
        return sh.decode(codebook.detach().contiguous())

    @staticmethod
    def backward(ctx, g):
        return codebook_grad(g, ctx.sh), None


def decode_features_rest(codebook: torch.Tensor, sh: SHCodebook) -> torch.Tensor:
    """`sh.decode()` from the code rows `codebook` (K, D), differentiable in them: forward gsr_vq_decode, backward
    gsr_vq_codebook_grad.  `rasterize(...)` of shs built from it is differentiable down to the code rows; `sh.indices` carries
    no gradient."""
    return _DecodeFeaturesRest.apply(codebook, sh)


class SHCodebookFineTuner:
    """Training through the codebook: the indices fixed, the K code rows the parameters (the third step of LightGaussian,
    Compact3D and "Compressed 3D Gaussian Splatting").  `codebook` is `sh.codebook` itself, updated in place; `optimizer` is
    its optim.Adam — lr: the reference's features_rest rate (training.jl:236), eps: its 1e-15.

      features_rest()          the decode to hand to the rasterizer
      step(g_features_rest)    codebook_grad + one Adam step of the code rows; no synchronisation

    The step without autograd: `backward_raw`, then `tuner.step(vshs[:, 1:, :])`, then `trainer_tail_step` for the other
    groups.  The tail steps every group it is given: hand it, as `features_rest`, the decoded tensor with a throw-away Adam
    whose lr is 0.0 — its update subtracts 0 · m / (√v + ε) — and write `tuner.features_rest()` into `shs[:, 1:, :]` after the
    tail, which had rebuilt shs from that tensor."""

    def __init__(self, sh: SHCodebook, lr: float = 25e-4 / 20, eps: float = 1e-15):
        if sh.codebook.device.type != "cuda" or not sh.codebook.is_contiguous():
            raise ValueError("the codebook must be a contiguous HIP device tensor (no CPU path)")
        self.sh = sh
        self.codebook = sh.codebook
        self.optimizer = optim.Adam(self.codebook, lr, eps=eps)
        self.grad = torch.empty_like(self.codebook)

    def features_rest(self) -> torch.Tensor:
        return self.sh.decode()

    def step(self, g_features_rest: torch.Tensor) -> None:
        codebook_grad(g_features_rest, self.sh, out=self.grad)
        self.optimizer.step(self.codebook, self.grad)
