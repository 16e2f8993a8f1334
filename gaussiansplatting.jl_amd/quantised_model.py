"""The quantised model container: every attribute of a model as 8- or 16-bit codes with per-block ranges, the SH rest through
the codebook of sh_codebook.py (include/gsr.h gsr_quant_*; csrc/quant.hip).  No reference counterpart.  It is
the last step of LightGaussian (Fan et al. 2023), Compact3D (Navaneet et al. 2023) and "Compressed 3D Gaussian Splatting"
(Niedermayr et al. 2024): at SH degree 3 with a codebook a Gaussian is 6 + 3 + 1 + 3 + 4 + 2 = 19 bytes on the device.

  quant_ranges(rows, block_rows=0) / quant_encode(rows, bits, ranges, block_rows=0, kind=LINEAR) / quant_decode(codes, bits, ...)
  QuantSpec                              per group (bits, block_rows)
  pack_model(model, sh_codebook=None, spec=QuantSpec(), order="morton")  -> QuantisedModel
  QuantisedModel.unpack() / nbytes / save(path, compressed=True) / load(path, device)
  FakeQuantizer(spec).refresh(model) / .apply(model, sh_codebook=None)   quantisation-aware fine-tuning
  positive_w_rotations_(rotations, adam=None)                            q -> -q where w < 0, once before such a run

A group is an (n, cols) float32 matrix; its codes have the same layout, uint8 up to 8 bits and uint16 above.  The definition of
ranges, encode and decode is the header's, one rounded fp32 operation each; tests/quant_ref.py restates it in numpy.  Out of
scope: bit-packing of other widths, an entropy coder beyond zlib, a geometry codebook, rendering from codes."""
from __future__ import annotations

import zipfile

import numpy as np
import torch

from . import _lib as L

GROUPS = ("points", "features_dc", "features_rest", "opacities", "scales", "rotations")  # the library's group order
LINEAR, UNIT_QUAT = L.QUANT_LINEAR, L.QUANT_UNIT_QUAT
MAX_COLS = 48
FORMAT_VERSION = 1


def n_blocks(n: int, block_rows: int) -> int:
    return 1 if block_rows == 0 else -(-int(n) // int(block_rows))


def _check_block_rows(block_rows: int) -> int:
    block_rows = int(block_rows)
    if block_rows != 0 and (block_rows < 64 or block_rows > 1024 or block_rows % 64):
        raise ValueError(f"block_rows = {block_rows}: 0, or a multiple of 64 in [64, 1024]")
    return block_rows


def _check_bits(bits: int) -> int:
    bits = int(bits)
    if not 1 <= bits <= 16:
        raise ValueError(f"bits = {bits}: 1 .. 16")
    return bits


def code_dtype(bits: int):
    return torch.uint8 if bits <= 8 else torch.uint16


def _matrix(t: torch.Tensor, name="rows"):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be on the HIP device (no CPU path)")
    if t.dim() != 2 or not 1 <= int(t.shape[1]) <= MAX_COLS:
        raise ValueError(f"{name} must be (n, cols) with 1 <= cols <= {MAX_COLS}, not {tuple(t.shape)}")
    return t.contiguous()


def _check_ranges(ranges, n, cols, block_rows, kind, device):
    if kind == UNIT_QUAT:
        if cols != 4:
            raise ValueError("unit quaternions are (n, 4) rows")
        return None
    want = (n_blocks(n, block_rows), 2, cols)
    if not (isinstance(ranges, torch.Tensor) and ranges.dtype == torch.float32 and tuple(ranges.shape) == want
            and ranges.device == device and ranges.is_contiguous()):
        raise ValueError(f"ranges must be a contiguous float32 {want} tensor on the rows' device")
    return ranges


def quant_ranges(rows: torch.Tensor, block_rows: int = 0) -> torch.Tensor:
    """(n_blocks, 2, cols): per block and column the minimum and maximum of the finite values (gsr_quant_ranges)."""
    rows = _matrix(rows)
    block_rows = _check_block_rows(block_rows)
    n, cols = (int(v) for v in rows.shape)
    ranges = torch.empty((n_blocks(n, block_rows), 2, cols), dtype=torch.float32, device=rows.device)
    if ranges.numel():
        with torch.cuda.device(rows.device):
            L.check(L.load().gsr_quant_ranges(n, cols, L.ptr(rows, True), block_rows, L.ptr(ranges), L.stream()))
    return ranges


def quant_encode(rows: torch.Tensor, bits: int, ranges=None, block_rows: int = 0, kind: int = LINEAR) -> torch.Tensor:
    """The codes of `rows`, (n, cols) uint8 (bits <= 8) or uint16 (gsr_quant_encode).  kind UNIT_QUAT: ranges is not used."""
    rows = _matrix(rows)
    bits, block_rows = _check_bits(bits), _check_block_rows(block_rows)
    n, cols = (int(v) for v in rows.shape)
    ranges = _check_ranges(ranges, n, cols, block_rows, kind, rows.device)
    codes = torch.empty((n, cols), dtype=code_dtype(bits), device=rows.device)
    if n:
        with torch.cuda.device(rows.device):
            L.check(L.load().gsr_quant_encode(n, cols, bits, kind, L.ptr(rows), block_rows, L.ptr(ranges), L.ptr(codes), L.stream()))
    return codes


def quant_decode(codes: torch.Tensor, bits: int, ranges=None, block_rows: int = 0, kind: int = LINEAR) -> torch.Tensor:
    """The float32 (n, cols) values of `codes` (gsr_quant_decode)."""
    bits, block_rows = _check_bits(bits), _check_block_rows(block_rows)
    if not isinstance(codes, torch.Tensor) or codes.dtype != code_dtype(bits):
        raise TypeError(f"codes of {bits} bits must be a {code_dtype(bits)} tensor")
    if codes.device.type != "cuda":
        raise ValueError("codes must be on the HIP device (no CPU path)")
    if codes.dim() != 2 or not 1 <= int(codes.shape[1]) <= MAX_COLS:
        raise ValueError(f"codes must be (n, cols) with 1 <= cols <= {MAX_COLS}")
    codes = codes.contiguous()
    n, cols = (int(v) for v in codes.shape)
    ranges = _check_ranges(ranges, n, cols, block_rows, kind, codes.device)
    out = torch.empty((n, cols), dtype=torch.float32, device=codes.device)
    if n:
        with torch.cuda.device(codes.device):
            L.check(L.load().gsr_quant_decode(n, cols, bits, kind, L.ptr(codes), block_rows, L.ptr(ranges), L.ptr(out), L.stream()))
    return out


class QuantSpec:
    """Per group (bits, block_rows).  The defaults: positions at 16 bits in blocks of 256 rows (after the Morton sort a block is
    a small box, so its grid is fine where the scene is dense); features_dc, opacities and scales at 8 bits with one range per
    column; rotations at 8 bits as unit quaternions in [-1, 1] (no ranges; block_rows must be 0); features_rest at 8 bits, used
    only when no SH codebook is given.  Isotropic (N, 1) scales are one column."""

    def __init__(self, points=(16, 256), features_dc=(8, 0), features_rest=(8, 0), opacities=(8, 0), scales=(8, 0), rotations=(8, 0)):
        for name, v in zip(GROUPS, (points, features_dc, features_rest, opacities, scales, rotations)):
            bits, block_rows = (int(x) for x in v)
            _check_bits(bits)
            _check_block_rows(block_rows)
            if name == "rotations" and block_rows != 0:
                raise ValueError("rotations are unit quaternions in the constant range [-1, 1]: block_rows must be 0")
            setattr(self, name, (bits, block_rows))

    def kind(self, name: str) -> int:
        return UNIT_QUAT if name == "rotations" else LINEAR

    def as_array(self) -> np.ndarray:
        return np.asarray([getattr(self, g) for g in GROUPS], np.int64)

    @classmethod
    def from_array(cls, a) -> "QuantSpec":
        a = np.asarray(a)
        if a.shape != (len(GROUPS), 2) or a.dtype.kind not in "iu":
            raise ValueError("the spec is a (6, 2) integer array")
        return cls(*[tuple(int(x) for x in row) for row in a])

    def __eq__(self, other):
        return isinstance(other, QuantSpec) and np.array_equal(self.as_array(), other.as_array())

    def __repr__(self):
        return "QuantSpec(" + ", ".join(f"{g}={getattr(self, g)}" for g in GROUPS) + ")"


def _model_box(points: torch.Tensor):
    """The box of the finite coordinates (lo x, y, z, hi x, y, z), or None when there is none to sort by.  One host read."""
    finite = torch.isfinite(points)
    big = torch.finfo(torch.float32).max
    lo = torch.where(finite, points, torch.full_like(points, big)).amin(0)
    hi = torch.where(finite, points, torch.full_like(points, -big)).amax(0)
    box = torch.cat([lo, hi]).tolist()
    if not all(np.isfinite(box)) or any(box[3 + k] < box[k] for k in range(3)):
        return None
    return box


def _permute_u16(idx: torch.Tensor, perm64: torch.Tensor) -> torch.Tensor:
    return idx.view(torch.int16)[perm64].contiguous().view(torch.uint16)


class QuantisedModel:
    """A packed model.  `codes[g]` (n, cols) uint8 / uint16 and `ranges[g]` (n_blocks, 2, cols) float32 (None for rotations) per
    stored group, `shapes[g]` the group's shape in the model, `sh` the SHCodebook standing for features_rest (or None: it is
    the 8-bit group, or empty), `ids` int32 or None, `permutation` the int32 row order pack_model applied (new row r = old row
    permutation[r]; None: the order was kept) — on the object only, not in the file."""

    def __init__(self, n, spec, codes, ranges, shapes, sh=None, ids=None, permutation=None):
        self.n, self.spec, self.codes, self.ranges, self.shapes = int(n), spec, dict(codes), dict(ranges), dict(shapes)
        self.sh, self.ids, self.permutation = sh, ids, permutation
        for g, c in self.codes.items():
            bits, block_rows = getattr(spec, g)
            cols = int(np.prod(self.shapes[g][1:]))
            if g not in GROUPS or c.dtype != code_dtype(bits) or tuple(c.shape) != (self.n, cols) or int(self.shapes[g][0]) != self.n:
                raise ValueError(f"{g}: codes of shape {tuple(c.shape)} and type {c.dtype} for {self.n} rows of {cols} at {bits} bits")
            r = self.ranges.get(g)
            if spec.kind(g) == UNIT_QUAT:
                if cols != 4:
                    raise ValueError("rotations must be (n, 4)")
            elif r is None or r.dtype != torch.float32 or tuple(r.shape) != (n_blocks(self.n, block_rows), 2, cols):
                raise ValueError(f"{g}: ranges must be float32 ({n_blocks(self.n, block_rows)}, 2, {cols})")
        need = [g for g in GROUPS if g != "features_rest"]
        if any(g not in self.codes for g in need):
            raise ValueError("a packed model holds points, features_dc, opacities, scales and rotations")
        if sh is not None and ("features_rest" in self.codes or int(sh.indices.shape[0]) != self.n):
            raise ValueError("the SH codebook stands for features_rest and has one index per Gaussian")
        if ids is not None and (ids.dtype != torch.int32 or tuple(ids.shape) != (self.n,)):
            raise ValueError("ids must be int32 (n,)")

    @property
    def nbytes(self) -> int:
        """Bytes of the container on the device: the codes, the ranges, and the codebook with its uint16 indices."""
        total = sum(c.numel() * c.element_size() for c in self.codes.values())
        total += sum(r.numel() * 4 for r in self.ranges.values() if r is not None)
        return total + (self.sh.nbytes if self.sh is not None else 0)

    def unpack(self):
        """The densification.GaussianModel of the dequantised values, in the container's row order; features_rest from
        SHCodebook.decode, from the 8-bit group, or empty."""
        from . import densification
        out = {}
        for g, c in self.codes.items():
            bits, block_rows = getattr(self.spec, g)
            out[g] = quant_decode(c, bits, self.ranges.get(g), block_rows, self.spec.kind(g)).view(self.shapes[g])
        if self.sh is not None:
            out["features_rest"] = self.sh.decode()
        elif "features_rest" not in out:
            out["features_rest"] = torch.empty((self.n, 0, 3), dtype=torch.float32, device=out["points"].device)
        return densification.GaussianModel(out["points"], out["features_dc"], out["features_rest"], out["scales"], out["rotations"],
                                           out["opacities"], ids=self.ids)

    def save(self, path, compressed: bool = True) -> None:
        """A numpy.savez (or savez_compressed: zlib) archive without pickles: format_version, n, spec (6, 2), per stored group
        <g>_codes, <g>_ranges, <g>_shape; the codebook as sh_codebook float32 (K, D), sh_indices uint16 (n,), sh_shape (the
        SHCodebook.save conventions); ids when present.  The permutation is not stored."""
        def u(t):
            a = t.detach().cpu()
            return a.view(torch.int16).numpy().view(np.uint16) if a.dtype == torch.uint16 else a.numpy()
        z = dict(format_version=np.asarray(FORMAT_VERSION, np.int64), n=np.asarray(self.n, np.int64), spec=self.spec.as_array())
        for g, c in self.codes.items():
            z[f"{g}_codes"] = u(c)
            z[f"{g}_shape"] = np.asarray(self.shapes[g], np.int64)
            if self.ranges.get(g) is not None:
                z[f"{g}_ranges"] = u(self.ranges[g])
        if self.sh is not None:
            z["sh_codebook"], z["sh_indices"], z["sh_shape"] = u(self.sh.codebook), u(self.sh.indices), np.asarray(self.sh.shape, np.int64)
        if self.ids is not None:
            z["ids"] = u(self.ids)
        (np.savez_compressed if compressed else np.savez)(path, **z)

    @classmethod
    def load(cls, path, device="cpu") -> "QuantisedModel":
        """The container of `save`.  ValueError for anything that is not one: not an archive, a missing or extra-typed entry,
        another format version, shapes that do not fit each other."""
        from .sh_codebook import SHCodebook
        try:
            with np.load(path, allow_pickle=False) as f:
                z = {k: f[k] for k in f.files}
        except FileNotFoundError:
            raise
        except (zipfile.BadZipFile, OSError, EOFError, KeyError, ValueError) as e:
            raise ValueError(f"not a quantised model archive: {e}") from None
        if not isinstance(z, dict) or "format_version" not in z or "spec" not in z or "n" not in z:
            raise ValueError("not a quantised model archive")
        try:
            if z["format_version"].dtype.kind not in "iu" or int(z["format_version"]) != FORMAT_VERSION:
                raise ValueError(f"format version {z['format_version']}, this reader knows {FORMAT_VERSION}")
            n = int(z["n"])
            if z["n"].dtype.kind not in "iu" or n < 0:
                raise ValueError("bad n")
            spec = QuantSpec.from_array(z["spec"])

            def t(a):
                a = np.ascontiguousarray(a)
                if a.dtype == np.uint16:
                    return torch.from_numpy(a.view(np.int16).copy()).view(torch.uint16).to(device)
                return torch.from_numpy(a.copy()).to(device)
            codes, ranges, shapes = {}, {}, {}
            for g in GROUPS:
                if f"{g}_codes" not in z:
                    continue
                bits, _ = getattr(spec, g)
                c, shape = z[f"{g}_codes"], z[f"{g}_shape"]
                if c.dtype != (np.uint8 if bits <= 8 else np.uint16) or c.ndim != 2 or shape.dtype.kind not in "iu" or shape.ndim != 1:
                    raise ValueError(f"{g}: codes of type {c.dtype} at {bits} bits")
                codes[g], shapes[g] = t(c), tuple(int(v) for v in shape)
                r = z.get(f"{g}_ranges")
                if r is not None:
                    if r.dtype != np.float32:
                        raise ValueError(f"{g}: ranges must be float32")
                    ranges[g] = t(r)
            sh = None
            if "sh_codebook" in z:
                cb, idx, shape = z["sh_codebook"], z["sh_indices"], z["sh_shape"]
                if cb.dtype != np.float32 or cb.ndim != 2 or idx.dtype != np.uint16 or idx.ndim != 1 or shape.dtype.kind not in "iu":
                    raise ValueError("not an SH codebook")
                if shape.ndim != 1 or shape.size < 2 or idx.size != int(shape[0]) or int(np.prod(shape[1:])) != cb.shape[1] or cb.shape[0] < 1:
                    raise ValueError("the SH codebook's shape does not match its codebook and indices")
                sh = SHCodebook(t(cb), t(idx), shape)
            ids = None
            if "ids" in z:
                if z["ids"].dtype != np.int32:
                    raise ValueError("ids must be int32")
                ids = t(z["ids"])
            return cls(n, spec, codes, ranges, shapes, sh=sh, ids=ids)
        except (KeyError, TypeError, IndexError, OverflowError) as e:
            raise ValueError(f"malformed quantised model archive: {e!r}") from None


def _groups_of(model):
    """name -> (n, cols) contiguous view of the model's tensor, and its shape."""
    n = int(model.points.shape[0])
    out = {}
    for g in GROUPS:
        t = getattr(model, g)
        cols = int(np.prod(t.shape[1:])) if t.dim() > 1 else 1
        out[g] = (t.detach().contiguous().view(n, cols), tuple(int(v) for v in t.shape))
    return n, out


def pack_model(model, sh_codebook=None, spec: QuantSpec | None = None, order="morton") -> QuantisedModel:
    """Quantise a densification.GaussianModel.  order "morton": every row array — the SH indices and `ids` included — is first
    permuted by point_cloud.morton_permutation inside the box of the finite positions (one host read), so that consecutive rows
    are spatial neighbours and a block of positions is a small box; None keeps the order.  Then per group gsr_quant_ranges and
    gsr_quant_encode.  features_rest is `sh_codebook` (an SHCodebook of this model; its codebook is shared, its indices are
    permuted into a new object), or, without one, the spec's 8-bit group.  The permutation stays on the result."""
    from . import point_cloud
    from .sh_codebook import SHCodebook
    spec = QuantSpec() if spec is None else spec
    if order not in ("morton", None):
        raise ValueError('order is "morton" or None')
    n, groups = _groups_of(model)
    dev = model.points.device
    if sh_codebook is not None and int(sh_codebook.indices.shape[0]) != n:
        raise ValueError(f"an SH codebook of {int(sh_codebook.indices.shape[0])} rows for a model of {n}")
    perm = None
    with torch.cuda.device(dev):
        if order == "morton" and n > 1:
            box = _model_box(groups["points"][0])
            if box is not None:
                perm = point_cloud.morton_permutation(groups["points"][0], box)
        p64 = perm.long() if perm is not None else None
        codes, ranges, shapes = {}, {}, {}
        for g in GROUPS:
            rows, shape = groups[g]
            cols = int(rows.shape[1])
            if g == "features_rest" and (sh_codebook is not None or cols == 0):
                continue
            if p64 is not None:
                rows = rows[p64].contiguous()
            bits, block_rows = getattr(spec, g)
            kind = spec.kind(g)
            ranges[g] = None if kind == UNIT_QUAT else quant_ranges(rows, block_rows)
            codes[g] = quant_encode(rows, bits, ranges[g], block_rows, kind)
            shapes[g] = shape
        sh = None
        if sh_codebook is not None:
            idx = sh_codebook.indices if p64 is None else _permute_u16(sh_codebook.indices, p64)
            sh = SHCodebook(sh_codebook.codebook, idx, sh_codebook.shape)
        ids = getattr(model, "ids", None)
        if ids is not None and p64 is not None:
            ids = ids[p64].contiguous()
    return QuantisedModel(n, spec, codes, ranges, shapes, sh=sh, ids=ids, permutation=perm)


def positive_w_rotations_(rotations: torch.Tensor, adam=None) -> torch.Tensor:
    """Flip, in place, the rows (w, x, y, z) of `rotations` whose w is negative: -q is the same rotation.  `adam`: the rows'
    optim.Adam — its first moments change sign with them.  Returns the (n, 1) mask of the flipped rows.  No synchronisation.

    Why a fine-tuning run calls it first: the unit-quaternion code sign-fixes a row, u = -q / |q| where w < 0, so du/dq is a
    NEGATIVE multiple of the tangent projection there, and the straight-through gradient of FakeQuantizer — the identity — would
    move such a row uphill.  With every w >= 0 the identity differs from du/dq by the positive factor 1 / |q| only."""
    if rotations.dim() != 2 or int(rotations.shape[1]) != 4:
        raise ValueError("rotations must be (n, 4)")
    flip = rotations[:, :1] < 0
    sign = torch.where(flip, -1.0, 1.0).to(rotations.dtype)
    with torch.no_grad():
        rotations.mul_(sign)
        if adam is not None:
            adam.mu.view(rotations.shape).mul_(sign)
    return flip


class _FakeQuant(torch.autograd.Function):
    """decode(encode(x)) of every group in one gsr_quant_fake launch; backward: the straight-through estimator — the incoming
    gradient, unchanged and unmasked (a clamped value keeps its gradient: the ranges follow the parameters at every refresh)."""

    @staticmethod
    def forward(ctx, descr, *tensors):
        n = int(tensors[0].shape[0]) if tensors else 0
        outs = [torch.empty_like(t, memory_format=torch.contiguous_format) for t in tensors]
        if n and tensors:
            arr = (L.QuantGroup * len(tensors))()
            keep = []
            for i, (t, o, (cols, bits, kind, block_rows, ranges)) in enumerate(zip(tensors, outs, descr)):
                t = t.detach().contiguous()
                keep.append(t)
                arr[i] = L.QuantGroup(t.data_ptr(), o.data_ptr(), cols, bits, kind, block_rows, ranges.data_ptr() if ranges is not None else None)
            with torch.cuda.device(tensors[0].device):
                L.check(L.load().gsr_quant_fake(arr, len(tensors), n, L.stream()))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        return (None,) + tuple(grads)


class FakeQuantizer:
    """Quantisation-aware fine-tuning (the third step of Niedermayr et al.): the forward pass sees the values the container
    would hold, the optimizer keeps stepping the unquantised raw parameters.

      refresh(model)                 compute the ranges of every linear group from the model's current raw parameters
                                     (gsr_quant_ranges); call it again whenever the values have moved or the rows changed
      apply(model, sh_codebook=None) the six raw tensors, in the order points, features_dc, features_rest, opacities, scales,
                                     rotations, quantise-dequantised by ONE gsr_quant_fake launch.  Differentiable: a
                                     torch.autograd.Function whose backward is the straight-through estimator, the identity,
                                     unmasked.  With `sh_codebook` (an SHCodebook or an SHCodebookFineTuner, which then supplies
                                     and trains features_rest through its own step) features_rest is its decode and five groups
                                     are launched.  Rotations come back as the dequantised UNIT quaternions.

    The step without autograd:
      1. points, dc, rest, opacities, scales, rotations = fq.apply(model)      (under no_grad: plain tensors)
      2. shs, opacities_act, scales_act = rasterizer.prologue_forward(dc, rest, opacities, scales)   (gsr_prologue_forward)
      3. forward_raw and backward_raw on (points, shs, opacities_act, scales_act, rotations)
      4. rasterizer.prologue_backward(opacities_act, scales_act, vshs, vopacities, vscales): gsr_prologue_backward at the QUANTISED
         activated values — straight-through means these gradients are used as the gradients of the raw parameters
      5. optim.step_all on the RAW parameters (model.points, ...), not on the outputs of 1.
    The fused Adam tails (optim.trainer_tail_step, fused_backward_tail_step, sh_views_tail_step) rewrite shs, opacities_act
    and scales_act from the UNQUANTISED θ they have just stepped, so the next forward would not see quantised values: they are
    not used in this mode.

    Rotations: the identity is a descent direction only for rows with w >= 0 (positive_w_rotations_ above explains it): flip
    the model's rotations once before the run.

    Blocked position ranges (the default spec: blocks of 256 rows) want a Morton-sorted model — sort it once with
    densification.reorder_spatially (or train the unpacked container, which pack_model sorted); on an unsorted model a block's
    box is the scene's and the blocks buy nothing."""

    def __init__(self, spec: QuantSpec | None = None):
        self.spec = QuantSpec() if spec is None else spec
        self.ranges = None
        self._n = -1

    def refresh(self, model) -> None:
        n, groups = _groups_of(model)
        self.ranges = {}
        for g in GROUPS:
            rows, _ = groups[g]
            if self.spec.kind(g) == UNIT_QUAT or rows.shape[1] == 0:
                self.ranges[g] = None
            else:
                self.ranges[g] = quant_ranges(rows, getattr(self.spec, g)[1])
        self._n = n

    def apply(self, model, sh_codebook=None):
        if self.ranges is None:
            raise RuntimeError("refresh(model) computes the ranges first")
        n = int(model.points.shape[0])
        if n != self._n:
            raise ValueError(f"the ranges were computed for {self._n} rows, the model has {n}: refresh(model)")
        names, tensors, descr = [], [], []
        for g in GROUPS:
            t = getattr(model, g)
            cols = int(np.prod(t.shape[1:])) if t.dim() > 1 else 1
            if g == "features_rest" and (sh_codebook is not None or cols == 0):
                continue
            if not (t.is_cuda and t.dtype == torch.float32):
                raise ValueError(f"{g} must be a float32 HIP device tensor (no CPU path)")
            if cols > MAX_COLS:
                raise ValueError(f"{g}: {cols} columns, at most {MAX_COLS}")
            bits, block_rows = getattr(self.spec, g)
            names.append(g)
            tensors.append(t)
            descr.append((cols, bits, self.spec.kind(g), block_rows, self.ranges[g]))
        out = dict(zip(names, _FakeQuant.apply(descr, *tensors)))
        if sh_codebook is not None:
            out["features_rest"] = sh_codebook.features_rest() if hasattr(sh_codebook, "features_rest") else sh_codebook.decode()
        elif "features_rest" not in out:
            out["features_rest"] = model.features_rest
        return tuple(out[g] for g in GROUPS)
