"""Checkpoints: host mirror of src/checkpoint.jl + the `write_state!` / `read_state!` pairs of
`GaussianModel` (src/gaussians.jl:91-116) and `NU.Adam` (src/training.jl:396-413) — SURVEY.md
§8f rank 4.  A checkpoint is ONE safetensors file: a flat `name -> tensor` table under dotted
prefixes (`gaussians.points`, `optimizers.scales.mu.1`, ...) and every scalar as a string in
the `__metadata__` map, tagged `format = GaussianSplatting.jl-checkpoint-1`.  Pure host I/O.

On-disk layout.  safetensors stores, per tensor, a shape and the data in C (row-major) order OF THAT SHAPE.
The reference hands SafeTensors.jl its column-major Julia arrays and notes that tensors "are stored in C order,
so [reading] also un-permutes back to the column-major array that was written" (checkpoint.jl:30-33): the header
carries the JULIA shape — `points` is [3, N], `features_rest` [3, K-1, N], `rotations` [4, N] — and the bytes are
that logical array in row-major order.  This package keeps the C-order equivalents in memory ((N,3) ≙ Julia (3,N),
identical bytes to the Julia array), so every tensor is written with its axes reversed and reversed back on read;
a numpy/torch reader of a reference-written file therefore sees (3, N) and gets (N, 3) from `read_gaussians`.
Adam moments are written with the parameter's Julia shape (what `NU.Adam` holds before the first densification)
and accepted either shaped or flat (after `_append_optimizer!` / `_prune_optimizer!` they are flat vectors,
densification.jl:255-288).  Shapes are validated on read.  SafeTensors.jl 1.2.1 itself is external to the reference
tree, so this layout is pinned by the reference's comment and the safetensors specification (tests build a
byte-level file by hand), not by a file the reference wrote: PARITY UNPINNED in that sense.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

CHECKPOINT_FORMAT = "GaussianSplatting.jl-checkpoint-1"
OPTIMIZER_NAMES = ("points", "features_dc", "features_rest", "opacities", "scales", "rotations")  # training.jl:415-416
STRATEGY_STATS = ("max_radii", "accum_grad_means_2d", "denom")  # DefaultStrategy's per-Gaussian statistics (strategy.jl:30-34)


class Checkpoint:
    """A checkpoint opened for reading (checkpoint.jl:17-35): `tensor(key)`, `meta[key]`, `key in ckpt`."""

    def __init__(self, filename: str):
        from safetensors import safe_open
        self._f = safe_open(filename, framework="numpy")
        meta = self._f.metadata()
        if meta is None or meta.get("format") != CHECKPOINT_FORMAT:
            raise ValueError(f"`{filename}` is not a GaussianSplatting.jl checkpoint "
                             f"(no `{CHECKPOINT_FORMAT}` in its metadata).")
        self.meta: Dict[str, str] = dict(meta)
        self._keys = set(self._f.keys())

    def __contains__(self, key: str) -> bool:
        return key in self._keys

    def tensor(self, key: str) -> np.ndarray:
        """The array at `key` in this package's in-memory convention: file (Julia logical) axes reversed."""
        return _from_file(self._f.get_tensor(key))

    def raw_tensor(self, key: str) -> np.ndarray:
        """The array exactly as the file describes it (Julia logical shape)."""
        return np.ascontiguousarray(self._f.get_tensor(key))

    def read_scalar(self, key: str, typ=int):
        return typ(self.meta[key])


def _to_file(x: np.ndarray) -> np.ndarray:
    """In-memory (Gaussian index first) -> file layout (Julia logical shape, row-major bytes)."""
    x = np.asarray(x)
    return np.ascontiguousarray(x.transpose(tuple(reversed(range(x.ndim)))))


def _from_file(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a)
    return np.ascontiguousarray(a.transpose(tuple(reversed(range(a.ndim)))))


def save_checkpoint(filename: str, tensors: Dict[str, np.ndarray], meta: Dict[str, str]) -> None:
    """checkpoint.jl:44-55.  `tensors` are in-memory arrays (Gaussian index first); they are written with the
    reference's (Julia) shapes."""
    from safetensors.numpy import save_file
    meta = dict(meta)
    meta["format"] = CHECKPOINT_FORMAT
    save_file({k: _to_file(v) for k, v in tensors.items()}, filename, metadata=meta)


def load_checkpoint(filename: str) -> Checkpoint:
    """checkpoint.jl:57-70."""
    return Checkpoint(filename)


def _host(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x)


# ---- GaussianModel (gaussians.jl:91-116); `m` is a ply.GaussianModel (numpy or torch arrays) ----
def write_gaussians(tensors, meta, prefix: str, m) -> None:
    for name in ("points", "features_dc", "features_rest", "scales", "rotations", "opacities"):
        tensors[f"{prefix}.{name}"] = _host(getattr(m, name))
    meta[f"{prefix}.sh_degree"] = str(int(m.sh_degree))
    meta[f"{prefix}.max_sh_degree"] = str(int(m.max_sh_degree))


def read_gaussians(ckpt: Checkpoint, prefix: str):
    from .ply import GaussianModel
    t = {name: ckpt.tensor(f"{prefix}.{name}") for name in
         ("points", "features_dc", "features_rest", "scales", "rotations", "opacities")}
    n = t["points"].shape[0]
    want = {"points": lambda a: a.ndim == 2 and a.shape[1] == 3, "features_dc": lambda a: a.ndim == 3 and a.shape[1:] == (1, 3),
            "features_rest": lambda a: a.ndim == 3 and a.shape[2] == 3, "scales": lambda a: a.ndim == 2 and a.shape[1] in (1, 3),
            "rotations": lambda a: a.ndim == 2 and a.shape[1] == 4, "opacities": lambda a: a.ndim == 2 and a.shape[1] == 1}
    for name, ok in want.items():
        if not ok(t[name]) or t[name].shape[0] != n:
            raise ValueError(f"{prefix}.{name}: file shape {ckpt.raw_tensor(f'{prefix}.{name}').shape} is not the reference's "
                             f"layout for {n} Gaussians (expected Julia shapes (3,N), (3,1,N), (3,K-1,N), (3|1,N), (4,N), (1,N))")
    return GaussianModel(t["points"], t["features_dc"], t["features_rest"], t["scales"], t["rotations"],
                         t["opacities"], ckpt.read_scalar(f"{prefix}.sh_degree"),
                         ckpt.read_scalar(f"{prefix}.max_sh_degree"))


# ---- NU.Adam (training.jl:396-413): one numbered moment pair per parameter array ----
def write_adam(tensors, meta, prefix: str, opt, shape=None) -> None:
    """`shape`: the parameter's in-memory shape, e.g. (N,3) — the moments are then written with the parameter's Julia
    shape, as `NU.Adam` holds them; None writes the flat vector (what they are after a densification)."""
    mu, nu = _host(opt.mu), _host(opt.nu)
    if shape is not None:
        if int(np.prod(shape)) != mu.size:
            raise ValueError(f"{prefix}: moments of {mu.size} elements do not match a parameter of shape {tuple(shape)}")
        mu, nu = mu.reshape(shape), nu.reshape(shape)
    tensors[f"{prefix}.mu.1"] = mu
    tensors[f"{prefix}.nu.1"] = nu
    meta[f"{prefix}.n_moments"] = "1"
    meta[f"{prefix}.current_step"] = str(int(opt.current_step))


def read_adam(opt, ckpt: Checkpoint, prefix: str, numel=None) -> None:
    """In place on an optim.Adam (device moments).  Shaped (parameter-shaped) and flat moments are both accepted: the
    flat vector of the in-memory (Gaussian-first, C-order) array IS the column-major flattening of the Julia array."""
    import torch
    n = ckpt.read_scalar(f"{prefix}.n_moments")
    if n != 1:
        raise ValueError(f"{prefix}: {n} moment pairs, expected one per parameter array")
    for attr, key in (("mu", "mu.1"), ("nu", "nu.1")):
        host = torch.from_numpy(ckpt.tensor(f"{prefix}.{key}").reshape(-1).astype(np.float32))
        if numel is not None and host.numel() != numel:
            raise ValueError(f"{prefix}.{key}: {host.numel()} elements, the parameter has {numel}")
        cur = getattr(opt, attr)
        setattr(opt, attr, host.to(cur.device) if cur is not None else host)
    opt.current_step = ckpt.read_scalar(f"{prefix}.current_step")


# ---- SkyDome (sky_dome.jl:322-333); `sky` has `gaussians` (a ply.GaussianModel), `optimizer` (one moment pair), `radius` ----
def write_sky(tensors, meta, prefix: str, sky) -> None:
    write_gaussians(tensors, meta, f"{prefix}.gaussians", sky.gaussians)
    write_adam(tensors, meta, f"{prefix}.optimizer", sky.optimizer, shape=tuple(_host(sky.gaussians.features_dc).shape))
    meta[f"{prefix}.radius"] = repr(float(np.float32(sky.radius)))


def read_sky(sky, ckpt: Checkpoint, prefix: str) -> None:
    """In place, as `read_state!(sky, ckpt, prefix)`: the model's arrays and the colour optimizer; the dome keeps the radius
    (and the rasterizer) it was built with.  The file's dome must have the trainer's size."""
    g = read_gaussians(ckpt, f"{prefix}.gaussians")
    cur = sky.gaussians
    n = int(_host(cur.points).shape[0])
    if g.n != n:
        raise ValueError(f"{prefix}.gaussians: {g.n} Gaussians in the file, the trainer's dome has {n}")
    for name in ("points", "features_dc", "features_rest", "scales", "rotations", "opacities"):
        dst, src = getattr(cur, name), np.ascontiguousarray(getattr(g, name), dtype=np.float32)
        if tuple(dst.shape) != src.shape:
            raise ValueError(f"{prefix}.gaussians.{name}: file shape {src.shape[::-1]} does not match the dome's {tuple(dst.shape)[::-1]}")
        if hasattr(dst, "copy_"):
            import torch
            dst.copy_(torch.from_numpy(src))
        else:
            np.copyto(dst, src)
    read_adam(sky.optimizer, ckpt, f"{prefix}.optimizer", numel=int(g.features_dc.size))
    if hasattr(sky, "_refresh_activations"):
        sky._refresh_activations()


# ---- the SH codebook under fine-tuning (sh_codebook.SHCodebookFineTuner; no reference counterpart) ----
def _u16_host(x) -> np.ndarray:
    """uint16 indices (a torch.uint16 tensor, or a numpy array) as a numpy uint16 array."""
    if hasattr(x, "detach"):
        import torch
        return np.ascontiguousarray(x.detach().cpu().view(torch.int16).numpy().view(np.uint16))
    return np.ascontiguousarray(x, dtype=np.uint16)


def write_sh_codebook(tensors, meta, prefix: str, tuner) -> None:
    """`tuner`: a SHCodebookFineTuner (`sh`, `optimizer`), or a bare SHCodebook (no moments are written).  The group:
    `{prefix}.codebook` float32 (K, D), `.indices` uint16 (n), `.shape` int64 — the features_rest the codebook stands for —
    and the code rows' optimizer under `{prefix}.optimizer` (write_adam)."""
    sh = getattr(tuner, "sh", tuner)
    cb = _host(sh.codebook).astype(np.float32, copy=False)
    tensors[f"{prefix}.codebook"] = cb
    tensors[f"{prefix}.indices"] = _u16_host(sh.indices)
    tensors[f"{prefix}.shape"] = np.asarray(tuple(sh.shape), np.int64)
    opt = getattr(tuner, "optimizer", None)
    if opt is not None:
        write_adam(tensors, meta, f"{prefix}.optimizer", opt, shape=cb.shape)


def read_sh_codebook(tuner, ckpt: Checkpoint, prefix: str) -> None:
    """In place: the code rows are copied into `sh.codebook` (the tensor the optimizer and autograd know), `sh.indices` is
    replaced — so `sh.groups()` is built again — and the optimizer's moments are restored when the object has an optimizer
    and the file its moments.  The file's codebook must have the object's shape."""
    import torch
    sh = getattr(tuner, "sh", tuner)
    cb = np.ascontiguousarray(ckpt.tensor(f"{prefix}.codebook"), dtype=np.float32)
    idx = np.ascontiguousarray(ckpt.tensor(f"{prefix}.indices"))
    shape = tuple(int(v) for v in ckpt.tensor(f"{prefix}.shape").reshape(-1))
    if idx.dtype != np.uint16 or idx.ndim != 1 or cb.ndim != 2:
        raise ValueError(f"{prefix}: not an SH codebook group")
    if tuple(cb.shape) != tuple(sh.codebook.shape):
        raise ValueError(f"{prefix}.codebook: {cb.shape} in the file, the object's codebook is {tuple(sh.codebook.shape)}")
    if not shape or idx.size != shape[0] or int(np.prod(shape[1:])) != cb.shape[1]:
        raise ValueError(f"{prefix}.shape: {shape} does not match its codebook and indices")
    with torch.no_grad():
        sh.codebook.copy_(torch.from_numpy(cb))
    sh.indices = torch.from_numpy(idx.view(np.int16).copy()).view(torch.uint16).to(sh.indices.device)
    sh.shape = shape
    opt = getattr(tuner, "optimizer", None)
    if opt is not None and f"{prefix}.optimizer.n_moments" in ckpt.meta:
        read_adam(opt, ckpt, f"{prefix}.optimizer", numel=int(cb.size))


def save_state(filename: str, gaussians, optimizers: Dict[str, object], step: int, strategy=None,
               extra_meta: Optional[Dict[str, str]] = None, bilateral_grid=None, sky=None, sh_codebook=None) -> None:
    """The Gaussian + optimizer part of `save_state` (training.jl:418-445).  `strategy` (a densification.DefaultStrategy):
    its split-noise position is added as two metadata scalars (`strategy.split_seed_base`, `strategy.split_rounds`; an
    mcmc.MCMCStrategy: `strategy.seed_base`, `strategy.sample_rounds`, `strategy.noise_steps` — its `state_dict()`) —
    keys the reference's reader never asks for, so the file stays a valid reference checkpoint; the reference itself draws
    split noise from the backend's RNG and has nothing to save there (densification.jl:128).
    `extra_meta`: more string scalars of the same kind — e.g. {"gsr.ssim_precision": "fast"}: the arithmetic of the loss head the
    run trained with (the library default is the contracted build, not bit-identical to the exact twin).
    `sky` (a sky_dome.SkyDome): the reference's `sky.*` group (sky_dome.jl:322-327) — `sky.gaussians.*`, the colour
    optimizer `sky.optimizer.{mu.1,nu.1,n_moments,current_step}` and the scalar `sky.radius`.
    `sh_codebook` (a sh_codebook.SHCodebookFineTuner): the group `sh_codebook.{codebook, indices, shape}` and the code rows'
    optimizer `sh_codebook.optimizer.*` (write_sh_codebook) — tensors the reference's reader never asks for."""
    tensors, meta = {}, {}
    write_gaussians(tensors, meta, "gaussians", gaussians)
    for name in OPTIMIZER_NAMES:
        write_adam(tensors, meta, f"optimizers.{name}", optimizers[name], shape=tuple(_host(getattr(gaussians, name)).shape))
    meta["step"] = str(int(step))
    if strategy is not None:
        for k, v in strategy.state_dict().items():
            meta[f"strategy.{k}"] = str(int(v))
        # ... and its running statistics (strategy.jl:30-34: max_radii, accum_∇means_2d, denom).  The reference does not
        # save them — a resumed reference run densifies from half an interval's statistics —; with them a resume in the
        # middle of a densification interval continues BIT-IDENTICALLY (tests/test_gpu_train_protocol.py).  Extra tensors the
        # reference's reader never asks for.
        for k in STRATEGY_STATS:
            if getattr(strategy, k, None) is not None:
                tensors[f"strategy.{k}"] = _host(getattr(strategy, k))
    if bilateral_grid is not None:
        # training.jl:429-433: the grids with their Julia shape (gx, gy, gz, 12, n) and their NU.Adam
        grids = _host(bilateral_grid.grids)
        tensors["bilateral.grids"] = grids
        write_adam(tensors, meta, "bilateral.opt", bilateral_grid.optimizer, shape=grids.shape)
    if sky is not None:
        write_sky(tensors, meta, "sky", sky)
    if sh_codebook is not None:
        write_sh_codebook(tensors, meta, "sh_codebook", sh_codebook)
    for k, v in (extra_meta or {}).items():
        meta[str(k)] = str(v)
    save_checkpoint(filename, tensors, meta)


def load_state(filename: str, optimizers: Dict[str, object], strategy=None, bilateral_grid=None, sky=None, sh_codebook=None):
    """Counterpart (training.jl:447-470): returns (GaussianModel, step); optimizers are filled in place, and so is
    `strategy`'s split-noise position when the file carries one.  `bilateral_grid` (a bilateral_grid.BilateralGrid): its
    grids and optimizer are restored in place when the file has them (training.jl:452-459, `haskey` semantics: a file
    without them leaves the grids as they are).  `sky` (a sky_dome.SkyDome): restored in place when the file has
    `sky.gaussians.points` (training.jl:463-465, the same semantics: a file without the group leaves the dome as built, and
    without `sky` the group is ignored).  `sh_codebook` (a sh_codebook.SHCodebookFineTuner): restored in place when the file
    has `sh_codebook.codebook`, the same semantics."""
    ckpt = load_checkpoint(filename)
    g = read_gaussians(ckpt, "gaussians")
    for name in OPTIMIZER_NAMES:
        read_adam(optimizers[name], ckpt, f"optimizers.{name}", numel=int(np.asarray(getattr(g, name)).size))
    # the strategy's scalars: DefaultStrategy's split-noise position, or whatever the strategy names in STATE_KEYS
    # (mcmc.MCMCStrategy: its seed and its sampling / noise counters) — restored when the file carries all of them
    keys = getattr(strategy, "STATE_KEYS", ("split_seed_base", "split_rounds"))
    if strategy is not None and all(f"strategy.{k}" in ckpt.meta for k in keys):
        strategy.load_state_dict({k: ckpt.read_scalar(f"strategy.{k}") for k in keys})
    # the running statistics belong to a DefaultStrategy; a strategy without them (mcmc.MCMCStrategy) leaves them in the file
    if strategy is not None and all(hasattr(strategy, k) and f"strategy.{k}" in ckpt for k in STRATEGY_STATS):
        import torch
        n = int(np.asarray(g.points).shape[0])
        for k in STRATEGY_STATS:
            host = ckpt.tensor(f"strategy.{k}").reshape(-1)
            if host.size != n:
                raise ValueError(f"strategy.{k}: {host.size} entries for {n} Gaussians")
            cur = getattr(strategy, k)
            setattr(strategy, k, torch.from_numpy(np.ascontiguousarray(host)).to(cur.device if cur is not None else "cpu"))
    if bilateral_grid is not None and "bilateral.grids" in ckpt:
        import torch
        host = ckpt.tensor("bilateral.grids")
        cur = bilateral_grid.grids
        if tuple(host.shape) != tuple(cur.shape):
            raise ValueError(f"bilateral.grids: file shape {ckpt.raw_tensor('bilateral.grids').shape} does not match the "
                             f"trainer's grids (Julia shape {tuple(reversed(tuple(cur.shape)))})")
        cur.copy_(torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)))
        read_adam(bilateral_grid.optimizer, ckpt, "bilateral.opt", numel=int(host.size))
    if sky is not None and "sky.gaussians.points" in ckpt:
        read_sky(sky, ckpt, "sky")
    if sh_codebook is not None and "sh_codebook.codebook" in ckpt:
        read_sh_codebook(sh_codebook, ckpt, "sh_codebook")
    return g, ckpt.read_scalar("step")
