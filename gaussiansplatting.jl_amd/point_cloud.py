"""From a point cloud to a model on the device: `compute_scales` (src/dataset.jl:236-249) and the constructor
`GaussianModel(kab, points, colors, scales; max_sh_degree, isotropic, use_ids)` (src/gaussians.jl:22-56).

The neighbour search is the library's (csrc/knn.hip, gsr_knn_scales): the exact three nearest neighbours of every point,
found group by group along a Morton order of the cloud — no host tree, no round trip of the points.  The O(N) fills of the
constructor are torch operations.  Arrays are the C-order equivalents of the reference's, Gaussian index first.  Loading a
COLMAP reconstruction and taking colours from images are not built: both functions start at device tensors."""
from __future__ import annotations

import ctypes as C

import numpy as np

import torch

from . import _args as A
from . import _lib as L
from .densification import GaussianModel
from .sky_dome import SH0, inverse_sigmoid

f32 = np.float32


def _check_points(points, name="points"):
    if not (isinstance(points, torch.Tensor) and points.is_cuda):
        raise ValueError(f"{name} must be a HIP device tensor (no CPU path)")
    return int(A.check(points, f"{name} must be a contiguous float32 (N, 3) HIP tensor", shape=(None, 3)).shape[0])


def morton_permutation(points: torch.Tensor, box) -> torch.Tensor | None:
    """The permutation `densification.reorder_spatially` sorts a model by: gsr_morton_codes inside `box` (lo x, y, z, hi x,
    y, z), stable argsort.  None for a box that is a single point (every code equal: the identity)."""
    n = int(points.shape[0])
    if all(box[3 + k] == box[k] for k in range(3)):
        return None
    codes = torch.empty(n, dtype=torch.int64, device=points.device)  # 63-bit codes: order as signed = as unsigned
    L.check(L.load().gsr_morton_codes(n, L.ptr(points), (C.c_float * 3)(*box[:3]), (C.c_float * 3)(*box[3:]), L.ptr(codes),
                                      L.stream()))
    return torch.argsort(codes, stable=True).to(torch.int32)


def compute_scales(points: torch.Tensor, point_size: float = 1.0, isotropic: bool = False, order="morton",
                   return_dist2: bool = False):
    """compute_scales (dataset.jl:236-249): per point the log of the root mean squared distance to its three nearest
    neighbours, times sqrt(point_size) — (N, 3) with the value in all three columns, or (N, 1) when `isotropic`.
    `order`: "morton" (the default) groups the search along a Z-order curve of the cloud; None searches in the given order; a
    device tensor of N row numbers is used as the permutation.  The result does not depend on it, the time does.
    `return_dist2`: also the (N, 3) squared distances, ascending.  One host read (the cloud's box, which is also the check
    that every coordinate is finite)."""
    n = _check_points(points)
    if 0 < n < 4:
        raise ValueError(f"{n} points: three neighbours need at least 4 (the reference's knn(kdtree, xyz, 4) throws)")
    if not float(point_size) > 0.0:
        raise ValueError(f"point_size = {point_size} must be positive")
    sd = 1 if isotropic else 3
    scales = torch.empty((n, sd), dtype=torch.float32, device=points.device)
    dist2 = torch.empty((n, 3), dtype=torch.float32, device=points.device) if return_dist2 else None
    if n > 0:
        box = torch.cat([points.amin(0), points.amax(0)]).tolist()  # amin / amax propagate a NaN; an Inf is its own extreme
        if not all(np.isfinite(box)):
            raise ValueError("points holds a non-finite coordinate")
        if isinstance(order, torch.Tensor):
            if not (order.is_cuda and order.device == points.device and order.dtype in (torch.int32, torch.int64)
                    and tuple(order.shape) == (n,)):
                raise ValueError("order must be an int32 / int64 HIP tensor of N row numbers on the points' device")
            perm = order.to(torch.int32).contiguous()
        elif order == "morton":
            perm = morton_permutation(points, box)
        elif order is None:
            perm = None
        else:
            raise ValueError(f"order = {order!r}: 'morton', None or a permutation tensor")
        lib = L.load()
        nb = int(lib.gsr_knn_scratch_bytes(n))
        scratch = torch.empty(nb, dtype=torch.uint8, device=points.device)  # (torch allocations are 256-byte aligned)
        L.check(lib.gsr_knn_scales(n, L.ptr(points), L.ptr(perm), float(point_size), sd, L.ptr(scales), L.ptr(dist2),
                                   L.ptr(scratch), nb, L.stream()))
    return (scales, dist2) if return_dist2 else scales


def model_from_point_cloud(points: torch.Tensor, colors: torch.Tensor, scales: torch.Tensor | None = None, *,
                           max_sh_degree: int = 3, isotropic: bool = False, use_ids: bool = False,
                           point_size: float = 1.0) -> GaussianModel:
    """GaussianModel(kab, points, colors, scales; max_sh_degree, isotropic, use_ids) (gaussians.jl:22-56): positions as
    given, features_dc = rgb_2_sh.(colors), higher SH bands zero, identity rotations, opacity inverse_sigmoid(0.1), `ids`
    zeros when asked.  `scales` None: compute_scales(points; point_size) (what the trainer passes, training.jl).  The model
    owns its arrays: `points` and `scales` are copied, never aliased (the reference's `adopt`)."""
    if not 0 <= int(max_sh_degree) <= 3:
        raise ValueError(f"`max_sh_degree={max_sh_degree}` must be in `[0, 3]` range.")
    n = _check_points(points)
    dev = points.device
    if not (isinstance(colors, torch.Tensor) and colors.is_cuda and colors.device == dev and colors.dtype == torch.float32
            and tuple(colors.shape) == (n, 3)):
        raise ValueError("colors must be a float32 (N, 3) HIP tensor on the points' device")
    if scales is None:
        scales = compute_scales(points, point_size=point_size, isotropic=isotropic)
    else:
        if not (isinstance(scales, torch.Tensor) and scales.is_cuda and scales.device == dev and scales.dtype == torch.float32
                and scales.dim() == 2 and scales.shape[0] == n and scales.shape[1] in (1, 3)):
            raise ValueError("scales must be a float32 (N, 3) or (N, 1) HIP tensor on the points' device")
        if isotropic and scales.shape[1] == 3:  # mean(scales; dims=1)
            total = (scales[:, 0:1] + scales[:, 1:2]) + scales[:, 2:3]
            # (a tensor divisor: torch turns a division by a Python scalar into a product with its reciprocal)
            scales = total / torch.full_like(total, 3.0)
        else:
            scales = scales.clone()
    k = (int(max_sh_degree) + 1) ** 2
    features_dc = ((colors - 0.5) * float(f32(1) / SH0)).reshape(n, 1, 3).contiguous()  # rgb_2_sh (gaussians.jl:133), fp32
    features_rest = torch.zeros((n, k - 1, 3), dtype=torch.float32, device=dev)
    rotations = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    rotations[:, 0] = 1.0
    opacities = torch.full((n, 1), float(inverse_sigmoid(f32(0.1))), dtype=torch.float32, device=dev)
    ids = torch.zeros(n, dtype=torch.int32, device=dev) if use_ids else None
    return GaussianModel(points.clone(), features_dc, features_rest, scales.contiguous(), rotations, opacities, ids)
