"""One surface of the scene from its rendered depth: TSDF fusion of the :rgbd / :rgbdn frames and naive surface-nets mesh
extraction on the gsr_tsdf_integrate / gsr_mesh_count / gsr_mesh_emit entry points (csrc/tsdf.hip) — the step
every 2DGS / GOF / PGSR-style pipeline ends with, without a frame leaving the device.

    volume = TSDFVolume.around(points, resolution=512, margin=0.1)
    fuse_views(rast, points, (shs, oa, sa), rotations, cameras, sh_degree, volume)     # one forward-only render per view
    mesh = extract_mesh(volume)                                                        # ONE read-back: the two counts
    data = mesh_ply_bytes(mesh)

Layouts: the volume is (nz, ny, nx, 2) float32 {tsdf, weight} — sample (i, j, k) at origin + voxel_size·(i, j, k), x fastest —,
the optional colour volume (nz, ny, nx, 3); a frame is the rasterizer's (H, W, C >= 5): 0..2 rgb, 3 the depth sum D, 4 alpha.
A sample is fused with the expected depth D/α of the pixel it projects to (pixel i samples u = i, the rasterizer's
convention), wherever α >= min_alpha and the sample is not more than `trunc` behind that depth.  Views are fused in call order;
everything is run-to-run bit-identical.  There is no CPU path.  File I/O is not built: `mesh_ply_bytes` ends at the bytes."""
from __future__ import annotations

import collections
import ctypes as C
import math

import numpy as np

from . import _args as A
from . import _lib as L
from .geometry_frames import MIN_ALPHA, camera_struct

NEAR = 0.2
MAX_DIM = 65535            # a side of the volume (include/gsr.h)
MAX_MESH_SAMPLES = 1 << 30

Mesh = collections.namedtuple("Mesh", "vertices faces colors")   # (M, 3) float32, (F, 3) int32, (M, 3) float32 | None


def _read_back(t):
    """THE device -> host copy of this module: the two counts of `extract_mesh`, the box of `TSDFVolume.around`."""
    return t.cpu().numpy()


def _positive(x, name):
    x = float(np.float32(x))
    if not (x > 0.0 and math.isfinite(x)):
        raise ValueError(f"{name} must be finite and > 0")
    return x


class TSDFVolume:
    """A dense truncated-signed-distance volume on the device: `dims` = (nx, ny, nz) samples, sample (i, j, k) at
    origin + voxel_size·(i, j, k).  `volume` (nz, ny, nx, 2) holds {tsdf, weight}, `color` (nz, ny, nx, 3) or None."""

    def __init__(self, dims, origin, voxel_size, trunc, color: bool = False, device="cuda"):
        torch = A._torch()
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) < 1 or max(dims) > MAX_DIM:
            raise ValueError(f"dims must be three sample counts in [1, {MAX_DIM}]")
        origin = np.asarray(origin, np.float32)
        if origin.shape != (3,) or not np.isfinite(origin).all():
            raise ValueError("origin must be three finite numbers")
        self.dims, self.origin = dims, origin
        self.voxel_size, self.trunc = _positive(voxel_size, "voxel_size"), _positive(trunc, "trunc")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("a TSDFVolume lives on a HIP device (no CPU path)")
        if self.device.index is None:   # "cuda": the current device, named, so that it compares equal to a tensor's
            self.device = torch.device("cuda", torch.cuda.current_device())
        nx, ny, nz = dims
        self.volume = torch.empty((nz, ny, nx, 2), dtype=torch.float32, device=self.device)
        self.color = torch.empty((nz, ny, nx, 3), dtype=torch.float32, device=self.device) if color else None
        self._origin_c = (C.c_float * 3)(*[float(x) for x in origin])
        self.reset()

    @classmethod
    def around(cls, points, resolution: int, margin: float = 0.0, trunc=None, color: bool = False):
        """The box of a model's points (N, 3), grown by `margin` world units on every side, sampled with `resolution` samples
        along its longest side (the other sides: as many as cover them); trunc defaults to 4 voxels.  One small read-back: the
        minimum and the maximum."""
        torch = A._torch()
        A.check(points, "points must be a contiguous float32 (N, 3) HIP tensor", shape=(None, 3))
        resolution = int(resolution)
        if points.shape[0] < 1 or not 2 <= resolution <= MAX_DIM:
            raise ValueError(f"around needs at least one point and a resolution in [2, {MAX_DIM}]")
        margin = float(margin)
        if not (margin >= 0.0 and math.isfinite(margin)):
            raise ValueError("margin must be finite and >= 0")
        box = _read_back(torch.stack([points.min(0).values, points.max(0).values])).astype(np.float64)
        if not np.isfinite(box).all():
            raise ValueError("the points are not finite")
        lo, hi = box[0] - margin, box[1] + margin
        longest = float((hi - lo).max())
        if not longest > 0.0:
            raise ValueError("the box of the points is empty: give a margin")
        h = longest / (resolution - 1)
        dims = [min(resolution, int(math.ceil(e / h - 1e-9)) + 1) for e in (hi - lo)]
        return cls(dims, lo, h, 4.0 * h if trunc is None else trunc, color, points.device)

    def reset(self):
        """tsdf = 1, weight = 0, colour 0."""
        torch = A._torch()
        self.volume.copy_(torch.tensor([1.0, 0.0], dtype=torch.float32, device=self.device).expand_as(self.volume))
        if self.color is not None:
            self.color.zero_()
        return self

    def integrate(self, image, camera, min_alpha: float = MIN_ALPHA, near: float = NEAR):
        """Fuses one frame (H, W, C >= 5) of `camera` into the volume (gsr_tsdf_integrate).  Asynchronous; nothing is read back."""
        torch = A._torch()
        message = "image must be a contiguous float32 (H, W, C >= 5) HIP tensor on the volume's device"
        H, W, Cn = A.check(image, message, shape=(None, None, None), device=self.device).shape
        if Cn < 5:
            raise ValueError(message)
        if not float(min_alpha) > 0.0:
            raise ValueError("min_alpha must be > 0")
        if math.isnan(float(near)):
            raise ValueError("near must be a number")
        cs = camera_struct(camera, W, H)
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            L.check(L.load().gsr_tsdf_integrate(nx, ny, nz, self._origin_c, self.voxel_size, self.trunc, W, H, Cn, L.ptr(image),
                                                C.byref(cs), float(min_alpha), float(near), L.ptr(self.volume), L.ptr(self.color),
                                                L.stream()))
        return self


def fuse_views(rast, points, acts, rotations, cameras, sh_degree, volume: TSDFVolume):
    """The loop of `geometry_frames.render_views` into a volume: per view ONE forward-only render of the :rgbd / :rgbdn
    rasterizer `rast` (zero background), then `volume.integrate`.  `acts` = (shs, σ(opacities), exp(scales)) as
    `prologue_forward` returns them.  Nothing is read back.  -> volume."""
    if rast.mode == "rgb":
        raise ValueError("fuse_views needs an :rgbd or :rgbdn rasterizer: the fusion reads the depth and alpha channels")
    if not isinstance(volume, TSDFVolume):
        raise ValueError("volume must be a TSDFVolume")
    shs, opacities_act, scales_act = acts
    for camera in cameras:
        image = rast.forward_raw(points, shs, opacities_act, scales_act, rotations, camera, sh_degree, (0.0, 0.0, 0.0),
                                 forward_only=True)
        volume.integrate(image, camera)
    return volume


def mesh_scratch_bytes(dims) -> int:
    return int(L.load().gsr_mesh_scratch_bytes(*[int(d) for d in dims]))


def extract_mesh(volume: TSDFVolume) -> Mesh:
    """Naive surface nets of the volume -> Mesh(vertices (M, 3) float32, faces (F, 3) int32, colors (M, 3) float32 | None), device
    tensors: one vertex per active cell (8 observed corners, not all on one side) at the mean of its edge crossings, one quad =
    two triangles per sign-changing grid edge between four active cells, wound so that the normal points from inside
    (tsdf < 0) to outside.  gsr_mesh_count, ONE read-back of the two counts, an exact allocation, gsr_mesh_emit."""
    torch = A._torch()
    if not isinstance(volume, TSDFVolume):
        raise ValueError("volume must be a TSDFVolume")
    nx, ny, nz = volume.dims
    if nx * ny * nz > MAX_MESH_SAMPLES:
        raise ValueError("the extraction indexes at most 2^30 samples")
    dev = volume.device
    lib = L.load()
    nb = mesh_scratch_bytes(volume.dims)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)   # (torch allocations are 256-byte aligned)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.gsr_mesh_count(nx, ny, nz, L.ptr(volume.volume), L.ptr(counts), L.ptr(scratch, empty_is_null=True), nb, L.stream()))
        m, q = (int(x) for x in _read_back(counts))
        vertices = torch.empty((m, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((2 * q, 3), dtype=torch.int32, device=dev)
        colors = None if volume.color is None else torch.empty((m, 3), dtype=torch.float32, device=dev)
        if m > 0:
            L.check(lib.gsr_mesh_emit(nx, ny, nz, volume._origin_c, volume.voxel_size, L.ptr(volume.volume), L.ptr(volume.color),
                                      L.ptr(scratch), nb, m, 2 * q, L.ptr(vertices), L.ptr(colors), L.ptr(faces, empty_is_null=True),
                                      L.stream()))
    return Mesh(vertices, faces, colors)


def _quantize8(x: np.ndarray) -> np.ndarray:
    """`frame_rgb8`'s quantiser rule (csrc/quant_level.h): floor(clamp(x, 0, 1)·255 + 0.5), each step one fp32 operation."""
    f32 = np.float32
    return np.floor(np.fmin(np.fmax(x.astype(f32), f32(0)), f32(1)) * f32(255) + f32(0.5)).astype(np.uint8)


def mesh_ply_bytes(mesh: Mesh) -> bytes:
    """The mesh as binary little-endian PLY bytes: vertex x / y / z (float), red / green / blue (uchar, when the mesh has
    colours), and the face list (uchar count, int indices).  Reads the mesh back; tensors on any device."""
    torch = A._torch()
    v, f, c = mesh.vertices, mesh.faces, mesh.colors
    if not (isinstance(v, torch.Tensor) and v.dtype == torch.float32 and v.dim() == 2 and v.shape[1] == 3):
        raise ValueError("vertices must be a float32 (M, 3) tensor")
    if not (isinstance(f, torch.Tensor) and f.dtype == torch.int32 and f.dim() == 2 and f.shape[1] == 3):
        raise ValueError("faces must be an int32 (F, 3) tensor")
    if c is not None and not (isinstance(c, torch.Tensor) and c.dtype == torch.float32 and c.shape == v.shape):
        raise ValueError("colors must be a float32 (M, 3) tensor or None")
    m, n = int(v.shape[0]), int(f.shape[0])
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {m}", "property float x", "property float y", "property float z"]
    vdt = [("p", "<f4", 3)]
    if c is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
        vdt.append(("c", "u1", 3))
    head += [f"element face {n}", "property list uchar int vertex_indices", "end_header"]
    vert = np.zeros(m, np.dtype(vdt))
    vert["p"] = _read_back(v)
    if c is not None:
        vert["c"] = _quantize8(_read_back(c))
    face = np.zeros(n, np.dtype([("n", "u1"), ("v", "<i4", 3)]))
    face["n"] = 3
    face["v"] = _read_back(f)
    return ("\n".join(head) + "\n").encode("ascii") + vert.tobytes() + face.tobytes()
