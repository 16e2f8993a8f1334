"""Host mirror of what the reference makes of a frame's geometry channels: `depth_image` / `normal_image` and the per-view
loop of scripts/render-views.jl (:264-308, :390-407), the viewer's grey depth picture `gl_depth` / `to_depth`
(src/rasterization/rasterizer.jl:163-198) and `handle_pick!` (src/gui/worker.jl:688-726).  The per-pixel work and the exact
depth percentile run on the gsr_depth_scale / gsr_frame_depth16 / gsr_frame_normal8 / gsr_pick_point entry points
(csrc/frames.hip): the frame never leaves the device and no depth is sorted on the host.

Layouts: a frame is the rasterizer's (H, W, C) ≙ the reference's (C, W, H): channels 0..2 rgb, 3 depth, 4 alpha, 5..7 normal;
the depth picture is (H, W) uint16, the normal picture (H, W, 3) uint8; the statistics of `depth_scale` are one (4,) int32
device tensor {bits of the white level, n, bits of v[j], bits of v[j+1]}.  File I/O (PNG, depth-scales.csv, --skip-existing)
is not built: every function ends at the bytes."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _args as A
from . import _lib as L
from .camera import Camera

MIN_ALPHA = 1e-3          # render-views.jl MIN_ALPHA
VIEWER_DEPTH_MAX = 50.0   # rasterizer.jl:163-198: the raw depth channel times 1/50


def _check_frame(image, c_min: int):
    message = f"image must be a contiguous float32 (H, W, C >= {c_min}) HIP tensor"
    H, W, Cn = A.check(image, message, shape=(None, None, None)).shape
    if Cn < c_min:
        raise ValueError(message)
    return H, W, Cn


def _check_min_alpha(min_alpha):
    if not float(min_alpha) > 0.0:
        raise ValueError("min_alpha must be > 0")
    return float(min_alpha)


def _check_percentile(percentile):
    p = float(percentile)
    if not (0.0 < p <= 100.0):
        raise ValueError("percentile must be in (0, 100]")
    return p


def frames_scratch_bytes(W: int, H: int) -> int:
    return int(L.load().gsr_frames_scratch_bytes(int(W), int(H)))


_SCRATCH = A.FrameScratch(frames_scratch_bytes, align=8)  # depth_scale's histograms and keys


def depth_scale(image, percentile: float = 99.0, min_alpha: float = MIN_ALPHA, stats=None, scratch=None):
    """The white level of `depth_image` (render-views.jl:272-277) -> the (4,) int32 device tensor {bits of scale, n, bits of
    v[j], bits of v[j+1]} (`stats`, or a new one): the `percentile`-th of the expected depths D/α of the covered pixels
    (α >= min_alpha), Statistics.jl's `quantile` (definition 7) of exactly the two order statistics it interpolates, clamped
    to >= 1e-6; 1 when no pixel is covered.  Nothing is read back: `scale_of(stats)` views the white level as a float."""
    torch = A._torch()
    p, ma = _check_percentile(percentile), _check_min_alpha(min_alpha)   # the scalars first: refused whatever the tensors are
    H, W, Cn = _check_frame(image, 5)
    stats = torch.empty(4, dtype=torch.int32, device=image.device) if stats is None else \
        A.check_like(stats, "stats", (4,), image.device, torch.int32)
    buf = _SCRATCH.get(scratch, W, H, image.device)
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_depth_scale(W, H, Cn, image.data_ptr(), ma, p, stats.data_ptr(), buf.data_ptr(), L.stream()))
    return stats


def scale_of(stats):
    """The white level inside `depth_scale`'s statistics, as a (1,) float32 view on the device."""
    return stats[:1].view(A._torch().float32)


def frame_depth16(image, depth_max: float = 0.0, percentile: float = 99.0, expected: bool = True, min_alpha: float = MIN_ALPHA,
                  flip_rows: bool = False, out=None, stats=None, scratch=None):
    """The 16-bit depth picture of a frame -> ((H, W) uint16 (`out`, or a new tensor), statistics or None).  expected=True is
    `depth_image`: the expected depth D/α of the covered pixels, 0 elsewhere; expected=False the raw depth channel.  The white
    level is `depth_max` when > 0, else `depth_scale(image, percentile)` — handed on as a device pointer, with no read-back
    in between — and then the second result is its statistics tensor.  word = floor(clamp(x / scale, 0, 1) · 65535 + 0.5)."""
    torch = A._torch()
    ma = _check_min_alpha(min_alpha)
    depth_max = float(depth_max)
    if not (depth_max >= 0.0 and math.isfinite(depth_max)):
        raise ValueError("depth_max must be finite and >= 0")
    if depth_max == 0.0:
        _check_percentile(percentile)
    H, W, Cn = _check_frame(image, 5 if (expected or depth_max == 0.0) else 4)
    out = torch.empty((H, W), dtype=torch.uint16, device=image.device) if out is None else \
        A.check_like(out, "out", (H, W), image.device, torch.uint16)
    stats = depth_scale(image, percentile, ma, stats, scratch) if depth_max == 0.0 else None
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_frame_depth16(W, H, Cn, image.data_ptr(), 1 if expected else 0, ma, depth_max, L.ptr(stats),
                                           1 if flip_rows else 0, out.data_ptr(), L.stream()))
    return out, stats


def viewer_depth16(image, flip_rows: bool = False, out=None):
    """`to_depth` / `gl_depth` (rasterizer.jl:163-198) at 16 bits: the raw depth channel times 1/50, clamped."""
    return frame_depth16(image, depth_max=VIEWER_DEPTH_MAX, expected=False, flip_rows=flip_rows, out=out)[0]


def _rotation9(R_c2w):
    """A (3, 3) camera->world rotation -> the nine floats of the C entry point, column-major."""
    R = np.asarray(R_c2w, np.float32)
    if R.shape != (3, 3) or not np.isfinite(R).all():
        raise ValueError("R_c2w must be a finite (3, 3) matrix")
    return (C.c_float * 9)(*[float(R[r, c]) for c in range(3) for r in range(3)])


def frame_normal8(image, R_c2w=None, min_alpha: float = MIN_ALPHA, out=None):
    """`normal_image` (render-views.jl:291-308) -> (H, W, 3) uint8 (`out`, or a new tensor): the alpha-normalised normal,
    re-normalised to unit length, rotated by the host matrix `R_c2w` (3, 3) = transpose(camera.R) when given, encoded as
    0.5·(n + 1) with `frame_rgb8`'s quantiser; uncovered pixels and degenerate sums encode the zero vector (128)."""
    torch = A._torch()
    ma = _check_min_alpha(min_alpha)
    H, W, Cn = _check_frame(image, 8)
    rot = None if R_c2w is None else C.byref(_rotation9(R_c2w))
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=image.device) if out is None else \
        A.check_like(out, "out", (H, W, 3), image.device, torch.uint8)
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_frame_normal8(W, H, Cn, image.data_ptr(), ma, rot, out.data_ptr(), L.stream()))
    return out


def camera_struct(camera: Camera, W: int, H: int) -> L.CameraS:
    """The host fields `pick_point` reads: R (column-major), camera_center, focal, principal."""
    if (int(camera.width), int(camera.height)) != (W, H):
        raise ValueError("camera resolution does not match the image")
    cs = L.CameraS()
    R = np.asarray(camera.R, np.float32)
    cc = camera.camera_center
    for c in range(3):
        for r in range(3):
            cs.R[c * 3 + r] = float(R[r, c])
        cs.t[c] = float(camera.t[c])
        cs.camera_center[c] = float(cc[c])
    for k in range(2):
        cs.focal[k] = float(camera.focal[k])
        cs.principal[k] = float(camera.principal[k])
    if not (cs.focal[0] > 0 and cs.focal[1] > 0):
        raise ValueError("focal lengths must be positive")
    return cs


def pick_point(image, camera: Camera, px: int, py: int, half_window: int = 4, out=None):
    """`handle_pick!` (worker.jl:688-726) -> a (4,) device tensor {x, y, z, count}: the world point under the 1-based pixel
    (px, py), from the mean of the depths > 1e-2 in the (2·half_window + 1)² window around it, unprojected through the
    intrinsics and the pose; zeros when the window holds no such depth or the pixel lies outside the frame."""
    torch = A._torch()
    if not 0 <= int(half_window) <= 16:
        raise ValueError("half_window must be in [0, 16]")
    H, W, Cn = _check_frame(image, 4)
    cs = camera_struct(camera, W, H)
    out = torch.empty(4, dtype=torch.float32, device=image.device) if out is None else A.check_like(out, "out", (4,), image.device)
    with torch.cuda.device(image.device):
        L.check(L.load().gsr_pick_point(W, H, Cn, image.data_ptr(), C.byref(cs), int(px), int(py), int(half_window),
                                        out.data_ptr(), L.stream()))
    return out


def _read_back(t):
    """THE device -> host copy of `render_views`."""
    return t.cpu().numpy()


def render_views(rast, points, acts, rotations, cameras, sh_degree, depth_max: float = 0.0, percentile: float = 99.0,
                 world_normals: bool = False):
    """The loop body of scripts/render-views.jl (:390-407) for a list of cameras -> (rgb8 [(H, W, 3) uint8], depth16
    [(H, W) uint16], normal8 [(H, W, 3) uint8], scales [float]): per view ONE forward-only render of the :rgbdn rasterizer
    `rast` (zero background), then `frame_rgb8`, `frame_depth16` and `frame_normal8` into that view's device tensors.  `acts` =
    (shs, σ(opacities), exp(scales)) as `prologue_forward` returns them.  The white levels — `depth_max` when > 0, else each
    view's `percentile`-th covered depth — are read back ONCE, after the last view: the depth-scales.csv column."""
    torch = A._torch()
    from .evaluation import frame_rgb8
    if rast.mode != "rgbdn":
        raise ValueError("render_views needs an :rgbdn rasterizer: the normal picture reads channels 5..7")
    cameras = list(cameras)
    depth_max = float(depth_max)
    if not (depth_max >= 0.0 and math.isfinite(depth_max)):
        raise ValueError("depth_max must be finite and >= 0")
    _check_percentile(percentile)
    shs, opacities_act, scales_act = acts
    W, H, dev = rast.width, rast.height, points.device
    rgb, depth, normal = [], [], []
    if not cameras:
        return rgb, depth, normal, []
    stats = torch.zeros((len(cameras), 4), dtype=torch.int32, device=dev)
    scratch = torch.empty(frames_scratch_bytes(W, H), dtype=torch.uint8, device=dev) if depth_max == 0.0 else None
    for v, camera in enumerate(cameras):
        image = rast.forward_raw(points, shs, opacities_act, scales_act, rotations, camera, sh_degree, (0.0, 0.0, 0.0),
                                 forward_only=True)
        rgb.append(frame_rgb8(image))
        depth.append(frame_depth16(image, depth_max, percentile, stats=stats[v], scratch=scratch)[0])
        normal.append(frame_normal8(image, np.asarray(camera.R, np.float32).T if world_normals else None))
    if depth_max > 0.0:
        return rgb, depth, normal, [float(np.float32(depth_max))] * len(cameras)
    scales = np.ascontiguousarray(_read_back(stats)[:, 0]).view(np.float32)
    return rgb, depth, normal, [float(s) for s in scales]
