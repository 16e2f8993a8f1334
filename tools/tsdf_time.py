"""Times the TSDF fusion and the surface-nets extraction (csrc/tsdf.hip through surface_mesh) beside the same results computed
with torch operations on the same device:

  integrate : one 1920 x 1080 frame of an analytic unit sphere into a 512 x 512 x 256 volume, with and without colour, vs.
              `torch_integrate` below (the per-sample definition as whole-volume tensor expressions);
  extract   : gsr_mesh_count + the read-back of the counts + gsr_mesh_emit on the volume fused from five views, vs.
              `torch_extract` (masks, cumulative sums, nonzero, gathers).

`integrate` is also expressed as the bytes it must touch — 16 per fused sample, 40 with colour — over the measured copy rate of
the device (6.29 TB/s).  Device milliseconds are between two device events on the current stream: the median of `--runs` timed
runs after `--warmup` untimed ones.  The torch results are compared with the kernels' before anything is timed.  Not part of
bench.py; run it under a timeout of its own:

    timeout 900 python tools/tsdf_time.py [--out profiles/tsdf/times.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12   # bytes / s, float4 copy


def median_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def look_at_origin(pkg, centre, W, H, f):
    c = np.asarray(centre, np.float64)
    z = -c / np.linalg.norm(c)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[2]) >= 0.9 else np.array([0.0, 0.0, 1.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return pkg.Camera(W, H, (f, f), (0.5, 0.5), R.astype(np.float32), (-R @ c).astype(np.float32))


def sphere_frame(cam, device):
    """(H, W, 5): alpha = 1 where the pixel's ray hits the unit sphere at the origin, D its z-depth, rgb = 0.5 + 0.5·normal."""
    W, H = cam.width, cam.height
    R = torch.tensor(np.asarray(cam.R, np.float64), device=device)
    t = torch.tensor(np.asarray(cam.t, np.float64), device=device)
    jj, ii = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float64), torch.arange(W, device=device, dtype=torch.float64),
                            indexing="ij")
    d = torch.stack([(ii - cam.principal[0] * W) / cam.focal[0], (jj - cam.principal[1] * H) / cam.focal[1], torch.ones_like(ii)], -1)
    dd, dt = (d * d).sum(-1), d @ t
    disc = dt * dt - dd * (t @ t - 1.0)
    hit = disc > 0
    s = (dt - torch.sqrt(disc.clamp_min(0.0))) / dd
    normal = (s[..., None] * d - t) @ R
    img = torch.zeros((H, W, 5), dtype=torch.float32, device=device)
    img[..., :3] = torch.where(hit[..., None], 0.5 + 0.5 * normal, torch.zeros_like(normal)).float()
    img[..., 3] = torch.where(hit, s, torch.zeros_like(s)).float()
    img[..., 4] = hit.float()
    return img


def torch_integrate(volume, color, origin, h, trunc, image, cam, min_alpha, near):
    """gsr_tsdf_integrate as tensor expressions over the whole volume (in place)."""
    nz, ny, nx = volume.shape[:3]
    H, W = image.shape[:2]
    dev = volume.device
    R, t = np.asarray(cam.R, np.float32), np.asarray(cam.t, np.float32)
    px = (float(origin[0]) + h * torch.arange(nx, device=dev, dtype=torch.float32))[None, None, :]
    py = (float(origin[1]) + h * torch.arange(ny, device=dev, dtype=torch.float32))[None, :, None]
    pz = (float(origin[2]) + h * torch.arange(nz, device=dev, dtype=torch.float32))[:, None, None]
    pc = [((float(R[r, 0]) * px + float(R[r, 1]) * py) + float(R[r, 2]) * pz) + float(t[r]) for r in range(3)]
    z = pc[2]
    u = (float(cam.focal[0]) * pc[0]) / z + float(np.float32(cam.principal[0]) * np.float32(W))
    v = (float(cam.focal[1]) * pc[1]) / z + float(np.float32(cam.principal[1]) * np.float32(H))
    fu, fv = torch.floor(u + 0.5), torch.floor(v + 0.5)
    ok = (z > near) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    pix = torch.where(ok, fv * W + fu, torch.zeros_like(fu)).long()
    flat = image.view(-1, image.shape[2])
    alpha = flat[:, 4][pix]
    ok &= alpha >= min_alpha
    sdf = flat[:, 3][pix] / alpha - z
    ok &= sdf >= -trunc
    s = torch.clamp_max(sdf / trunc, 1.0)
    tsdf, w = volume[..., 0], volume[..., 1]
    w1 = w + 1.0
    if color is not None:
        q = (flat[:, :3][pix] / alpha[..., None]).clamp(0.0, 1.0)
        color.copy_(torch.where(ok[..., None], (color * w[..., None] + q) / w1[..., None], color))
    volume[..., 0] = torch.where(ok, (tsdf * w + s) / w1, tsdf)
    volume[..., 1] = torch.where(ok, w1, w)
    return int(ok.sum())


def _corner(a, dx, dy, dz):
    nz, ny, nx = a.shape[:3]
    return a[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1]


def torch_extract(volume, origin, h):
    """gsr_mesh_count + gsr_mesh_emit (no colours) as tensor expressions -> (vertices (M, 3), faces (F, 3) int32)."""
    tsdf, weight = volume[..., 0], volume[..., 1]
    dev = volume.device
    inside, obs = tsdf < 0, weight > 0
    corners = [(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)]
    all_obs = _corner(obs, *corners[0]).clone()
    n_in = _corner(inside, *corners[0]).to(torch.int8)
    for c in corners[1:]:
        all_obs &= _corner(obs, *c)
        n_in += _corner(inside, *c)
    active = all_obs & (n_in > 0) & (n_in < 8)
    K, J, I = torch.nonzero(active, as_tuple=True)                    # ascending cell index
    vid = torch.full(active.shape, -1, dtype=torch.int32, device=dev)
    vid[K, J, I] = torch.arange(K.numel(), dtype=torch.int32, device=dev)
    s = [torch.zeros(K.numel(), device=dev) for _ in range(3)]
    n = torch.zeros(K.numel(), device=dev)
    for axis in range(3):
        for e in range(4):
            lo, hi = e & 1, e >> 1
            a = [(0, lo, hi), (lo, 0, hi), (lo, hi, 0)][axis]
            b = tuple(a[d] + (1 if d == axis else 0) for d in range(3))
            Ta, Tb = tsdf[K + a[2], J + a[1], I + a[0]], tsdf[K + b[2], J + b[1], I + b[0]]
            cross = (Ta < 0) != (Tb < 0)
            t = Ta / (Ta - Tb)
            for d in range(3):
                s[d] = torch.where(cross, s[d] + (t if d == axis else float(a[d])), s[d])
            n += cross
    verts = torch.stack([float(origin[d]) + h * (idx.float() + s[d] / n) for d, idx in enumerate((I, J, K))], -1)
    quads = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        e = [0, 0, 0]
        e[a] = 1
        m = _corner(obs, 0, 0, 0) & _corner(obs, *e) & (_corner(inside, 0, 0, 0) != _corner(inside, *e))
        k, j, i = torch.nonzero(m, as_tuple=True)
        p = [i, j, k]
        keep = (p[b] >= 1) & (p[c] >= 1)
        p = [x[keep] for x in p]
        ids = []
        for n_ in range(4):      # c0 = p - e_b - e_c, c1 = p - e_c, c2 = p, c3 = p - e_b
            q = list(p)
            if n_ in (0, 3):
                q[b] = q[b] - 1
            if n_ in (0, 1):
                q[c] = q[c] - 1
            ids.append(vid[q[2], q[1], q[0]])
        ids = torch.stack(ids, -1)
        keep = (ids >= 0).all(-1)
        ids, p = ids[keep], [x[keep] for x in p]
        ids = torch.where(inside[p[2], p[1], p[0]][:, None], ids, ids.flip(-1))
        key = 3 * (p[0].long() + tsdf.shape[2] * (p[1].long() + tsdf.shape[1] * p[2].long())) + a
        quads.append((key, ids))
    key = torch.cat([q[0] for q in quads])
    ids = torch.cat([q[1] for q in quads])[torch.argsort(key)]
    faces = torch.stack([ids[:, [0, 1, 2]], ids[:, [0, 2, 3]]], 1).reshape(-1, 3)
    return verts, faces.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=[512, 512, 256])
    ap.add_argument("--frame", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gsr_pkg
    pkg = gsr_pkg.load()
    SM = pkg.surface_mesh
    dev = torch.device("cuda", torch.cuda.current_device())
    nx, ny, nz = args.dims
    W, H = args.frame
    h = 2.6 / (max(nx, ny) - 1)
    origin, trunc = (-1.3, -1.3, -1.3), 4.0 * h
    f = 0.45 * W
    cams = [look_at_origin(pkg, c, W, H, f) for c in ((0, 0, -3.0), (3.0, 0, -0.6), (-3.0, 0, -0.6), (0, 3.0, -0.6), (0, -3.0, -0.6))]
    frames = [sphere_frame(cam, dev) for cam in cams]
    n = nx * ny * nz
    lines = [f"device: {torch.cuda.get_device_name(0)}; volume {nx} x {ny} x {nz} = {n} samples, h = {h:.5f}, trunc = 4 h; frame {W} x {H}; "
             f"median (min .. max) of {args.runs} runs after {args.warmup} warm-up runs, device events"]

    for color in (False, True):
        vol = SM.TSDFVolume(args.dims, origin, h, trunc, color=color, device=dev)
        ref_v = vol.volume.clone()
        ref_c = None if vol.color is None else vol.color.clone()
        vol.integrate(frames[0], cams[0])
        touched = torch_integrate(ref_v, ref_c, origin, vol.voxel_size, vol.trunc, frames[0], cams[0], float(np.float32(SM.MIN_ALPHA)), SM.NEAR)
        torch.cuda.synchronize()
        same_w = bool(torch.equal(vol.volume[..., 1], ref_v[..., 1]))
        worst = float((vol.volume[..., 0] - ref_v[..., 0]).abs().max())
        worst_c = 0.0 if ref_c is None else float((vol.color - ref_c).abs().max())
        hip = median_ms(lambda: vol.integrate(frames[0], cams[0]), args.warmup, args.runs)
        tor = median_ms(lambda: torch_integrate(ref_v, ref_c, origin, vol.voxel_size, vol.trunc, frames[0], cams[0],
                                                float(np.float32(SM.MIN_ALPHA)), SM.NEAR), 1, max(3, args.runs // 4))
        nbytes = touched * (40 if color else 16)
        floor_ms = nbytes / COPY_RATE * 1e3
        lines.append(f"integrate, colour {'on ' if color else 'off'}: HIP {hip[0]:7.3f} ms ({hip[1]:.3f} .. {hip[2]:.3f}); {touched} of {n} samples fused, "
                     f"{nbytes / 1e6:.0f} MB touched = {floor_ms:.3f} ms at 6.29 TB/s: {floor_ms / hip[0]:.2f} of the copy rate; "
                     f"torch {tor[0]:8.3f} ms ({tor[1]:.3f} .. {tor[2]:.3f}); torch / HIP = {tor[0] / hip[0]:.1f}; same weights as torch: {same_w}, "
                     f"worst |tsdf - torch| {worst:.1e}, colour {worst_c:.1e}")
        print(lines[-1], flush=True)
        del ref_v, ref_c
        if color:
            continue
        # the fused result: five views, then the extraction
        vol.reset()
        for frame, cam in zip(frames, cams):
            vol.integrate(frame, cam)
        mesh = SM.extract_mesh(vol)
        t_v, t_f = torch_extract(vol.volume, origin, vol.voxel_size)
        torch.cuda.synchronize()
        same_f = bool(t_f.shape == mesh.faces.shape and torch.equal(t_f, mesh.faces))
        worst = float((t_v - mesh.vertices).abs().max()) if t_v.shape == mesh.vertices.shape else float("nan")
        hip = median_ms(lambda: SM.extract_mesh(vol), args.warmup, args.runs)
        tor = median_ms(lambda: torch_extract(vol.volume, origin, vol.voxel_size), 1, max(3, args.runs // 4))
        lines.append(f"count + read-back + emit: HIP {hip[0]:7.3f} ms ({hip[1]:.3f} .. {hip[2]:.3f}); {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces; "
                     f"{n * 8 / 1e6:.0f} MB of volume = {n * 8 / COPY_RATE * 1e3:.3f} ms at 6.29 TB/s; torch {tor[0]:8.3f} ms ({tor[1]:.3f} .. {tor[2]:.3f}); "
                     f"torch / HIP = {tor[0] / hip[0]:.1f}; same faces as torch: {same_f}, worst |vertex - torch| {worst:.1e}")
        print(lines[-1], flush=True)
        del t_v, t_f, mesh
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
