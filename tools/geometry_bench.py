#!/usr/bin/env python3
"""Device times of the geometry regularisation kernels at 1920x1080: the depth-normal consistency forward
(tile pass + the one-workgroup final pass), its backward (onto channels 3..7 of a cotangent) and the flatten loss with its
gradient over `--gaussians` Gaussians.  HIP events around `--iters` launches each, after `--warmup` launches.  Prints one
JSON line with the per-launch milliseconds, the algorithmic bytes of each kernel and its rate against the STREAM triad
(gsr_stream_triad) measured in the same process.

The launches rotate over `--frames` frames (default 6 x 66 MB > the 256 MiB Infinity Cache), so that a frame is not still
on-die from the launch before: the rates are against memory, as the triad's.  A `rocprofv3 --kernel-trace --stats` run of
this tool gives the per-kernel split."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--focal", type=float, default=1000.0)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()

    import numpy as np
    import torch
    import gsr_pkg
    import geometry_torch as gt
    pkg = gsr_pkg.load()
    G, L = pkg.geometry_regularization, pkg._lib
    W, H, n = a.width, a.height, a.gaussians
    cam = pkg.Camera(W, H, (a.focal, a.focal))
    frames = [torch.as_tensor(gt.noisy_frame(W, H, a.focal, seed=k)).cuda() for k in range(a.frames)]
    vps = [torch.zeros_like(f) for f in frames]
    scr = [torch.empty(G.normal_loss_scratch_bytes(W, H), dtype=torch.uint8, device="cuda") for _ in frames]
    scales = torch.as_tensor(np.random.default_rng(0).normal(-3.0, 1.0, (n, 3)).astype(np.float32)).cuda()
    vscales = torch.zeros((n, 3), device="cuda")
    k = [0]

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    def fwd():
        i = k[0] = (k[0] + 1) % a.frames
        return G.depth_normal_loss(frames[i], cam, 0.05, scratch=scr[i])

    def bwd():
        i = k[0] = (k[0] + 1) % a.frames
        G.depth_normal_loss_backward_(frames[i], cam, vps[i], 0.05, scratch=scr[i])

    t_fwd = timed(fwd)
    for i in range(a.frames):          # every scratch holds its frame's scalars before the backward is timed
        k[0] = i - 1
        fwd()
    t_bwd = timed(bwd)
    t_flat = timed(lambda: G.flatten_loss(scales, 0.005, vscales=vscales))
    loss = float(fwd().item())

    lib = L.load()
    n_tri = 128 * 1024 * 1024
    ta, tb, tc = (torch.ones(n_tri, device="cuda") for _ in range(3))
    cs = torch.cuda.current_stream().cuda_stream
    t_tri = timed(lambda: L.check(lib.gsr_stream_triad(ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), n_tri, 0.5, cs)))
    triad = 12.0 * n_tri / (t_tri * 1e-3) / 1e9

    P = W * H
    valid = float((G.depth_normal_loss(frames[0], cam, 0.05, stats=True, scratch=scr[0])[1][1] / ((W - 2) * (H - 2))).item())
    # algorithmic bytes: the 32-byte record of every pixel read (fwd); the record read + channels 3..7 of the cotangent
    # read and written on the pixels that receive something, counted as whole records since 128-byte lines move whole
    # (bwd, an upper bound: untouched lines are not written); raw scales read, ∇scales read and written (flatten)
    mb = dict(fwd=P * 32 / 1e6, bwd=3 * P * 32 / 1e6, flatten=n * 36 / 1e6)
    ms = dict(fwd=t_fwd, bwd=t_bwd, flatten=t_flat)
    res = dict(width=W, height=H, focal=a.focal, gaussians=n, frames=a.frames, iters=a.iters, valid_fraction=round(valid, 4),
               normal_fwd_ms=round(t_fwd, 5), normal_bwd_ms=round(t_bwd, 5), flatten_ms=round(t_flat, 5),
               normal_fwd_mb=round(mb["fwd"], 2), normal_bwd_mb=round(mb["bwd"], 2), flatten_mb=round(mb["flatten"], 2),
               triad_gbs=round(triad, 1), loss=loss, device=torch.cuda.get_device_name(0))
    for key in ("fwd", "bwd", "flatten"):
        gbs = mb[key] / ms[key]      # MB / ms = GB/s
        res[f"{key}_gbs"] = round(gbs, 1)
        res[f"{key}_of_triad"] = round(gbs / triad, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
