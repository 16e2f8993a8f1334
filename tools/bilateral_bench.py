#!/usr/bin/env python3
"""Device times of the bilateral grid kernels at the reference's default setting: slice forward, slice
backward (∇image in place + the full ∇grid of the view) and the fused TV + Adam tail over all grids, at 1920x1080,
16x16x8, n = 200 training images.  HIP events around `--iters` launches each, after `--warmup` launches.  Prints one
JSON line with the per-launch milliseconds and the algorithmic bytes of each kernel.  The launches are issued from
Python; a `rocprofv3 --kernel-trace --stats` run of this tool gives the same per-kernel times, so at
these kernel lengths the events measure the device, not the host's submission rate."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--grid", type=int, nargs=3, default=(16, 16, 8))
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()

    import numpy as np
    import torch
    import gsr_pkg
    pkg = gsr_pkg.load()
    bg = pkg.bilateral_grid
    W, H, (gx, gy, gz), n = a.width, a.height, a.grid, a.images
    r = np.random.default_rng(0)
    d = lambda x: torch.as_tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
    image = d(r.uniform(0, 1, (H, W, 3)).astype(np.float32))
    vout = d(r.normal(0, 1e-6, (H, W, 3)).astype(np.float32))
    B = bg.BilateralGrid(n, (gx, gy, gz), device="cuda")
    B.grids.add_(d(r.normal(0, 0.01, tuple(B.grids.shape)).astype(np.float32)))
    view = 3

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

    out = torch.empty_like(image)
    vimg = torch.empty_like(image)
    fwd = timed(lambda: bg.slice_forward(image, B.grid(view), out=out))
    bwd = timed(lambda: B.slice_backward_(image, view, vimg.copy_(vout)))
    copy = timed(lambda: vimg.copy_(vout))
    vg = B.vgrid.clone()

    def tail():
        B.vgrid_view = view
        B.step(view, 5000)
    tl = timed(tail)
    assert torch.equal(vg, B.vgrid)
    P, G = W * H, gx * gy * gz * 12
    res = dict(width=W, height=H, grid=[gx, gy, gz], images=n, iters=a.iters,
               slice_fwd_ms=round(fwd, 5), slice_bwd_ms=round(bwd - copy, 5), adam_tail_ms=round(tl, 5),
               total_ms=round(fwd + bwd - copy + tl, 5),
               # algorithmic bytes: image read + out written (fwd); image + cotangent read, ∇image written (bwd);
               # θ, μ, ν read and written, the view's ∇grid read (tail)
               slice_fwd_mb=round(2 * P * 12 / 1e6, 2), slice_bwd_mb=round(3 * P * 12 / 1e6, 2),
               adam_tail_mb=round((6 * n * G + G) * 4 / 1e6, 2),
               tv_loss=float(B.tv_term.item()), device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
