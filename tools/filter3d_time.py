"""Times the 3-D smoothing filter (csrc/filter3d.hip through smoothing_filter) beside the same results computed with torch
operations on the same device — the per-camera loop of N-sized temporaries the original code runs:

  sweep : compute_filter_3d at N = 1 000 000 against V = 32 and V = 256 cameras (the three kernels of gsr_filter3d_compute)
          vs. `torch_sweep` below;
  apply : apply_filter_3d_forward + apply_filter_3d_backward at N = 1 000 000 vs. the torch expressions and their autograd.

Device milliseconds are between two device events on the current stream: the median of `--runs` timed runs after `--warmup`
untimed ones.  The torch results are compared with the kernels' before anything is timed.  Not part of bench.py; run it under
a timeout of its own:

    timeout 600 python tools/filter3d_time.py [--out profiles/filter3d/times.txt]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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


def ring_of_cameras(pkg, V, W=1920, H=1080):
    """V cameras on a circle of radius 6 around the origin, looking at it."""
    cams = []
    f = 0.5 * W / math.tan(math.radians(30.0))
    for v in range(V):
        a = 2.0 * math.pi * v / V
        c = np.array([6.0 * math.sin(a), 0.4 * math.sin(3 * a), -6.0 * math.cos(a)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        up = np.cross(fwd, right)
        R = np.stack([right, up, fwd])
        cams.append(pkg.Camera(W, H, (f, f * 1.01), (0.5, 0.5), R.astype(np.float32), (-R @ c).astype(np.float32)))
    return cams


def torch_sweep(points, table, near, k):
    """The original's loop: one pass of torch operations per camera over N-sized temporaries."""
    n = points.shape[0]
    tmin = torch.full((n,), float("inf"), device=points.device)
    seen = torch.zeros(n, dtype=torch.bool, device=points.device)
    p0, p1, p2 = points[:, 0], points[:, 1], points[:, 2]
    for c in table:   # a host table: the scalars are Python floats
        xc = [((c[i] * p0 + c[i + 3] * p1) + c[i + 6] * p2) + c[9 + i] for i in range(3)]
        z = xc[2]
        valid = z > near
        for j in range(2):
            u = c[12 + j] * xc[j] + c[14 + j] * z
            valid = valid & (c[16 + j] * z <= u) & (u <= c[18 + j] * z)
        tmin = torch.where(valid, torch.minimum(tmin, z * c[20]), tmin)
        seen |= valid
    filt = k * tmin
    fill = torch.where(seen, filt, torch.zeros_like(filt)).max()
    return torch.where(seen, filt, fill), seen


def torch_apply(o, s, f):
    se = torch.sqrt(s * s + (f * f)[:, None])
    return o * (s / se).prod(1, keepdim=True), se


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gsr_pkg
    pkg = gsr_pkg.load()
    SF = pkg.smoothing_filter
    n = args.n
    rng = np.random.default_rng(20)
    pts = torch.from_numpy((rng.standard_normal((n, 3)) * 2.0).astype(np.float32)).cuda()
    lines = [f"device: {torch.cuda.get_device_name(0)}; N = {n}; median (min .. max) of {args.runs} runs after {args.warmup} warm-up runs, device events"]
    filt = None
    for V in args.views:
        table_h = SF.camera_table(ring_of_cameras(pkg, V))
        table = torch.from_numpy(table_h).cuda()
        rows = [[float(x) for x in r] for r in table_h]
        k = float(SF.filter_scale())
        filt, seen, count = SF.compute_filter_3d(pts, table, return_seen=True)
        t_filt, t_seen = torch_sweep(pts, rows, SF.NEAR, k)
        torch.cuda.synchronize()
        same_seen = bool((seen.bool() == t_seen).all())
        worst = float(((filt - t_filt).abs() / t_filt.abs().clamp_min(1e-30)).max())
        hip = median_ms(lambda: SF.compute_filter_3d(pts, table), args.warmup, args.runs)
        tor = median_ms(lambda: torch_sweep(pts, rows, SF.NEAR, k), args.warmup, max(3, args.runs // 4))
        pairs = n * V
        lines.append(f"sweep V = {V:3d}: HIP {hip[0]:8.3f} ms ({hip[1]:.3f} .. {hip[2]:.3f}), {pairs / hip[0] / 1e6:.1f} G pairs/s; "
                     f"torch loop {tor[0]:9.3f} ms ({tor[1]:.3f} .. {tor[2]:.3f}); torch / HIP = {tor[0] / hip[0]:.1f}; "
                     f"seen {int(count.item())} of {n}, same seen flags as torch: {same_seen}, worst relative difference {worst:.1e}")
        print(lines[-1], flush=True)
    o = torch.from_numpy(rng.uniform(0.004, 0.999, (n, 1)).astype(np.float32)).cuda()
    s = torch.from_numpy(np.exp(rng.uniform(math.log(1e-3), math.log(1.0), (n, 3))).astype(np.float32)).cuda()
    g_o, g_s = torch.randn(n, 1, device="cuda"), torch.randn(n, 3, device="cuda")

    def hip_pair():
        SF.apply_filter_3d_forward(o, s, filt)
        SF.apply_filter_3d_backward(o, s, filt, g_o, g_s)

    def torch_pair():
        ol, sl = o.detach().requires_grad_(True), s.detach().requires_grad_(True)
        oe, se = torch_apply(ol, sl, filt)
        torch.autograd.backward([oe, se], [g_o, g_s])
        return oe.detach(), se.detach(), ol.grad, sl.grad

    oe, se = SF.apply_filter_3d_forward(o, s, filt)
    vo, vs = SF.apply_filter_3d_backward(o, s, filt, g_o, g_s)
    t_oe, t_se, t_vo, t_vs = torch_pair()
    worst = max(float(((a - b).abs() / b.abs().clamp_min(1e-30)).max()) for a, b in ((oe, t_oe), (se, t_se), (vo, t_vo)))
    hip = median_ms(hip_pair, args.warmup, args.runs)
    tor = median_ms(torch_pair, args.warmup, args.runs)
    lines.append(f"apply forward + backward: HIP {hip[0]:.3f} ms ({hip[1]:.3f} .. {hip[2]:.3f}), {n * 88 / hip[0] / 1e6:.0f} GB/s of the 88 bytes a row "
                 f"needs; torch + autograd {tor[0]:.3f} ms ({tor[1]:.3f} .. {tor[2]:.3f}); torch / HIP = {tor[0] / hip[0]:.1f}; "
                 f"worst relative difference of o_eff, se, vo {worst:.1e}")
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
