#!/usr/bin/env python3
"""Device times of the anchored depth supervision kernels at 1920x1080, for :rgbd (C = 5) and :rgbdn
(C = 8) frames: the forward (records + partials, header, loss pass, final pass), the backward (onto channels 3 and 4 of a
cotangent), and, as the baseline, the float32 torch formulation of tests/depth_torch.py run by torch on the same device,
forward + backward, in the same process.  HIP events around `--iters` launches each, after `--warmup` launches.  Prints one
JSON line with the per-launch milliseconds, the algorithmic bytes of each call and its rate against the STREAM triad
(gsr_stream_triad) measured in the same process.

The launches rotate over `--frames` frames (default 6; with their priors, cotangents and scratch 6 x (41..66 + 8 + 41..66
+ 33) MB > the 256 MiB Infinity Cache), so that a frame is not still on-die from the launch before: the rates are against
memory, as the triad's.  A `rocprofv3 --kernel-trace --stats` run of this tool gives the per-kernel split."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def big_frame(dt, np, W, H, C, seed):
    """The family of tests/depth_torch.make_frame at full size, with about 70 % valid priors and a 15 % sky block."""
    r = np.random.default_rng(seed)
    an = dt.DISPARITY
    rx = (np.arange(W) + 0.5 - 0.5 * W) / W
    ry = (np.arange(H) + 0.5 - 0.5 * H) / W
    e0 = 5.0 * 1.0630 / (1.0 - 0.2 * rx[None, :] + 0.3 * ry[:, None])
    e = e0 * (1.0 + 1e-2 * r.standard_normal((H, W)))
    t = (1.0 / (e0 + float(an.floor)) - float(an.b)) / float(an.a) + 2e-3 * r.standard_normal((H, W))
    alpha = r.uniform(0.05, 1.0, (H, W))
    alpha[r.random((H, W)) < 0.3] = 1.0
    sky_w, sky_h = int(0.5 * W), int(0.3 * H)     # 15 % of the frame
    t[:sky_h, W - sky_w:] = 0.005
    e[:sky_h, W - sky_w:W - sky_w // 2] = 3.0
    e[:sky_h, W - sky_w // 2:] = 500.0
    t[r.random((H, W)) < 0.3] = -1.0
    frame = np.zeros((H, W, C), np.float32)
    frame[..., :3] = 0.5
    frame[..., 3] = e * alpha
    frame[..., 4] = alpha
    return frame, t.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch-iters", type=int, default=20)
    a = ap.parse_args()

    import numpy as np
    import torch
    import gsr_pkg
    import depth_torch as dt
    pkg = gsr_pkg.load()
    DS, L = pkg.depth_supervision, pkg._lib
    W, H = a.width, a.height
    an = dt.DISPARITY
    anchor = DS.DepthAnchor(float(an.a), float(an.b), float(an.floor), float(an.disparity), float(an.p_far))
    k = [0]

    def timed(fn, iters=a.iters, warmup=a.warmup):
        for _ in range(warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    lib = L.load()
    n_tri = 128 * 1024 * 1024
    ta, tb, tc = (torch.ones(n_tri, device="cuda") for _ in range(3))
    cs = torch.cuda.current_stream().cuda_stream
    t_tri = timed(lambda: L.check(lib.gsr_stream_triad(ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), n_tri, 0.5, cs)))
    triad = 12.0 * n_tri / (t_tri * 1e-3) / 1e9
    del ta, tb, tc

    P = W * H
    res = dict(width=W, height=H, frames=a.frames, iters=a.iters, triad_gbs=round(triad, 1), device=torch.cuda.get_device_name(0),
               scratch_mb=round(DS.depth_loss_scratch_bytes(W, H) / 1e6, 2))
    for C in (5, 8):
        data = [big_frame(dt, np, W, H, C, seed=s) for s in range(a.frames)]
        frames = [torch.as_tensor(f).cuda() for f, _ in data]
        priors = [torch.as_tensor(p).cuda() for _, p in data]
        vps = [torch.zeros_like(f) for f in frames]
        scr = [torch.empty(DS.depth_loss_scratch_bytes(W, H), dtype=torch.uint8, device="cuda") for _ in frames]

        def fwd():
            i = k[0] = (k[0] + 1) % a.frames
            return DS.depth_loss(frames[i], priors[i], anchor, dt.QSTEP, 2.0, scratch=scr[i])

        def bwd():
            i = k[0] = (k[0] + 1) % a.frames
            DS.depth_loss_backward_(frames[i], priors[i], anchor, dt.QSTEP, vps[i], 2.0, scratch=scr[i])

        def both():
            i = k[0] = (k[0] + 1) % a.frames
            DS.depth_loss(frames[i], priors[i], anchor, dt.QSTEP, 2.0, scratch=scr[i])
            DS.depth_loss_backward_(frames[i], priors[i], anchor, dt.QSTEP, vps[i], 2.0, scratch=scr[i])

        t_fwd = timed(fwd)
        for i in range(a.frames):          # every scratch holds its frame's records before the backward is timed
            k[0] = i - 1
            fwd()
        t_bwd = timed(bwd)
        t_both = timed(both)
        loss, st = DS.depth_loss(frames[0], priors[0], anchor, dt.QSTEP, 2.0, stats=True, scratch=scr[0])
        maps = [dt.depth_target(an, p, dt.QSTEP) for _, p in data]
        valid = float(maps[0][2].mean())
        on_dev = [tuple(torch.as_tensor(m).cuda() for m in mp) for mp in maps]

        def torch_both():   # the baseline: the float32 formulation under torch autograd, forward + backward
            i = k[0] = (k[0] + 1) % a.frames
            x = frames[i].detach().requires_grad_(True)
            tg, hb, va, fa = on_dev[i]
            l, _ = dt.ssi_depth_loss(x[..., 3], x[..., 4], tg, hb, va, fa, an.floor, 1.0, info=False)
            (2.0 * l).backward()
            return l

        t_torch = timed(torch_both, iters=a.torch_iters, warmup=3)
        k[0] = -1                          # frame 0, as `loss`
        l_torch = 2.0 * float(torch_both().detach())
        # algorithmic bytes.  forward: every frame record (4·C) and the prior (4) read, the 16-byte record written, then read
        # once by the loss pass; backward: the records read, and on the pixels that receive something the frame record read
        # and the cotangent's record read and written (whole records: 128-byte lines move whole) — an upper bound
        mb = dict(fwd=P * (4 * C + 4 + 16 + 16) / 1e6, bwd=P * (16 + 3 * 4 * C) / 1e6)
        mb["both"] = mb["fwd"] + mb["bwd"]
        ms = dict(fwd=t_fwd, bwd=t_bwd, both=t_both)
        r = dict(valid_fraction=round(valid, 4), fwd_ms=round(t_fwd, 5), bwd_ms=round(t_bwd, 5), fwd_bwd_ms=round(t_both, 5),
                 torch_fwd_bwd_ms=round(t_torch, 4), speedup_vs_torch=round(t_torch / t_both, 1), loss=float(loss.item()),
                 torch_loss=l_torch, sigma=float(st[3].item()))
        for key in ("fwd", "bwd", "both"):
            gbs = mb[key] / ms[key]      # MB / ms = GB/s
            r[f"{key}_mb"] = round(mb[key], 2)
            r[f"{key}_gbs"] = round(gbs, 1)
            r[f"{key}_of_triad"] = round(gbs / triad, 3)
        res[f"C{C}"] = r
        del frames, priors, vps, scr, on_dev
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
