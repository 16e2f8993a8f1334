#!/usr/bin/env python3
"""Device times of the sky-dome kernels at 1920x1080, for :rgbd (C = 5) and :rgbdn (C = 8) frames: the
forward (composite into a second frame + the sky-mask loss: one streaming pass and the one-workgroup final pass), the
in-place composite without a mask, the backward (vsky + the add onto channel 4 of a cotangent), and, as the baseline, the
float32 torch composition of tests/sky_torch.py run by torch on the same device, forward + backward, in the same process.
HIP events around `--iters` launches each, after `--warmup` launches.  Prints one JSON line with the per-launch
milliseconds, the algorithmic bytes of each call and its rate against the STREAM triad (gsr_stream_triad) measured in the
same process.

The launches rotate over `--frames` frame sets (default 6; a set is frame + sky + mask + out + cotangent + vsky, 180 to
260 MB, so six of them are several times the 256 MiB Infinity Cache): a frame is not still on-die from the launch before,
and the rates are against memory, as the triad's.  A `rocprofv3 --kernel-trace --stats` run of this tool gives the
per-kernel split."""
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
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch-iters", type=int, default=20)
    a = ap.parse_args()

    import torch
    import gsr_pkg
    import sky_torch as st
    pkg = gsr_pkg.load()
    SD, L = pkg.sky_dome, pkg._lib
    W, H, LW = a.width, a.height, 0.7
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
               scratch_kb=round(SD.sky_scratch_bytes(W, H) / 1e3, 1))
    for C in (5, 8):
        data = [st.make_case(W, H, C, seed=s) for s in range(a.frames)]
        frames = [torch.as_tensor(f).cuda() for f, _, _, _ in data]
        skies = [torch.as_tensor(s).cuda() for _, s, _, _ in data]
        masks = [torch.as_tensor(m["fractional"]).cuda() for _, _, m, _ in data]
        cots = [torch.as_tensor(g).cuda() for _, _, _, g in data]
        del data
        outs = [torch.empty_like(f) for f in frames]
        vps = [g.clone() for g in cots]
        vskies = [torch.empty_like(s) for s in skies]
        scr = [torch.empty(SD.sky_scratch_bytes(W, H), dtype=torch.uint8, device="cuda") for _ in frames]

        def fwd():
            i = k[0] = (k[0] + 1) % a.frames
            return SD.composite_sky(frames[i], skies[i], outs[i], masks[i], LW, scratch=scr[i])

        def fwd_in_place():     # the frame keeps changing: only the time is used
            i = k[0] = (k[0] + 1) % a.frames
            SD.composite_sky(outs[i], skies[i], outs[i])

        def bwd():
            i = k[0] = (k[0] + 1) % a.frames
            SD.sky_composite_backward_(frames[i], skies[i], vps[i], masks[i], LW, vsky=vskies[i], scratch=scr[i])

        def both():
            i = k[0] = (k[0] + 1) % a.frames
            SD.composite_sky(frames[i], skies[i], outs[i], masks[i], LW, scratch=scr[i])
            SD.sky_composite_backward_(frames[i], skies[i], vps[i], masks[i], LW, vsky=vskies[i], scratch=scr[i])

        t_fwd = timed(fwd)              # every scratch holds its frame's 1 / max(Σw, 1) before the backward is timed
        t_bwd = timed(bwd)
        t_both = timed(both)
        t_inp = timed(fwd_in_place)
        k[0] = -1
        _, loss = fwd()

        def torch_both():   # the baseline: the float32 composition under torch autograd, forward + backward
            i = k[0] = (k[0] + 1) % a.frames
            x, s = frames[i].detach().requires_grad_(True), skies[i].detach().requires_grad_(True)
            comp, l, _ = st.composite_and_loss(x, s, masks[i], LW)
            ((comp * cots[i][..., :3]).sum() + l).backward()
            return l

        t_torch = timed(torch_both, iters=a.torch_iters, warmup=3)
        k[0] = -1
        l_torch = float(torch_both().detach())
        # algorithmic bytes.  forward: the frame record (4·C), the sky record (12) and the mask (4) read, the frame record
        # written; in place without a mask: the record and the sky read, the record written back (whole 128-byte lines move
        # whole); backward: the frame record (for alpha), the sky record and the mask read, the cotangent's record read and
        # written, the sky cotangent (12) written
        mb = dict(fwd=P * (8 * C + 16) / 1e6, in_place=P * (8 * C + 12) / 1e6, bwd=P * (12 * C + 28) / 1e6)
        mb["both"] = mb["fwd"] + mb["bwd"]
        ms = dict(fwd=t_fwd, in_place=t_inp, bwd=t_bwd, both=t_both)
        r = dict(fwd_ms=round(t_fwd, 5), in_place_ms=round(t_inp, 5), bwd_ms=round(t_bwd, 5), fwd_bwd_ms=round(t_both, 5),
                 torch_fwd_bwd_ms=round(t_torch, 4), speedup_vs_torch=round(t_torch / t_both, 1), loss=float(loss.item()),
                 torch_loss=l_torch)
        for key in ("fwd", "in_place", "bwd", "both"):
            gbs = mb[key] / ms[key]      # MB / ms = GB/s
            r[f"{key}_mb"] = round(mb[key], 2)
            r[f"{key}_gbs"] = round(gbs, 1)
            r[f"{key}_of_triad"] = round(gbs / triad, 3)
        res[f"C{C}"] = r
        del frames, skies, masks, cots, outs, vps, vskies, scr
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
