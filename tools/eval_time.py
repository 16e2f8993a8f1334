"""Times the evaluation head (gsr_eval_metrics, csrc/eval.hip) at 1920x1080 against the composed way of getting the same
numbers — torch slice, permute, sky composite, 8-bit rounding and u8 -> float of the target, then gsr_ssim_forward(train=0),
then torch means — for :rgb and for :rgbd with a sky frame, quantize=True and a byte target.  Median of `--runs` timed
runs after `--warmup` untimed ones, each between two device events on the current stream.  Not part of bench.py; run it
under a timeout of its own:

    timeout 300 python tools/eval_time.py [--out profiles/eval_head/eval_time.json]
"""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gsr_pkg
    pkg = gsr_pkg.load()
    EV, FS = pkg.evaluation, pkg.fused_ssim
    W, H = args.width, args.height
    r = np.random.default_rng(0)
    inv255 = torch.tensor(np.float32(1) / np.float32(255), device="cuda")
    target = torch.from_numpy(r.integers(0, 256, (H, W, 3)).astype(np.uint8)).cuda()
    sky = torch.from_numpy(r.uniform(0, 1, (H, W, 3)).astype(np.float32)).cuda()
    C1, C2 = float(np.float32(0.01) ** 2), float(np.float32(0.03) ** 2)
    result = dict(width=W, height=H, runs=args.runs, warmup=args.warmup, device=torch.cuda.get_device_name(0), modes={})
    for mode, C, use_sky in (("rgb", 3, False), ("rgbd+sky", 5, True)):
        frame = torch.from_numpy(r.uniform(-0.1, 1.1, (H, W, C)).astype(np.float32)).cuda()
        s = sky if use_sky else None
        out = torch.empty(4, device="cuda")
        scratch = torch.empty(EV.eval_scratch_bytes(W, H), dtype=torch.uint8, device="cuda")

        def fused():
            EV.eval_metrics(frame, target, s, True, out=out, scratch=scratch)

        composed_out = torch.empty(4, device="cuda")

        def composed():
            x = frame[..., :3]
            if use_sky:
                x = x + (1.0 - frame[..., 4])[..., None] * sky
            x = torch.floor(torch.clamp(x, 0.0, 1.0) * 255.0 + 0.5) * inv255
            x = x.permute(2, 0, 1).contiguous()[None]
            y = (target.to(torch.float32) * inv255).permute(2, 0, 1).contiguous()[None]
            with FS.exact_arithmetic():
                m = FS._fused_ssim(x, y, C1, C2, train=False)[0]
            d = x - y
            mse = (d.double() * d.double()).mean()
            composed_out[0] = m.double().mean().float()
            composed_out[1] = mse.float()
            composed_out[2] = (-10.0 * torch.log10(mse)).float()
            composed_out[3] = d.abs().double().mean().float()

        fused(); composed()
        torch.cuda.synchronize()
        a, b = out.cpu().numpy(), composed_out.cpu().numpy()
        f_ms, c_ms = median_ms(fused, args.warmup, args.runs), median_ms(composed, args.warmup, args.runs)
        result["modes"][mode] = dict(eval_metrics_ms=f_ms[0], eval_metrics_min_max_ms=f_ms[1:], composed_ms=c_ms[0],
                                     composed_min_max_ms=c_ms[1:], ratio_composed_over_fused=c_ms[0] / f_ms[0],
                                     eval_metrics_out=[float(v) for v in a], composed_out=[float(v) for v in b])
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
