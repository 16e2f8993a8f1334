"""What fine-tuning through the SH codebook recovers, on §23's quality protocol: the trained-like synthetic scene
(synthetic.make_trained_like), eight views of synthetic.view_pose, a score-weighted codebook of K = 256 / 4096 codes.  The
targets are the uncompressed model's renders; `--steps` training steps update the K code rows alone (the indices and every
other parameter fixed): forward, the L1 + SSIM loss head, backward_raw, SHCodebookFineTuner.step on `vshs[:, 1:, :]` in place.
Reports the PSNR against the uncompressed render over the eight views before and after, and the steps per second of that loop.
Numbers for DESIGN.md §24, asserted nowhere.

    timeout 900 python tools/vq_finetune_quality.py [--out profiles/sh_codebook/finetune_quality.txt]
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=400)
    ap.add_argument("--codes", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--lr", type=float, default=25e-4 / 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gsr_pkg
    pkg = gsr_pkg.load()
    S, CS, syn = pkg.sh_codebook, pkg.contribution, pkg.synthetic
    W, H, n = args.width, args.height, args.n
    sc = syn.make_trained_like(n, W, H, 3)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
    means, shs, opac, scales, rots = d(sc.means), d(sc.shs), d(sc.opacities.reshape(-1, 1)), d(sc.scales), d(sc.rotations)
    cams = []
    for j in range(8):
        R, t = syn.view_pose(j, 8)
        cams.append(pkg.Camera(W, H, tuple(sc.focal), tuple(sc.principal), R, t))
    rast = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgb", device="cuda:0")
    bg = (0.0, 0.0, 0.0)

    def render_all(shs_t):
        return [rast.forward_raw(means, shs_t, opac, scales, rots, c, 3, bg, forward_only=True).clone() for c in cams]

    def psnr(shs_t, ref):
        mse = [float(((a - b) ** 2).mean()) for a, b in zip(render_all(shs_t), ref)]
        p = [10.0 * math.log10(1.0 / m) if m > 0 else float("inf") for m in mse]
        return float(np.mean(p)), float(min(p))

    ref = render_all(shs)
    targets = [r.permute(2, 0, 1).contiguous() for r in ref]
    scores = CS.score_views(rast, (means, shs, opac, scales, rots), cams, 3)
    wq = S.weights_from_scores(scores.weight_sum)
    rest = shs[:, 1:, :].contiguous()
    lines = [f"device: {torch.cuda.get_device_name(0)}; trained-like scene, {n} Gaussians, 8 views of {W} x {H}; score-weighted "
             f"codebooks of {args.iters} Lloyd iterations; {args.steps} steps of the code rows alone, lr {args.lr:g}, eps 1e-15, "
             f"loss 0.8 L1 + 0.2 (1 - SSIM) against the uncompressed renders"]
    for K in args.codes:
        sh = S.fit_sh_codebook(rest, K, iters=args.iters, weights=wq)
        tuner = S.SHCodebookFineTuner(sh, lr=args.lr)
        work = shs.clone()
        work[:, 1:, :] = tuner.features_rest()
        before = psnr(work, ref)
        first = last = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for step in range(args.steps):
            v = step % 8
            work[:, 1:, :] = tuner.features_rest()
            img = rast.forward_raw(means, work, opac, scales, rots, cams[v], 3, bg)
            loss, vpix = pkg.fused_ssim.l1_ssim_loss(rast, img, targets[v])
            vshs = rast.backward_raw(vpix, means, work, opac, scales, rots, cams[v], 3, bg, color_cotangent=True)[1]
            tuner.step(vshs[:, 1:, :])
            if step < 8:
                first = loss.clone() if first is None else first + loss
            if step >= args.steps - 8:
                last = loss.clone() if last is None else last + loss
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        work[:, 1:, :] = tuner.features_rest()
        after = psnr(work, ref)
        lines.append(f"K = {K:4d} score-weighted: PSNR against the uncompressed render, mean of 8 views {before[0]:.2f} dB (min {before[1]:.2f}) "
                     f"before, {after[0]:.2f} dB (min {after[1]:.2f}) after {args.steps} steps; loss, mean of 8 views, {float(first) / 8:.5f} "
                     f"in the first pass, {float(last) / 8:.5f} in the last; {args.steps / dt:.0f} steps/s ({1e3 * dt / args.steps:.3f} ms per step, "
                     f"host clock around the whole loop)")
        print(lines[-1], flush=True)
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
