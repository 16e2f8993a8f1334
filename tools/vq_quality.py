"""What SH codebook compression costs in image quality on the trained-like synthetic scene (synthetic.make_trained_like): the
PSNR of the render with decoded features_rest against the uncompressed render, over the eight views of synthetic.view_pose,
for K = 256 / 4096, unweighted and weighted by the views' contribution scores (weights_from_scores), and the archive sizes.
The scene's features_rest is independent noise per coefficient — the hardest case for a codebook; a trained capture has
structure that this scene lacks.  Numbers for DESIGN.md §23, asserted nowhere.

    timeout 600 python tools/vq_quality.py [--out profiles/sh_codebook/quality.txt]
"""
import argparse
import math
import os
import sys
import tempfile

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

    def render_all(shs_t):
        return [rast.forward_raw(means, shs_t, opac, scales, rots, c, 3, (0.0, 0.0, 0.0), forward_only=True).clone() for c in cams]

    ref = render_all(shs)
    scores = CS.score_views(rast, (means, shs, opac, scales, rots), cams, 3)
    wq = S.weights_from_scores(scores.weight_sum)
    rest = shs[:, 1:, :].contiguous()
    lines = [f"device: {torch.cuda.get_device_name(0)}; trained-like scene, {n} Gaussians, 8 views of {W} x {H}; features_rest "
             f"{rest.numel() * 4} bytes uncompressed; {args.iters} Lloyd iterations; weights: {int((wq == 1).sum())} rows at 1, mean {float(wq.float().mean()):.1f}"]
    dc_only = torch.cat([shs[:, :1, :], torch.zeros_like(rest)], 1).contiguous()
    cases = [("features_rest dropped (zeros)", dc_only, 0, None)]
    for K in args.codes:
        for name, w in (("unweighted", None), ("score-weighted", wq)):
            cbk = S.fit_sh_codebook(rest, K, iters=args.iters, weights=w)
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "c.npz")
                cbk.save(path)
                size = os.path.getsize(path)
            h = cbk.history.view(torch.int32)
            cases.append((f"K = {K:4d} {name:14s} (last iteration: {int(h[-1, 0])} rows changed, {int(h[-1, 1])} empty codes)",
                          torch.cat([shs[:, :1, :], cbk.decode()], 1).contiguous(), size, cbk))
    for name, shs_t, size, cbk in cases:
        imgs = render_all(shs_t)
        mse = [float(((a - b) ** 2).mean()) for a, b in zip(imgs, ref)]
        psnr = [10.0 * math.log10(1.0 / m) if m > 0 else float("inf") for m in mse]
        extra = f"; archive {size} bytes ({cbk.nbytes} of arrays), {rest.numel() * 4 / size:.1f}x smaller" if cbk is not None else ""
        lines.append(f"{name}: PSNR against the uncompressed render, mean of 8 views {np.mean(psnr):.2f} dB (min {min(psnr):.2f}){extra}")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
