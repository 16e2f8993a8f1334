"""What the quantised model container costs in image quality on the trained-like synthetic scene (synthetic.make_trained_like,
the protocol of tools/vq_quality.py): the PSNR of the render of the unpacked container against the uncompressed render over the
eight views of synthetic.view_pose — each group quantised alone, the default spec, positions at 16 bits with one block against
blocks of 256, the default spec with the K = 4096 score-weighted SH codebook — the archive bytes plain and compressed, and
the dB that `--steps` fake-quantised steps (FakeQuantizer, the step without autograd) recover or lose, without the codebook at
two learning-rate scales and with it.  Asserted nowhere.

    timeout 900 python tools/quant_quality.py [--out profiles/quantised_model/quality.txt]
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
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gsr_pkg
    pkg = gsr_pkg.load()
    Q, S, CS, D, O, RZ, syn = (pkg.quantised_model, pkg.sh_codebook, pkg.contribution, pkg.densification, pkg.optim, pkg.rasterizer,
                               pkg.synthetic)
    W, H, n = args.width, args.height, args.n
    sc = syn.make_trained_like(n, W, H, 3)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    op = np.clip(sc.opacities.reshape(-1, 1).astype(np.float64), 1e-6, 1 - 1e-6)
    model = D.GaussianModel(d(sc.means), d(sc.shs[:, :1, :]), d(sc.shs[:, 1:, :]), d(np.log(sc.scales)), d(sc.rotations),
                            d(np.log(op / (1 - op))))
    cams = []
    for j in range(8):
        R, t = syn.view_pose(j, 8)
        cams.append(pkg.Camera(W, H, tuple(sc.focal), tuple(sc.principal), R, t))
    rast = RZ.GaussianRasterizer(W, H, mode="rgb", device="cuda:0")
    bg = (0.0, 0.0, 0.0)

    def acts(m):
        shs, oa, sa = RZ.prologue_forward(m.features_dc, m.features_rest, m.opacities, m.scales)
        return m.points, shs, oa, sa, m.rotations

    def render_all(m):
        a = acts(m)
        return [rast.forward_raw(*a, c, 3, bg, forward_only=True).clone() for c in cams]

    ref = render_all(model)

    def psnr(m):
        mse = [float(((a - b) ** 2).mean()) for a, b in zip(render_all(m), ref)]
        p = [10.0 * math.log10(1.0 / v) if v > 0 else float("inf") for v in mse]
        return f"{np.mean(p):6.2f} dB (min {min(p):.2f})", float(np.mean(p))

    lines = [f"device: {torch.cuda.get_device_name(0)}; trained-like scene, {n} Gaussians at SH degree 3, 8 views of {W} x {H}; PSNR of the "
             f"unpacked container's render against the uncompressed render, mean of the views (min); the PLY rows are {236 * n} bytes"]
    # each group alone: the others at 16 bits in blocks of 64 would still add their own error, so the others are copied unquantised
    default = Q.QuantSpec()
    whole = Q.pack_model(model, None, default)
    sorted_model = D.GaussianModel(*[getattr(model, k)[whole.permutation.long()].contiguous() for k in D.PARAMS])
    un = whole.unpack()
    for g in Q.GROUPS:
        parts = {k: getattr(sorted_model, k) for k in D.PARAMS}
        parts[g] = getattr(un, g)
        bits, br = getattr(default, g)
        lines.append(f"{g:13s} alone ({bits:2d} bits, block_rows {br:3d}): {psnr(D.GaussianModel(**parts))[0]}")

    def sizes(qm):
        out = []
        with tempfile.TemporaryDirectory() as tmp:
            for comp in (False, True):
                p = os.path.join(tmp, f"m{int(comp)}.npz")
                qm.save(p, compressed=comp)
                out.append(os.path.getsize(p))
        return out

    plain, comp = sizes(whole)
    base = psnr(un)
    lines.append(f"default spec, features_rest at 8 bits: {base[0]}; {whole.nbytes} bytes of arrays ({whole.nbytes / n:.1f} per Gaussian), archive "
                 f"{plain} bytes plain, {comp} compressed ({236 * n / comp:.1f}x smaller than the PLY rows)")
    for br in (0, 256):
        spec = Q.QuantSpec(points=(16, br))
        parts = {k: getattr(sorted_model, k) for k in D.PARAMS}
        parts["points"] = Q.pack_model(sorted_model, None, spec, order=None).unpack().points
        lines.append(f"positions at 16 bits, block_rows {br:3d}, the other groups unquantised: {psnr(D.GaussianModel(**parts))[0]}")
    scores = CS.score_views(rast, acts(model), cams, 3)
    sh = S.fit_sh_codebook(model.features_rest, 4096, iters=10, weights=S.weights_from_scores(scores.weight_sum))
    with_sh = Q.pack_model(model, sh, default)
    plain, comp = sizes(with_sh)
    lines.append(f"default spec with the K = 4096 score-weighted SH codebook: {psnr(with_sh.unpack())[0]}; {with_sh.nbytes} bytes of arrays "
                 f"({(with_sh.nbytes - sh.codebook.numel() * 4) / n:.2f} per Gaussian + the codebook), archive {plain} bytes plain, {comp} compressed "
                 f"({236 * n / comp:.1f}x smaller than the PLY rows)")
    print("\n".join(lines), flush=True)

    # quantisation-aware fine-tuning, the step without autograd, one view per step: the default spec without a codebook at a
    # tenth and at a hundredth of the training rates (started from the model that IS the target, there is only the quantisation
    # error to remove), and with the codebook, whose 34 dB are there to recover (SHCodebookFineTuner supplies features_rest)
    def qat(scale, with_codebook):
        m = D.GaussianModel(*[getattr(sorted_model, k).clone() for k in D.PARAMS])
        lrs = dict(points=1.6e-4, features_dc=2.5e-3, features_rest=2.5e-3 / 20, opacities=2.5e-2, scales=5e-3, rotations=1e-3)
        names = [g for g in Q.GROUPS if not (with_codebook and g == "features_rest")]
        raw = [getattr(m, g) for g in names]
        opts = [O.Adam(t, scale * lrs[g], eps=1e-15) for g, t in zip(names, raw)]
        Q.positive_w_rotations_(m.rotations, opts[-1])
        tuner = None
        if with_codebook:
            tuner = S.SHCodebookFineTuner(S.SHCodebook(with_sh.sh.codebook.clone(), with_sh.sh.indices, with_sh.sh.shape))
        fq = Q.FakeQuantizer(default)
        for step in range(args.steps):
            if step % 100 == 0:
                fq.refresh(m)
            with torch.no_grad():
                pts, dc, rest, opq, scq, rot = fq.apply(m, sh_codebook=tuner)
            shs, oa, sa = RZ.prologue_forward(dc, rest, opq, scq)
            cam = cams[step % 8]
            img = rast.forward_raw(pts, shs, oa, sa, rot, cam, 3, bg)
            vpix = (torch.sign(img - ref[step % 8]) / img.numel()).contiguous()
            vm, vshs, vo, vsc, vr = rast.backward_raw(vpix, pts, shs, oa, sa, rot, cam, 3, bg)[:5]
            vdc, vrest, vo_raw, vs_raw = RZ.prologue_backward(oa, sa, vshs, vo.view(-1, 1), vsc, scale_dims=3)
            if with_codebook:
                tuner.step(vshs[:, 1:, :])
                O.step_all(opts, raw, [vm, vdc, vo_raw, vs_raw, vr])
            else:
                O.step_all(opts, raw, [vm, vdc, vrest, vo_raw, vs_raw, vr])
        return psnr(Q.pack_model(m, tuner.sh if with_codebook else None, default, order=None).unpack())

    if args.steps > 0:
        with_sh_base = psnr(with_sh.unpack())
        for scale, cb, start in ((0.1, False, base), (0.01, False, base), (0.1, True, with_sh_base)):
            tuned = qat(scale, cb)
            lines.append(f"{'default spec + codebook' if cb else 'default spec'} after {args.steps} fake-quantised steps (L1, one view per step, "
                         f"{scale:g} x the training rates, ranges every 100 steps{', code rows through SHCodebookFineTuner' if cb else ''}): "
                         f"{tuned[0]}, {tuned[1] - start[1]:+.2f} dB against the container packed without them")
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
