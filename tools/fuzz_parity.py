#!/usr/bin/env python3
"""On the GPU box: the randomised HIP-vs-oracle sweep of tests/test_gpu_parity.py over MANY more seeds than the test suite
runs (cases 12 .. 12+N: modes, SH degrees, ragged resolutions, views, footprint sizes, opacity ranges, both list modes;
forward, every gradient).  Prints the failing cases with their assertion; exit code = number of failures.

  python tools/fuzz_parity.py [N = 300] [first case = 12]
  python tools/fuzz_parity.py deep [N = 60] [first case = 0]     dense scenes on 1..9 tiles: lists of 300 .. 40 000 instances
      per tile (the 1024 / 4096 / 8192 sort tiers, the tier launches of both compositing kernels, bins that overflow and
      finish in compact mode), all three modes, forward + every gradient
  python tools/fuzz_parity.py edge [N = 200] [first case = 0]    hostile inputs: fx != fy, arbitrary camera rotations and
      translations, near / far planes that cut the scene, opacities of exactly 0 / 1 / above the 0.99 clamp, scales from
      sub-pixel (culled by radius) to screen-filling, negative, 27:1 anisotropic, means behind the camera / on the planes / far
      off-screen, SH values that clamp; pose gradients from device-resident poses
  python tools/fuzz_parity.py ssim [N = 300] [first case = 0]    fused SSIM forward / backward (bit-exact) on random
      (B, C, H, W) from 1 x 1 x 1 x 1 up, and the L1 + DSSIM loss head on ragged resolutions
  python tools/fuzz_parity.py arbitrate sweep|edge|deep CASE ... failing cases of a campaign against the float64 autograd model:
      which of the suite's criteria — (a) tolerance, (b) conditioning, (c) a boundary pair — explains each gradient tensor
  python tools/fuzz_parity.py trainer [N = 40] [first case = 0]  the bit-exact trainer-tail / compaction tests of
      tests/test_gpu_trainer.py and the densification test of tests/test_gpu_densify.py at random sizes, SH degrees,
      isotropic / anisotropic scales and render modes (their data seeds are fixed inside the tests)
"""
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gsr_pkg  # noqa: E402

pkg = gsr_pkg.load()
from oracle import oracle as orc  # noqa: E402
import test_gpu_parity as T  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
from hip_helpers import HipRun, pose_distances, pose_grad_f64, pose_ok  # noqa: E402


import fuzz_scenes  # noqa: E402  (tests/fuzz_scenes.py: the seeded scene families, shared with the test suite)


# GSR_FUZZ_BINS_KEYS=K: every handle gets a bins budget of K keys per tile (gsr_config.bins_budget_bytes) and renders its view
# twice — K >= 1024 with lists beyond it: the second view keeps its bins and scatters the overflowing lists again
# (gsr_stats.compact_binning == 2); K < 64: compact mode.  The counts of each binning mode are printed at the end.
BINS_KEYS = int(os.environ.get("GSR_FUZZ_BINS_KEYS", "0"))
# GSR_FUZZ_GRAD_PRECISION=accurate|fp32_reference: every handle is created with that gsr_config.grad_precision (round 6)
GRAD_PRECISION = os.environ.get("GSR_FUZZ_GRAD_PRECISION") or None
BINNING_SEEN = {0: 0, 1: 0, 2: 0}


def _budget(cam):
    T_ = ((cam.width + 15) // 16) * ((cam.height + 15) // 16)
    return (T_ + 1) * 8 * BINS_KEYS if BINS_KEYS else 0


def _fwd(run):
    if BINS_KEYS:
        run.forward()
    img = run.forward()
    BINNING_SEEN[int(run.rast.stats.compact_binning)] += 1
    return img


def _scene_case(fs):
    """forward (every field, both list modes) + every gradient of one fuzz scene against the oracle."""
    st = orc.forward(fs.means, fs.shs, fs.opac, fs.scales, fs.rots, fs.cam, fs.deg, background=fs.bg, mode=fs.mode)
    run = HipRun(pkg, fs.means, fs.shs, fs.opac, fs.scales, fs.rots, fs.cam, fs.deg, fs.bg, fs.mode, pose_dev=fs.pose,
                 bins_budget_bytes=_budget(fs.cam), grad_precision=GRAD_PRECISION)
    img = _fwd(run).clone()
    T._compare_forward(st, run, img, fs.opac)
    vp = fs.cotangent()
    g = orc.backward(st, vp, fs.means, fs.shs, fs.opac, fs.scales, fs.rots, fs.cam, fs.deg, background=fs.bg,
                     **({"pose_grad": True} if fs.pose else {}))
    ok = st.n_rendered > 0 and np.linalg.norm(g.vmeans) > 0
    if ok:
        vR, vt = T._compare_backward(g, run.backward(vp), st.radii > 0)
        if fs.pose:
            assert T.rel_l2(vR.reshape(-1), g.vR) <= 1e-4 and T.rel_l2(vt, g.vt) <= 1e-4
    cul = HipRun(pkg, fs.means, fs.shs, fs.opac, fs.scales, fs.rots, fs.cam, fs.deg, fs.bg, fs.mode, exact_tile_cull=True,
                 bins_budget_bytes=_budget(fs.cam))
    assert torch.equal(_fwd(cul), img)
    if ok:
        T._compare_backward(g, cul.backward(vp), st.radii > 0)
    return st


def deep_case(case):
    st = _scene_case(fuzz_scenes.deep_scene(pkg, case))
    return int((st.ranges[:, 1] - st.ranges[:, 0]).max())


def edge_case(case):
    st = _scene_case(fuzz_scenes.edge_scene(pkg, case))
    return int((st.radii > 0).sum())


def ssim_case(case):
    rng = np.random.default_rng(33000 + case)
    from hip_helpers import dev
    shape = (int(rng.integers(1, 3)), int(rng.integers(1, 4)), int(rng.integers(1, 160)), int(rng.integers(1, 160)))
    scale = float(rng.choice([1.0, 1e-3, 50.0]))
    x = (rng.uniform(size=shape) * scale).astype(np.float32)
    y = (rng.uniform(size=shape) * scale).astype(np.float32)
    if case % 7 == 0:
        y = x.copy()
    m, d0, d1, d2 = orc.ssim_forward(x, y, train=True)
    Fs = pkg.fused_ssim
    with Fs.exact_arithmetic():  # the bit-exact twin of ssim.hip (the default build is compared at tolerance by the loss head below)
        hm, h0, h1, h2 = Fs._fused_ssim(dev(x), dev(y), train=True)
        for a, b in ((hm, m), (h0, d0), (h1, d1), (h2, d2)):
            assert np.array_equal(a.cpu().numpy(), b, equal_nan=True), ("ssim fwd", shape)
        dl = rng.standard_normal(shape).astype(np.float32)
        g = orc.ssim_backward(x, y, dl, d0, d1, d2)
        hg = Fs.fused_ssim_bwd(dev(x), dev(y), dev(dl), h0, h1, h2)
        assert np.array_equal(hg.cpu().numpy(), g, equal_nan=True), ("ssim bwd", shape)
    # loss head on a ragged image
    W, H = int(rng.integers(16, 200)), int(rng.integers(16, 150))
    mode = ["rgb", "rgbd"][case % 2]
    C = 3 if mode == "rgb" else 5
    img = rng.uniform(size=(H, W, C)).astype(np.float32)
    tgt = pkg.synthetic.make_target(W, H, case)
    loss, vp = orc.loss_head(img, tgt)
    rast = pkg.rasterizer.GaussianRasterizer(W, H, mode=mode)
    hl, hv = Fs.l1_ssim_loss(rast, dev(img), dev(tgt))
    torch.cuda.synchronize()
    assert abs(float(hl) - float(loss)) <= 1e-5 * max(1.0, abs(float(loss))), ("loss", W, H)
    assert T.rel_l2(hv.cpu().numpy(), vp) <= 1e-5, ("loss pullback", W, H)


def trainer_case(case):
    import test_gpu_trainer as TT
    import test_gpu_densify as TD
    rng = np.random.default_rng(21000 + case)
    n = int(rng.choice([1, 2, 63, 64, 65, 255, 256, 257, int(rng.integers(300, 6000))]))
    kr = int(rng.choice([0, 3, 8, 15]))
    iso = bool(rng.integers(0, 2))
    TT.test_prologue_forward_vs_oracle(pkg, orc, n, kr, iso)
    TT.test_prologue_backward_vs_oracle_bit_exact(pkg, orc, n, kr, iso)
    TT.test_mask_findall_vs_oracle(pkg, orc, int(rng.integers(1, 300000)), float(rng.choice([0.0, 1.0, rng.uniform()])))
    TT.test_fused_trainer_tail_equals_the_three_kernels_and_the_oracle(pkg, orc, kr, iso)
    max_deg = int(rng.integers(0, 4))
    deg = int(rng.integers(0, max_deg + 1))
    TT.test_backward_with_the_tail_in_its_epilogue_equals_backward_then_tail(
        pkg, int(rng.integers(1, 2500)), deg, max_deg, iso, ["rgb", "rgbd", "rgbdn"][case % 3], bool(case % 3 and case % 2))
    if case % 4 == 0:
        TD.test_densify_and_prune_matches_oracle(pkg, 1 if iso else 3, kr, int(rng.choice([0, 20])))


def _pose_verdict(fs, st, boundary_pair=False):
    """∇R / ∇t of a scene with device-resident poses (fuzz_parity.py:77): oracle (fp32), HIP and the float64 autograd model.  A pose
    gradient is ONE sum over every Gaussian of the view — signed terms that largely cancel — so its relative error is the
    per-Gaussian errors amplified by Σ|terms| / |Σ terms|.  Explained when HIP meets 1e-4 against float64, or is no further from
    float64 than the fp32 oracle is (x 4 + 1e-4, as criterion (b)).  boundary_pair: a per-Gaussian tensor of the scene got verdict (b) or
    (c) — needles beyond 10 : 1 whose ∇means carries the conditioning error (edge 8498: ONE 90 : 1 needle of radius 100 px, ∇means
    3e-3 off in HIP and 2e-4 in the oracle, whose double accumulators feed its fp32 chain cleaner sums), or a (pixel, splat) blend
    test decided differently — and the pose gradient, a sum over the same per-Gaussian terms, carries the same error: reported,
    not asserted."""
    vp = fs.cotangent()
    g = orc.backward(st, vp, fs.means, fs.shs, fs.opac, fs.scales, fs.rots, fs.cam, fs.deg, background=fs.bg, pose_grad=True)
    run = HipRun(pkg, fs.means, fs.shs, fs.opac, fs.scales, fs.rots, fs.cam, fs.deg, fs.bg, fs.mode, pose_dev=True, grad_precision=GRAD_PRECISION)
    run.forward()
    out = run.backward(vp)
    hR, ht = out[5].cpu().numpy().reshape(-1), out[6].cpu().numpy().reshape(-1)
    fR, ft = pose_grad_f64(fs.means, fs.shs, fs.opac, fs.scales, fs.rots, fs.cam, fs.deg, fs.bg, fs.mode, st, vp)
    res = {}
    for nm, h, o, f in (("vR", hR, g.vR, fR), ("vt", ht, g.vt, ft)):
        e_ho, e_o, e_h = pose_distances(h, o, f)
        ok = pose_ok(e_ho, e_o, e_h)
        assert ok or boundary_pair, f"{nm}: HIP-oracle {e_ho:.2e}, oracle-f64 {e_o:.2e}, HIP-f64 {e_h:.2e}"
        res[nm] = (("" if ok else "inherits the scene's (b) / (c) verdict: ") + f"HIP-oracle {e_ho:.1e}, oracle-f64 {e_o:.1e}, HIP-f64 {e_h:.1e}")
    return res


def arbitrate_cases(family, cases):
    """`python tools/fuzz_parity.py arbitrate sweep|edge CASE ...`: the float64 arbitration of the suite
    (tests/test_gpu_fuzz_regressions.py: criteria (a) / (b) / (c)) on failing cases of a campaign — oracle, HIP kernels and the
    float64 autograd model on the same scene; prints the verdict per gradient tensor, or the assertion that none applies."""
    import test_gpu_fuzz_regressions as R
    build = {"sweep": fuzz_scenes.sweep_scene, "edge": fuzz_scenes.edge_scene, "deep": fuzz_scenes.deep_scene}[family]
    bad = 0
    for case in cases:
        fs = build(pkg, case)
        try:
            res, st = R.three_way(pkg, orc, fs, grad_precision=GRAD_PRECISION)
            verdict = R.arbitrate(res, st, fs)
            if fs.pose:
                # (a fresh scene object: the campaign's cotangent is its rng's FIRST draw)
                verdict.update(_pose_verdict(build(pkg, case), st, any(str(v).startswith(("(b)", "(c)")) for v in verdict.values())))
            print(family, case, verdict, flush=True)
        except AssertionError as e:
            bad += 1
            print(family, case, "NOT EXPLAINED:", str(e)[:400], flush=True)
    print(f"{len(cases) - bad} / {len(cases)} failing {family} cases explained by criteria (a) / (b) / (c)")
    sys.exit(min(bad, 100))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "arbitrate":
        return arbitrate_cases(sys.argv[2], [int(a) for a in sys.argv[3:]])
    deep = len(sys.argv) > 1 and sys.argv[1] == "deep"
    edge = len(sys.argv) > 1 and sys.argv[1] == "edge"
    ssim = len(sys.argv) > 1 and sys.argv[1] == "ssim"
    trainer = len(sys.argv) > 1 and sys.argv[1] == "trainer"
    if deep or edge or ssim or trainer:
        sys.argv.pop(1)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else (60 if deep else 200 if edge else 40 if trainer else 300)
    first = int(sys.argv[2]) if len(sys.argv) > 2 else (0 if deep or edge or ssim or trainer else 12)
    bad = []
    longest = []
    for case in range(first, first + n):
        try:
            if deep:
                longest.append(deep_case(case))
            elif edge:
                edge_case(case)
            elif ssim:
                ssim_case(case)
            elif trainer:
                trainer_case(case)
            else:
                T.test_randomised_sweep_vs_oracle(pkg, orc, case)
        except Exception as e:  # noqa: BLE001
            tb = traceback.extract_tb(e.__traceback__)
            bad.append((case, f"{type(e).__name__}: {str(e)[:200]}", f"{tb[-1].filename.split('/')[-1]}:{tb[-1].lineno}"))
            print("FAIL case", case, bad[-1][1], "at", bad[-1][2], flush=True)
    if deep and longest:
        q = np.percentile(longest, [0, 25, 50, 75, 100]).astype(int)
        print("deepest tile list per case: min / quartiles / max =", list(q), " cases over 1024 / 4096 / 8192:",
              int((np.array(longest) > 1024).sum()), int((np.array(longest) > 4096).sum()), int((np.array(longest) > 8192).sum()))
    if deep or edge:
        print("binning mode of the checked views (gsr_stats.compact_binning 0 bins / 1 compact / 2 bins + overflow lists):", BINNING_SEEN)
    print(f"{n - len(bad)} / {n} {'deep ' if deep else 'edge ' if edge else 'ssim ' if ssim else 'trainer ' if trainer else ''}cases passed (cases {first}..{first + n - 1})")
    sys.exit(min(len(bad), 100))


if __name__ == "__main__":
    main()
