"""Times the SH codebook fine-tuning step's additions (csrc/vq_grad.hip through gsr_vq_group / gsr_vq_codebook_grad and
sh_codebook) at n = 1 M rows of 45 floats, K = 4096 and 256:

  group       gsr_vq_group, once per set of indices (off the per-step path);
  grad        gsr_vq_codebook_grad with the codes as the nearest-code search assigned them, and with 90 % of the rows in ONE code;
              also straight out of an (N, 16, 3) gradient (row_stride 48, base + 3 floats);
  step        what fine-tuning adds to a training step: decode + grad + Adam of the code rows (SHCodebookFineTuner);
  beside them torch's index_add_ on the same device (float atomics: not deterministic), gsr_vq_accumulate (the library's other
              deterministic sum: 64-bit integer atomics), and the bytes floor (n·dim·4 + n·4 bytes at the STREAM triad's rate,
              gsr_stream_triad, measured in the same process).

Device milliseconds are between two device events on the current stream: the median of `--runs` timed runs after `--warmup`
untimed ones.  Not part of bench.py; run it under a timeout of its own:

    timeout 600 python tools/vq_grad_time.py [--out profiles/sh_codebook/finetune_times.txt]
"""
import argparse
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


def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--codes", type=int, nargs="+", default=[4096, 256])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gsr_pkg
    pkg = gsr_pkg.load()
    L, S = pkg._lib, pkg.sh_codebook
    lib = L.load()
    n, dim = args.n, 45
    gen = torch.Generator(device="cuda").manual_seed(21)
    x = torch.randn((n, dim), device="cuda", generator=gen) * torch.linspace(1.0, 0.05, dim, device="cuda")
    vshs = torch.randn((n, 16, 3), device="cuda", generator=gen) * 1e-3       # a gradient as gsr_backward lays it out
    g = vshs[:, 1:, :].contiguous()
    st = L.stream()

    n_tri = 128 * 1024 * 1024
    ta, tb, tc = (torch.ones(n_tri, device="cuda") for _ in range(3))
    t_tri = median_ms(lambda: L.check(lib.gsr_stream_triad(ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), n_tri, 0.5, st)), 2, 5)
    triad = 12.0 * n_tri / t_tri[0] / 1e6   # GB/s
    del ta, tb, tc
    floor_ms = (n * dim * 4 + n * 4) / triad / 1e6
    lines = [f"device: {torch.cuda.get_device_name(0)}; n = {n}, dim = {dim}; median (min .. max) of {args.runs} runs after "
             f"{args.warmup} warm-up runs, device events; STREAM triad {triad:.0f} GB/s: the bytes floor of one gradient pass "
             f"(n*dim*4 + n*4 = {(n * dim * 4 + n * 4) / 1e6:.0f} MB) is {floor_ms:.3f} ms"]
    print(lines[-1], flush=True)
    for K in args.codes:
        cb = x[(torch.arange(K, device="cuda") * n) // K].contiguous()
        idx = torch.zeros(n, dtype=torch.uint16, device="cuda")
        nb = int(lib.gsr_vq_scratch_bytes(n, K, dim))
        scr = torch.empty(nb, dtype=torch.uint8, device="cuda")
        L.check(lib.gsr_vq_assign(n, K, dim, L.ptr(x), L.ptr(cb), None, L.ptr(idx), None, None, L.ptr(scr), nb, st))
        idx64 = idx.view(torch.int16).to(torch.int64) & 0xFFFF
        hot64 = torch.where(torch.rand(n, device="cuda", generator=gen) < 0.9, torch.full_like(idx64, 7 % K), idx64)
        hot = hot64.to(torch.int16).view(torch.uint16)   # (K <= 32768 here)
        counts = torch.bincount(idx64, minlength=K)
        sh, sh_hot = S.SHCodebook(cb.clone(), idx, (n, 15, 3)), S.SHCodebook(cb.clone(), hot, (n, 15, 3))

        def group():
            sh.invalidate_groups()
            sh.groups()

        t_group = median_ms(group, 1, 3)
        sh_hot.groups()
        out = torch.empty((K, dim), device="cuda")
        t_even = median_ms(lambda: S.codebook_grad(g, sh, out=out), args.warmup, args.runs)
        t_hot = median_ms(lambda: S.codebook_grad(g, sh_hot, out=out), args.warmup, args.runs)
        t_view = median_ms(lambda: S.codebook_grad(vshs[:, 1:, :], sh, out=out), args.warmup, args.runs)
        tuner = S.SHCodebookFineTuner(sh)

        def step():
            tuner.features_rest()
            tuner.step(g)

        t_step = median_ms(step, args.warmup, args.runs)
        t_dec = median_ms(sh.decode, args.warmup, args.runs)
        g2 = g.view(n, dim)
        t_ia = median_ms(lambda: torch.zeros((K, dim), device="cuda").index_add_(0, idx64, g2), args.warmup, args.runs)
        t_ia_hot = median_ms(lambda: torch.zeros((K, dim), device="cuda").index_add_(0, hot64, g2), args.warmup, args.runs)
        sums, wsum = torch.zeros((K, dim), dtype=torch.int64, device="cuda"), torch.zeros(K, dtype=torch.int64, device="cuda")

        def accumulate(which):
            L.check(lib.gsr_vq_accumulate(n, K, dim, L.ptr(g2), L.ptr(which), None, L.ptr(sums), L.ptr(wsum), st))

        t_acc = median_ms(lambda: accumulate(idx), args.warmup, args.runs)
        t_acc_hot = median_ms(lambda: accumulate(hot), args.warmup, args.runs)
        # agreement with the atomics' sum, to the derived bound's order (not asserted: index_add_ has its own rounding)
        ref = torch.zeros((K, dim), device="cuda", dtype=torch.float64).index_add_(0, idx64, g2.double())
        S.codebook_grad(g, sh, out=out)
        mass = torch.zeros((K, dim), device="cuda", dtype=torch.float64).index_add_(0, idx64, g2.double().abs())
        err = float(((out.double() - ref).abs() / mass.clamp_min(1e-300)).max())
        lines.append(
            f"K = {K:5d} (rows per code: median {int(counts.median())}, max {int(counts.max())}): group {fmt(t_group)} once; "
            f"grad {fmt(t_even)} as assigned = {t_even[0] / floor_ms:.2f}x the bytes floor, {fmt(t_hot)} with 90 % in one code "
            f"= {t_hot[0] / t_even[0]:.2f}x the even case, {fmt(t_view)} out of the (N, 16, 3) gradient in place; decode {fmt(t_dec)}; "
            f"the fine-tune addition per step (decode + grad + Adam) {fmt(t_step)}.  Beside it: torch index_add_ {fmt(t_ia)} as "
            f"assigned, {fmt(t_ia_hot)} hot; gsr_vq_accumulate {fmt(t_acc)} as assigned, {fmt(t_acc_hot)} hot "
            f"= {t_acc[0] / t_even[0]:.1f}x / {t_acc_hot[0] / t_hot[0]:.1f}x the fixed-order sum.  max |sum - float64| / sum|g| = 2^{np.log2(max(err, 1e-300)):.1f}")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
