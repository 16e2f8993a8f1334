"""Times one Lloyd iteration of the SH codebook k-means (csrc/vq.hip through gsr_vq_*), each kernel group on its own, beside a
torch formulation on the same device (chunked cdist + argmin + index_add_) — the only baseline there is:

  assign      n x K x dim at 1 M x 4096 x 45 and 1 M x 256 x 45 (prep + search), against the f32 MFMA peak (2·n·K·dim flop);
  accumulate  on the assignment the search found (near uniform) and on one with 90 % of the rows in ONE code;
  update      K x dim.

Device milliseconds are between two device events on the current stream: the median of `--runs` timed runs after `--warmup`
untimed ones.  Not part of bench.py; run it under a timeout of its own:

    timeout 600 python tools/vq_time.py [--out profiles/sh_codebook/times.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_TF = 155.0   # measured f32-input MFMA peak of the MI355X


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


def torch_assign(x, cb, chunk=65536):
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for a in range(0, x.shape[0], chunk):
        out[a:a + chunk] = torch.cdist(x[a:a + chunk], cb).argmin(1)
    return out


def torch_update(x, idx, K):
    sums = torch.zeros((K, x.shape[1]), device=x.device).index_add_(0, idx, x)
    cnt = torch.zeros(K, device=x.device).index_add_(0, idx, torch.ones(x.shape[0], device=x.device))
    return sums / cnt.clamp_min(1.0)[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--codes", type=int, nargs="+", default=[4096, 256])
    ap.add_argument("--dim", type=int, default=45)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gsr_pkg
    pkg = gsr_pkg.load()
    L = pkg._lib
    lib = L.load()
    n, dim = args.n, args.dim
    g = torch.Generator(device="cuda").manual_seed(21)
    x = torch.randn((n, dim), device="cuda", generator=g) * torch.linspace(1.0, 0.05, dim, device="cuda")
    lines = [f"device: {torch.cuda.get_device_name(0)}; n = {n}, dim = {dim}; median (min .. max) of {args.runs} runs after "
             f"{args.warmup} warm-up runs, device events"]
    st = L.stream()
    for K in args.codes:
        cb = x[(torch.arange(K, device="cuda") * n) // K].contiguous()
        idx = torch.zeros(n, dtype=torch.uint16, device="cuda")
        sums = torch.zeros((K, dim), dtype=torch.int64, device="cuda")
        wsum = torch.zeros(K, dtype=torch.int64, device="cuda")
        nb = int(lib.gsr_vq_scratch_bytes(n, K, dim))
        scr = torch.empty(nb, dtype=torch.uint8, device="cuda")
        new_cb = cb.clone()

        def assign():
            L.check(lib.gsr_vq_assign(n, K, dim, L.ptr(x), L.ptr(cb), None, L.ptr(idx), None, None, L.ptr(scr), nb, st))

        def accumulate(which):
            L.check(lib.gsr_vq_accumulate(n, K, dim, L.ptr(x), L.ptr(which), None, L.ptr(sums), L.ptr(wsum), st))

        def update():
            L.check(lib.gsr_vq_update(K, dim, L.ptr(sums), L.ptr(wsum), L.ptr(new_cb), None, st))

        assign()
        t_idx = torch_assign(x, cb)
        torch.cuda.synchronize()
        idx64 = idx.view(torch.int16).to(torch.int64) & 0xFFFF
        same = float((idx64 == t_idx).double().mean())
        hot = torch.where(torch.rand(n, device="cuda", generator=g) < 0.9, torch.full_like(idx64, 7 % K), idx64)
        hot = hot.to(torch.int16).view(torch.uint16)   # (K <= 32768 here)
        t_as = median_ms(assign, args.warmup, args.runs)
        t_un = median_ms(lambda: accumulate(idx), args.warmup, args.runs)
        t_hot = median_ms(lambda: accumulate(hot), args.warmup, args.runs)
        t_up = median_ms(update, args.warmup, args.runs)
        t_ta = median_ms(lambda: torch_assign(x, cb), 1, max(3, args.runs // 3))
        t_tu = median_ms(lambda: torch_update(x, t_idx, K), 1, max(3, args.runs // 3))
        tf = 2.0 * n * K * dim / t_as[0] / 1e9
        lines.append(f"K = {K:5d}: assign {t_as[0]:8.3f} ms ({t_as[1]:.3f} .. {t_as[2]:.3f}) = {tf:6.1f} TF, {100 * tf / PEAK_TF:4.1f} % of the {PEAK_TF:.0f} TF "
                     f"f32 MFMA peak; accumulate {t_un[0]:.3f} ms ({t_un[1]:.3f} .. {t_un[2]:.3f}) as assigned, {t_hot[0]:.3f} ms "
                     f"({t_hot[1]:.3f} .. {t_hot[2]:.3f}) with 90 % in one code; update {t_up[0]:.3f} ms; one iteration "
                     f"{t_as[0] + t_un[0] + t_up[0]:.3f} ms.  torch: cdist + argmin {t_ta[0]:.3f} ms, index_add_ update {t_tu[0]:.3f} ms, "
                     f"torch / HIP = {(t_ta[0] + t_tu[0]) / (t_as[0] + t_un[0] + t_up[0]):.1f}; same index as torch on {100 * same:.3f} % of the rows")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
