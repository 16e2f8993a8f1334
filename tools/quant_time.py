"""Times the quantised model container's kernels (csrc/quant.hip through gsr_quant_*) on the six groups of a degree-3 model —
points (n, 3) at 16 bits in blocks of 256, features_dc (n, 3), features_rest (n, 45), opacities (n, 1) and scales (n, 3) at 8 bits
with one block, rotations (n, 4) as 8-bit unit quaternions — beside the bytes each pass has to move at the bandwidth
gsr_stream_triad reaches in the same process, and beside the same operations as torch elementwise chains on the same device:

  ranges   the five linear groups, one call each        reads 4 bytes per element
  encode   the six groups, one call each                reads 4, writes 1 or 2 bytes per element
  decode   the six groups, one call each                reads 1 or 2, writes 4 bytes per element
  fake     the six groups in ONE gsr_quant_fake launch  reads 4, writes 4 bytes per element

Device milliseconds between two device events: the median (min .. max) of `--runs` runs after `--warmup` untimed ones.

    timeout 600 python tools/quant_time.py [--out profiles/quantised_model/times.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GROUPS = (("points", 3, 16, 256, 0), ("features_dc", 3, 8, 0, 0), ("features_rest", 45, 8, 0, 0), ("opacities", 1, 8, 0, 0),
          ("scales", 3, 8, 0, 0), ("rotations", 4, 8, 0, 1))


def timed(fn, warmup, runs):
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
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gsr_pkg
    pkg = gsr_pkg.load()
    L, Q = pkg._lib, pkg.quantised_model
    lib = L.load()
    n = args.n
    g = torch.Generator(device="cuda").manual_seed(25)
    st = L.stream()
    xs, rgs, codes, outs = {}, {}, {}, {}
    for name, cols, bits, br, kind in GROUPS:
        xs[name] = torch.randn((n, cols), device="cuda", generator=g)
        rgs[name] = None if kind else Q.quant_ranges(xs[name], br)
        codes[name] = Q.quant_encode(xs[name], bits, rgs[name], br, kind)
        outs[name] = torch.empty_like(xs[name])

    def ranges():
        for name, cols, bits, br, kind in GROUPS:
            if not kind:
                L.check(lib.gsr_quant_ranges(n, cols, L.ptr(xs[name]), br, L.ptr(rgs[name]), st))

    def encode():
        for name, cols, bits, br, kind in GROUPS:
            L.check(lib.gsr_quant_encode(n, cols, bits, kind, L.ptr(xs[name]), br, L.ptr(rgs[name]), L.ptr(codes[name]), st))

    def decode():
        for name, cols, bits, br, kind in GROUPS:
            L.check(lib.gsr_quant_decode(n, cols, bits, kind, L.ptr(codes[name]), br, L.ptr(rgs[name]), L.ptr(outs[name]), st))

    arr = (L.QuantGroup * len(GROUPS))(*[L.QuantGroup(xs[nm].data_ptr(), outs[nm].data_ptr(), cols, bits, kind, br,
                                                      rgs[nm].data_ptr() if rgs[nm] is not None else None)
                                         for nm, cols, bits, br, kind in GROUPS])

    def fake():
        L.check(lib.gsr_quant_fake(arr, len(GROUPS), n, st))

    # the same operations as torch elementwise chains (one range per column; the blocked positions as a (blocks, 256, 3) view)
    def t_ranges():
        for name, cols, bits, br, kind in GROUPS:
            if not kind:
                x = xs[name]
                x = x[: (n // br) * br].view(-1, br, cols) if br else x.view(1, n, cols)
                fin = torch.isfinite(x)
                torch.where(fin, x, torch.full_like(x, float("inf"))).amin(1), torch.where(fin, x, torch.full_like(x, float("-inf"))).amax(1)

    lohi = {}
    for name, cols, bits, br, kind in GROUPS:
        if kind:
            lo, hi = torch.full((1, cols), -1.0, device="cuda"), torch.full((1, cols), 1.0, device="cuda")
        else:
            r = rgs[name]
            lo, hi = (r[:, 0].repeat_interleave(br, 0)[:n], r[:, 1].repeat_interleave(br, 0)[:n]) if br else (r[:, 0], r[:, 1])
        Lf = float((1 << bits) - 1)
        lohi[name] = (lo.contiguous(), (Lf / (hi - lo)).contiguous(), ((hi - lo) / Lf).contiguous(), Lf)

    def t_encode_one(name, bits, kind):
        lo, inv, step, Lf = lohi[name]
        x = xs[name]
        if kind:
            x = x / x.norm(dim=1, keepdim=True) * torch.where(x[:, :1] < 0, -1.0, 1.0)
        return ((x - lo) * inv).nan_to_num(0.0).clamp(0.0, Lf).round().to(torch.uint8 if bits <= 8 else torch.int16)

    def t_decode_one(name, q):
        lo, inv, step, Lf = lohi[name]
        return torch.addcmul(lo, q.to(torch.float32), step)

    tq = {nm: t_encode_one(nm, bits, kind) for nm, cols, bits, br, kind in GROUPS}

    def t_encode():
        for name, cols, bits, br, kind in GROUPS:
            t_encode_one(name, bits, kind)

    def t_decode():
        for name, cols, bits, br, kind in GROUPS:
            t_decode_one(name, tq[name])

    def t_fake():
        for name, cols, bits, br, kind in GROUPS:
            t_decode_one(name, t_encode_one(name, bits, kind))

    # the bandwidth yardstick: a = b + q c over 64 M floats, 12 bytes per element
    cnt = 1 << 26
    ta, tb, tc = (torch.zeros(cnt, device="cuda") for _ in range(3))
    tri = timed(lambda: L.check(lib.gsr_stream_triad(L.ptr(ta), L.ptr(tb), L.ptr(tc), cnt, 0.5, st)), args.warmup, args.runs)
    bw = 12.0 * cnt / tri[0] / 1e6   # GB/s
    del ta, tb, tc

    el = sum(c for _, c, _, _, _ in GROUPS)
    el_lin = sum(c for _, c, _, _, k in GROUPS if not k)
    cb = sum(c * (1 if b <= 8 else 2) for _, c, b, _, _ in GROUPS)
    bytes_ = dict(ranges=4 * el_lin * n, encode=(4 * el + cb) * n, decode=(4 * el + cb) * n, fake=8 * el * n)
    lines = [f"device: {torch.cuda.get_device_name(0)}; n = {n}, the six groups of a degree-3 model ({el} floats, {cb} code bytes per "
             f"Gaussian); median (min .. max) of {args.runs} runs after {args.warmup} warm-up runs, device events",
             f"gsr_stream_triad over {cnt} floats: {tri[0]:.3f} ms = {bw:.0f} GB/s (the bandwidth of the floors below)"]
    for name, fn, tfn in (("ranges", ranges, t_ranges), ("encode", encode, t_encode), ("decode", decode, t_decode), ("fake", fake, t_fake)):
        t = timed(fn, args.warmup, args.runs)
        tt = timed(tfn, 1, max(3, args.runs // 3))
        floor = bytes_[name] / bw / 1e6
        lines.append(f"{name:6s}: {t[0]:7.3f} ms ({t[1]:.3f} .. {t[2]:.3f}); {bytes_[name] / 1e6:7.1f} MB -> floor {floor:.3f} ms, "
                     f"{t[0] / floor:.2f}x the floor; torch chain {tt[0]:.3f} ms, torch / HIP = {tt[0] / t[0]:.1f}")
        print(lines[-1], flush=True)
    # per group, the fake pass alone: which access regime costs what
    for nm, cols, bits, br, kind in GROUPS:
        one = (L.QuantGroup * 1)(L.QuantGroup(xs[nm].data_ptr(), outs[nm].data_ptr(), cols, bits, kind, br, rgs[nm].data_ptr() if rgs[nm] is not None else None))
        t = timed(lambda: L.check(lib.gsr_quant_fake(one, 1, n, st)), args.warmup, args.runs)
        floor = 8.0 * cols * n / bw / 1e6
        lines.append(f"  fake, {nm:13s} ({cols:2d} cols, {bits:2d} bits, block_rows {br:3d}{', unit quaternions' if kind else ''}): {t[0]:.3f} ms, {t[0] / floor:.2f}x its floor")
    print("\n".join(lines[:2] + lines[-6:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
