"""Times the geometry frames (gsr_depth_scale, gsr_frame_depth16, gsr_frame_normal8: csrc/frames.hip) on an :rgbdn frame of
1920x1080, and the reference's way of getting the white level — copy the 8-channel frame to the host, `quantile` there
(scripts/render-views.jl:396-402) — for scale.  Median of `--runs` timed runs after `--warmup` untimed ones, each between two
device events on the current stream (the host way: wall clock around the copy and the quantile).  Beside each time the
bytes the call has to move.  Not part of bench.py; run it under a timeout of its own:

    timeout 300 python tools/frames_time.py [--out profiles/frames/frames_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.eval_time import median_ms  # noqa: E402


def measured_triad_gbps(pkg):
    """The device's STREAM triad over 3 x 512 MiB, as bench.py --full measures `measured_triad_GBps`."""
    lib, n = pkg._lib.load(), 128 * 1024 * 1024
    ta, tb, tc = (torch.ones(n, device="cuda") for _ in range(3))
    cs = torch.cuda.current_stream().cuda_stream
    run = lambda: pkg._lib.check(lib.gsr_stream_triad(ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), n, 0.5, cs))  # noqa: E731
    for _ in range(2):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        run()
    e1.record()
    e1.synchronize()
    return 5 * 12.0 * n / (e0.elapsed_time(e1) * 1e-3) / 1e9


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
    GF = pkg.geometry_frames
    W, H, C = args.width, args.height, 8
    r = np.random.default_rng(0)
    host = r.uniform(0.0, 1.0, (H, W, C)).astype(np.float32)
    host[..., 3] = r.gamma(4.0, 1.5, (H, W)).astype(np.float32)          # depths with a long far tail
    host[..., 4] = np.where(r.integers(0, 8, (H, W)) == 0, 0.0, r.uniform(0.2, 1.0, (H, W))).astype(np.float32)
    host[..., 5:8] = r.normal(0.0, 0.5, (H, W, 3)).astype(np.float32)
    frame = torch.from_numpy(host).cuda()
    stats = torch.empty(4, dtype=torch.int32, device="cuda")
    scratch = torch.empty(GF.frames_scratch_bytes(W, H), dtype=torch.uint8, device="cuda")
    d16 = torch.empty((H, W), dtype=torch.uint16, device="cuda")
    n8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    R = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], np.float32)
    GF.depth_scale(frame, 99.0, stats=stats, scratch=scratch)
    torch.cuda.synchronize()
    lib, L = pkg._lib.load(), pkg._lib

    def encode_depth():
        L.check(lib.gsr_frame_depth16(W, H, C, frame.data_ptr(), 1, 1e-3, 0.0, stats.data_ptr(), 0, d16.data_ptr(), L.stream()))

    calls = {
        "depth_scale": (lambda: GF.depth_scale(frame, 99.0, stats=stats, scratch=scratch),
                        dict(key_pass=W * H * (8 + 4), narrow_pass_1=4 * W * H, narrow_pass_2=4 * W * H)),
        "frame_depth16": (encode_depth, dict(read=8 * W * H, write=2 * W * H)),
        "frame_normal8": (lambda: GF.frame_normal8(frame, None, out=n8), dict(read=16 * W * H, write=3 * W * H)),
        "frame_normal8_world": (lambda: GF.frame_normal8(frame, R, out=n8), dict(read=16 * W * H, write=3 * W * H)),
    }
    triad = measured_triad_gbps(pkg)
    result = dict(width=W, height=H, channels=C, runs=args.runs, warmup=args.warmup, device=torch.cuda.get_device_name(0),
                  measured_triad_GBps=round(triad, 1), calls={})
    for name, (fn, nbytes) in calls.items():
        ms = median_ms(fn, args.warmup, args.runs)
        total = int(sum(nbytes.values()))
        gbps = total / ms[0] * 1e-6
        result["calls"][name] = dict(ms=ms[0], min_max_ms=ms[1:], bytes=nbytes, bytes_total=total, GBps=gbps,
                                     frac_of_measured_triad=gbps / triad)
    # the reference's way: the whole frame to the host, the covered depths sorted there
    host_ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = frame.cpu().numpy()
        alpha = f[..., 4]
        e = (f[..., 3] / np.maximum(alpha, np.float32(1e-3)))[alpha >= np.float32(1e-3)]
        q = float(np.quantile(e, 0.99))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    dev_scale = float(stats[:1].view(torch.float32).item())
    result["host_copy_and_quantile_ms"] = float(np.median(host_ms))
    result["scale"] = dict(device=dev_scale, host_numpy=q)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
