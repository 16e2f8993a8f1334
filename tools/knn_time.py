"""Times the point-cloud initialisation (point_cloud.compute_scales: gsr_morton_codes + argsort, then the two passes of
gsr_knn_scales, csrc/knn.hip) at N = 200 000 and N = 1 000 000 on two clouds — the surface points of
synthetic.make_trained_like (jittered, as tools/train_harness.py initial_model draws them) and a dense blob with far
outliers (coordinate ratio 1e4) — against the only thing the project had before: the host KD-tree of
train_harness.compute_scales (scipy.spatial.cKDTree) on the same points, where scipy imports.

Device milliseconds are between two device events on the current stream: the median of `--runs` timed runs after `--warmup`
untimed ones.  The split of gsr_knn_scales into its gather and search kernels comes from torch.profiler's kernel records
(`null` where the profiler reports none).  Not part of bench.py; run it under a timeout of its own:

    timeout 900 python tools/knn_time.py [--out profiles/knn/knn_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


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
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def surface_points(pkg, n, seed):
    """n jittered surface points of a trained-like scene (train_harness.initial_model's draw)."""
    gt = pkg.synthetic.make_trained_like(max(2 * n, 100_000), 1920, 1080, 0, seed, sigma_px=4.0, subclip_fraction=0.1)
    rng = np.random.default_rng(seed + 17)
    solid = np.flatnonzero(gt.opacities_raw > 0.0)
    idx = rng.choice(solid, n, replace=solid.size < n)
    pts = gt.means[idx].astype(np.float64)
    pts += rng.normal(0.0, 2e-3, pts.shape) * np.maximum(pts[:, 2:3], 0.5)
    return np.ascontiguousarray(pts, np.float32)


def blob_outliers(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.normal(0.0, 1.0, (n, 3))
    k = max(1, n // 16)
    d = rng.normal(0.0, 1.0, (k, 3))
    p[rng.choice(n, k, replace=False)] = 1e4 * d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(p, np.float32)


def kernel_split_ms(fn, runs):
    """{kernel name fragment: mean device ms per launch} of the two knn kernels, from torch.profiler; None if it has none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(runs):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            for frag in ("knn_gather_kernel", "knn_search_kernel"):
                if frag in e.key:
                    t = getattr(e, "device_time_total", None)
                    if t is None:
                        t = getattr(e, "cuda_time_total", 0.0)
                    out[frag] = dict(mean_ms=float(t) / 1e3 / max(int(e.count), 1), launches=int(e.count))
        return out or None
    except Exception as ex:  # the record is the events' totals; the split is extra
        return dict(error=repr(ex))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200_000, 1_000_000])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gsr_pkg
    pkg = gsr_pkg.load()
    L, PC = pkg._lib, pkg.point_cloud
    lib = L.load()
    try:
        import train_harness
        from scipy.spatial import cKDTree  # noqa: F401
        host = train_harness.compute_scales
    except Exception:
        host = None
    result = dict(runs=args.runs, warmup=args.warmup, device=torch.cuda.get_device_name(0), cases=[])
    for n in args.sizes:
        for cloud, pts_h in (("trained_like_surface", surface_points(pkg, n, 2024)), ("blob_outliers", blob_outliers(n, 7))):
            pts = torch.from_numpy(pts_h).cuda()
            box = torch.cat([pts.amin(0), pts.amax(0)]).tolist()
            codes = torch.empty(n, dtype=torch.int64, device="cuda")
            lo, hi = (C.c_float * 3)(*box[:3]), (C.c_float * 3)(*box[3:])
            perm = PC.morton_permutation(pts, box)
            nb = int(lib.gsr_knn_scratch_bytes(n))
            scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
            scales = torch.empty((n, 3), device="cuda")

            def order():
                L.check(lib.gsr_morton_codes(n, L.ptr(pts), lo, hi, L.ptr(codes), L.stream()))
                return torch.argsort(codes, stable=True).to(torch.int32)

            def knn():
                L.check(lib.gsr_knn_scales(n, L.ptr(pts), L.ptr(perm), 1.0, 3, L.ptr(scales), None, L.ptr(scratch), nb, L.stream()))

            def whole():
                PC.compute_scales(pts)

            case = dict(n=n, cloud=cloud, unique_points=int(np.unique(pts_h, axis=0).shape[0]),
                        codes_argsort=median_ms(order, args.warmup, args.runs), knn_scales=median_ms(knn, args.warmup, args.runs),
                        compute_scales_with_host_read=median_ms(whole, args.warmup, args.runs),
                        knn_kernels=kernel_split_ms(knn, 5))
            if host is not None and args.host_runs > 0:
                ts = []
                for _ in range(args.host_runs):
                    t0 = time.perf_counter()
                    want = host(pts_h)
                    ts.append((time.perf_counter() - t0) * 1e3)
                case["host_ckdtree_ms"] = float(np.median(ts))
                case["host_runs"] = args.host_runs
                case["max_abs_scale_difference_to_host"] = float(np.abs(scales.cpu().numpy() - want).max())
                case["host_over_device"] = case["host_ckdtree_ms"] / (case["codes_argsort"]["median_ms"] + case["knn_scales"]["median_ms"])
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
