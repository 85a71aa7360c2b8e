"""Times the case preprocessing on one case: 256 x 256 x 160 at spacing (0.8, 0.8, 2.5) resampled to (1, 1, 1) (an anisotropic case:
cubic along x and y, order 0 along z), cropped, transposed and normalised, with a label of three values.

GPU: median wall time of `preprocess_case` over --runs runs after warm-up (host clock around a device synchronise; the upload of
the raw case is outside the timed window), and the device-event time of every library call of one run (_lib.profile_calls) with the
bytes each pass has to move, computed from the shapes.  Host: the same resampling through `scipy.ndimage.zoom` per axis in fp64, as
the reference runs it (configuration.py:1125-1129), when scipy is importable.  Prints one JSON line.  Not part of bench.py.
    python tools/bench_preprocess.py [--runs 20] [--no-scipy] [--no-label]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medical_image_generation_amd import _lib, preprocess as P  # noqa: E402

SHAPE, SPACING, TARGET = (256, 256, 160), (0.8, 0.8, 2.5), (1.0, 1.0, 1.0)


def make_case(seed=0):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, s, dtype=np.float32) for s in SHAPE], indexing="ij")
    r2 = g[0] ** 2 + g[1] ** 2 + g[2] ** 2
    image = np.where(r2 < 0.8, 900.0 * np.cos(3 * g[0]) * np.cos(2 * g[1]) * np.cos(4 * g[2]) + rng.integers(-100, 101, SHAPE), 0.0).astype(np.float32)
    label = np.zeros(SHAPE, np.uint8)
    label[r2 < 0.3] = 1
    label[(g[0] - 0.4) ** 2 + g[1] ** 2 + g[2] ** 2 < 0.02] = 2
    return image, label


def pass_bytes():
    """name of the library call -> list of bytes moved per invocation, in call order, from the shapes alone"""
    shape, out = list(SHAPE), {}
    zoom = np.asarray(SPACING) / np.asarray(TARGET)
    orders = P.resample_orders(SPACING)
    for axis in range(3):
        n_in = int(np.prod(shape))
        n_out = int(round(shape[axis] * zoom[axis]))
        if orders[axis] == 3:
            out.setdefault("mi_pp_prefilter3", []).append(4 * 4 * n_in)  # x read, c written, c read, c written
        shape[axis] = n_out
        out.setdefault("mi_pp_resample_axis", []).append(4 * (n_in + int(np.prod(shape))))
    return out, tuple(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-label", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess.py measures on the GPU: no device found")
    image, label = make_case()
    dimage, dlabel = torch.from_numpy(image).cuda(), (None if args.no_label else torch.from_numpy(label).cuda())

    def run():
        return P.preprocess_case(dimage, SPACING, TARGET, label=dlabel)

    for _ in range(3):
        result = run()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    image_only = []  # without a label there is no class-location sampling on the host: what is left is the voxel passes and their launches
    for k in range(3 + args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P.preprocess_case(dimage, SPACING, TARGET)
        torch.cuda.synchronize()
        if k >= 3:
            image_only.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    with _lib.profile_calls() as prof:
        run()
    torch.cuda.synchronize()
    per_call = {}
    for name, e0, e1 in prof.records:
        per_call.setdefault(name, []).append(e0.elapsed_time(e1))
    need, resampled = pass_bytes()
    passes = []
    for name, ms_list in per_call.items():
        for k, ms in enumerate(ms_list):
            row = {"call": name, "index": k, "ms": round(ms, 4)}
            if name in need and k < len(need[name]):
                row["bytes"] = need[name][k]
                row["GB/s"] = round(need[name][k] / ms / 1e6, 1)
            passes.append(row)
    out = {"case": {"shape": SHAPE, "spacing": SPACING, "target": TARGET, "resampled": resampled, "box": result["box"]},
           "gpu_ms_median": round(statistics.median(times), 3), "gpu_ms_min": round(min(times), 3), "gpu_ms_max": round(max(times), 3),
           "gpu_ms_median_image_only": round(statistics.median(image_only), 3), "gpu_kernel_ms_total": round(sum(sum(v) for v in per_call.values()), 3), "passes": passes, "runs": args.runs}
    if not args.no_scipy:
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None:
            x = image.astype(np.float64)
            zoom, orders = np.asarray(SPACING) / np.asarray(TARGET), P.resample_orders(SPACING)
            t0 = time.perf_counter()
            for axis in range(3):
                x = ndimage.zoom(x, [zoom[a] if a == axis else 1 for a in range(3)], order=orders[axis])
            out["scipy_resample_s"] = round(time.perf_counter() - t0, 3)
            gpu_resample_ms = sum(sum(v) for k, v in per_call.items() if k in ("mi_pp_prefilter3", "mi_pp_resample_axis"))
            out["gpu_resample_ms"] = round(gpu_resample_ms, 3)
            out["resample_speedup"] = round(out["scipy_resample_s"] * 1e3 / gpu_resample_ms, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
