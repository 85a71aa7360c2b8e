"""Times the distribution metrics (metrics.py: distribution_scores, MMDMetric).

FID + KID: `distribution_scores` on two [n, 2048] feature matrices, n = m in --sizes (default 128 and 512): device-event time of one
call after a warm-up call (the call synchronises once per Jacobi sweep, so the events span those waits too), the sweeps run, and the
device-event time of every library call inside it (_lib.profile_calls).  Beside it, for information only, the path a caller has without
these metrics, on this machine's CPU: `torch.cov` in fp64 + `scipy.linalg.sqrtm` (skipped with a note when scipy is missing).
MMD: `MMDMetric` on two batches of 16 x 1 x 128^3 fp32: device time, the GB/s that time implies for ONE read of both inputs, and whether
the Gram pass was the single-pass grid (R <= 64: every element read from HBM once).  Prints one JSON line.  Not part of bench.py.
    python tools/bench_dist_metrics.py [--sizes 128 512] [--no-scipy] [--no-mmd]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medical_image_generation_amd import _lib, metrics as M  # noqa: E402

F = 2048


def features(seed, n):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, F, generator=g) @ torch.randn(F, F, generator=g) * 0.3 + 0.5


def device_ms(fn):
    fn()  # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def per_call_ms(fn):
    with _lib.profile_calls() as prof:
        fn()
    return {k: round(v, 4) for k, v in prof.summary().items()}


def host_fid(x, y):
    from scipy import linalg
    x, y = x.double(), y.double()
    t0 = time.perf_counter()
    sx, sy = torch.cov(x.T), torch.cov(y.T)
    covmean = linalg.sqrtm((sx @ sy).numpy())
    d = x.mean(0) - y.mean(0)
    v = float(d @ d + torch.trace(sx) + torch.trace(sy)) - 2.0 * float(covmean.real.trace())
    return time.perf_counter() - t0, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-mmd", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dist_metrics.py measures on the GPU: no device found")
    out = {"features": F, "fid_kid": []}
    for n in args.sizes:
        x, y = features(1, n), features(2, n)
        dx, dy = x.cuda(), y.cuda()
        ms, res = device_ms(lambda: M.distribution_scores(dx, dy))
        row = {"n": n, "m": n, "device_ms": round(ms, 3), "jacobi_sweeps": res["jacobi_sweeps"], "fid": float(res["fid"]), "kid": float(res["kid"]),
               "jacobi_single_workgroup": bool(_lib.call_raw("mi_dm_jacobi_single_workgroup", n, n)),
               "per_call_ms": per_call_ms(lambda: M.distribution_scores(dx, dy))}
        if not args.no_scipy:
            try:
                s, v = host_fid(x, y)
                row["host_cov_sqrtm_s"] = round(s, 3)
                row["host_fid"] = v
            except ImportError:
                print("scipy is not importable here: the host torch.cov + scipy.linalg.sqrtm path is skipped", file=sys.stderr)
        out["fid_kid"].append(row)
    if not args.no_mmd:
        shape = (16, 1, 128, 128, 128)
        g = torch.Generator().manual_seed(3)
        y, p = torch.rand(shape, generator=g).cuda(), torch.rand(shape, generator=g).cuda()
        mmd = M.MMDMetric()
        ms, v = device_ms(lambda: mmd(y, p))
        nbytes = 2 * y.numel() * 4
        out["mmd"] = {"shape": shape, "device_ms": round(ms, 3), "input_bytes": nbytes, "GB/s_one_read": round(nbytes / ms / 1e6, 1),
                      "single_pass": bool(_lib.call_raw("mi_dm_gram_single_pass", 2 * shape[0])), "value": float(v),
                      "per_call_ms": per_call_ms(lambda: mmd(y, p))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
