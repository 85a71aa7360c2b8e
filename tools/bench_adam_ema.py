"""Time the fused optimizer launch with and without the averaged-weights shadow (mi_adam_step_dev vs mi_adam_ema_step_dev).

Sizes: the parameter counts of the two flagship networks, n = 41,336,641 and n = 441,490,952.  Per size and per form -- the entry
point alone (its launch pair: step-count increment + update) and FusedAdam.launch() with clipping (mi_sumsq_f32 in front) -- the
shadow-off and shadow-on launches alternate in one timed loop, each bracketed by HIP events; medians, the implied GB/s over the
arrays the update must move (4 read + 3 written = 28 B per parameter; 5 + 4 = 36 B with the shadow; + 4 B for the norm) and the
on / off ratio next to the ratio of those byte counts.

    python tools/bench_adam_ema.py [--warmup 5] [--reps 20] [--sizes 41336641 441490952]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medical_image_generation_amd._lib import call, ptr  # noqa: E402


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def case(n, clip, warmup, reps):
    g = torch.Generator(device="cuda").manual_seed(0)
    p, e = (torch.randn(n, generator=g, device="cuda") for _ in range(2))
    grad = 0.01 * torch.randn(n, generator=g, device="cuda")
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    step, sumsq = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    hp = torch.tensor([2e-5, 0.9, 0.999, 1e-8, 0.01, 1.0, 0.9999, 0.0], device="cuda")
    tail = (n, ptr(hp), 1, ptr(sumsq) if clip else None, 1.0, ptr(step))

    def launch(shadow):
        if clip:
            call("mi_sumsq_f32", ptr(grad), n, ptr(sumsq), 0)
        if shadow:
            call("mi_adam_ema_step_dev", ptr(p), ptr(grad), ptr(m), ptr(v), ptr(e), *tail)
        else:
            call("mi_adam_step_dev", ptr(p), ptr(grad), ptr(m), ptr(v), *tail)

    times = {False: [], True: []}
    for i in range(warmup + reps):
        for shadow in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(shadow)
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[shadow].append(e0.elapsed_time(e1))
    off, on = _median(times[False]), _median(times[True])
    b_off, b_on = 28 + 4 * clip, 36 + 4 * clip
    res = dict(n=n, form="sumsq + adam (clip)" if clip else "adam entry point", warmup=warmup, reps=reps, off_ms=round(off, 4), on_ms=round(on, 4),
               off_GBps=round(b_off * n / off / 1e6, 1), on_GBps=round(b_on * n / on / 1e6, 1), ratio=round(on / off, 4),
               bytes_ratio=round(b_on / b_off, 4), off_min_max_ms=[round(min(times[False]), 4), round(max(times[False]), 4)],
               on_min_max_ms=[round(min(times[True]), 4), round(max(times[True]), 4)])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[41336641, 441490952])
    a = ap.parse_args()
    if a.warmup < 5 or a.reps < 20:
        ap.error("at least 5 warm-up and 20 timed launches")
    if not torch.cuda.is_available():
        sys.exit("bench_adam_ema.py needs a GPU: there is nothing to time without one")
    for n in a.sizes:
        for clip in (False, True):
            case(n, clip, a.warmup, a.reps)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
