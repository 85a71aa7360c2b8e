"""Times sliding-window inference at a size a user would run: the C3a autoencoder (CFG:821-862 for a 128^3 single-channel dataset)
reconstructing a 192 x 256 x 256 case with roi 128^3, overlap 0.25, sw_batch_size 2, Gaussian blend (18 windows, 9 network calls).

  kernels     device-event time of every mi_sw_* call of one eager run (_lib.profile_calls), per window batch, with the bytes each
              pass has to move computed from the shapes -> achieved GB/s (a rate over event time: it includes the launch gaps of the
              per-row accumulate launches)
  network     device events around each network call of an eager run of its own (the profiler's events between the network's kernels
              would inflate it)
  end to end  median host-clock time around a device synchronise, eager against captured (use_graph=True), outputs compared
  full        one whole-volume `reconstruct` of the same case, its time and peak memory, or the error if it does not fit

Prints one JSON line.  Not part of bench.py.
    python tools/bench_sliding.py [--runs 5] [--case 192 256 256] [--roi 128] [--batch 2] [--no-full]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medical_image_generation_amd import _lib  # noqa: E402
from medical_image_generation_amd.autoencoderkl import AutoencoderKL  # noqa: E402
from medical_image_generation_amd.sliding import SlidingWindowInferer, WindowPlan, tiled_reconstruct  # noqa: E402

_DOWN = [[[1] * 3, [3] * 3, [1] * 3], [[2] * 3, [3] * 3, [1] * 3], [[2] * 3, [3] * 3, [1] * 3]]
C3A = dict(spatial_dims=3, in_channels=1, out_channels=1, latent_channels=8, num_res_blocks=2, num_channels=[32, 64, 128],
           attention_levels=[False, False, False], norm_num_groups=16, with_encoder_nonlocal_attn=False, with_decoder_nonlocal_attn=False,
           downsample_parameters=_DOWN, upsample_parameters=list(reversed(_DOWN))[:-1])


def make_case(shape):
    g = torch.meshgrid(*[torch.linspace(-1, 1, s) for s in shape], indexing="ij")
    r2 = g[0] ** 2 + g[1] ** 2 + g[2] ** 2
    x = torch.where(r2 < 0.9, 0.5 + 0.5 * torch.cos(5 * g[0]) * torch.cos(3 * g[1]) * torch.cos(4 * g[2]), torch.zeros(()))
    return x[None, None].contiguous()


def pass_bytes(plan, n, batch, channels=1):
    """Bytes per call of each entry point, from the shapes: input and output windows have the roi's extent here (reconstruct)."""
    t = math.prod(plan.roi)
    full = math.prod(plan.padded)
    gather = 2 * 4 * batch * channels * t                       # image read, tiles written
    acc_row = 4 * (channels * t + t + 2 * channels * t + 2 * t)  # pred, imp, acc read + written, wsum read + written (n == 0 rows)
    finish = 4 * (2 * n * channels * math.prod(plan.image) + math.prod(plan.image))
    return {"mi_sw_gather": gather, "mi_sw_accumulate": batch * acc_row, "mi_sw_finish": finish, "accumulator_bytes": 4 * (n * channels + 1) * full}


def timed_ms(fn, runs):
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--case", type=int, nargs=3, default=(192, 256, 256))
    ap.add_argument("--roi", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--no-full", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sliding.py measures on the GPU: no device found")
    torch.manual_seed(0)
    ae = AutoencoderKL(**C3A).cuda().eval()
    x = make_case(tuple(args.case)).cuda()
    kw = dict(roi_size=args.roi, sw_batch_size=args.batch, overlap=0.25, mode="gaussian")
    eager, captured = SlidingWindowInferer(**kw), SlidingWindowInferer(use_graph=True, **kw)
    plan = WindowPlan(tuple(args.case), args.roi, 0.25)
    calls = -(-plan.num_windows // args.batch)
    out = {"case": list(args.case), "roi": list(plan.roi), "windows": plan.num_windows, "network_calls": calls, "sw_batch_size": args.batch,
           "runs": args.runs}

    for _ in range(2):  # warm-up: conv plans, workspaces, the capture
        ref = tiled_reconstruct(ae, x, eager)
        got = tiled_reconstruct(ae, x, captured)
    out["captured_equals_eager"] = bool(torch.equal(ref, got))
    _, t_eager = timed_ms(lambda: tiled_reconstruct(ae, x, eager), args.runs)
    _, t_graph = timed_ms(lambda: tiled_reconstruct(ae, x, captured), args.runs)
    out["eager_ms_median"], out["eager_ms_min_max"] = round(statistics.median(t_eager), 3), [round(min(t_eager), 3), round(max(t_eager), 3)]
    out["captured_ms_median"], out["captured_ms_min_max"] = round(statistics.median(t_graph), 3), [round(min(t_graph), 3), round(max(t_graph), 3)]

    # the network call per window batch
    marks = []

    def network(t):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        p = ae.reconstruct(t)
        e1.record()
        marks.append((e0, e1))
        return p

    eager(x, network)
    torch.cuda.synchronize()
    net_ms = [e0.elapsed_time(e1) for e0, e1 in marks]
    out["network_ms_per_batch_median"], out["network_ms_total"] = round(statistics.median(net_ms), 3), round(sum(net_ms), 3)

    # the three blend kernels
    with _lib.profile_calls() as prof:
        tiled_reconstruct(ae, x, eager)
    torch.cuda.synchronize()
    need = pass_bytes(plan, 1, args.batch)
    out["accumulator_bytes"] = need.pop("accumulator_bytes")
    kernels, blend_total = {}, 0.0
    for name in ("mi_sw_gather", "mi_sw_accumulate", "mi_sw_finish"):
        ms = [e0.elapsed_time(e1) for n, e0, e1 in prof.records if n == name]
        blend_total += sum(ms)
        med = statistics.median(ms)
        kernels[name] = {"calls": len(ms), "ms_median": round(med, 4), "ms_total": round(sum(ms), 3), "bytes_per_call": need[name],
                         "GB/s": round(need[name] / med / 1e6, 1)}
    out["kernels"] = kernels
    out["blend_ms_total"] = round(blend_total, 3)
    out["blend_share_of_kernel_time"] = round(blend_total / (blend_total + sum(net_ms)), 4)

    if not args.no_full:
        del ref, got
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.max_memory_allocated()
        try:
            with torch.no_grad():
                ae.reconstruct(x)
                _, t_full = timed_ms(lambda: ae.reconstruct(x), max(1, args.runs // 2))
            out["full_volume_ms_median"] = round(statistics.median(t_full), 3)
            out["full_volume_peak_bytes"] = int(torch.cuda.max_memory_allocated())
        except (RuntimeError, _lib.HipError) as e:  # does not fit (or a kernel refuses the extent): that is the finding
            out["full_volume_error"] = f"{type(e).__name__}: {str(e)[:200]}"
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        tiled_reconstruct(ae, x, eager)
        torch.cuda.synchronize()
        out["tiled_peak_bytes"] = int(torch.cuda.max_memory_allocated())
        out["resident_before_bytes"] = int(base)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
