"""Times tiled diffusion sampling (`sample(..., window_inferer=)`) at a size a user would run: the C4 U-Net of bench.py, trained on 64^3
patches, generating a 96 x 160 x 160 case under 64^3 windows at overlap 0.25, sw_batch_size 2, Gaussian blend (18 windows, 9 model
calls per step), DDIM.

  step        host-clock time around a device synchronise of captured runs of K and 2K steps (median of --runs each): the per-step time is
              their difference over K, the rest is the per-run set-up (weight sum, staging, the copy of the start)
  plain       the same for the plain sampler at the window batch's shape (sw_batch_size x 64^3): what one model call of a step costs
              without tiling; ratio = tiled step / (calls x plain step)
  passes      device-event time of every library call of one eager step (_lib.profile_calls): the three voxel passes against everything
              else (the U-Net's kernels), with the bytes each pass has to move computed from the shapes -> achieved GB/s (a rate over
              event time: it includes the launch gaps of the per-row accumulate launches)

Prints one JSON line.  Not part of bench.py.
    python tools/bench_tiled_sampling.py [--runs 5] [--steps 10] [--case 96 160 160] [--roi 64] [--batch 2] [--overlap 0.25]
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
from medical_image_generation_amd.inferer import DDIMScheduler, DiffusionInferer  # noqa: E402
from medical_image_generation_amd.sliding import SlidingWindowInferer, WindowPlan  # noqa: E402
from medical_image_generation_amd.unet import DiffusionModelUNet  # noqa: E402

C4 = dict(spatial_dims=3, in_channels=1, out_channels=1, num_res_blocks=2, num_channels=(32, 64, 128, 256),
          attention_levels=(False, False, False, True), num_head_channels=(0, 0, 0, 64), norm_num_groups=32,
          strides=[[1] * 3] + [[2] * 3] * 3, kernel_sizes=[[3] * 3] * 4, paddings=[[1] * 3] * 4)
PASSES = ("mi_sw_gather_cl", "mi_sw_accumulate_cl", "mi_sw_diffusion_step")


def pass_bytes(n, c, case, roi, batch, calls):
    """Bytes one step has to move per entry point, from the shapes (unguided, no condition, eta 0: z is not read)."""
    t, v = math.prod(roi), math.prod(case)
    return {"mi_sw_gather_cl": calls * batch * c * t * (4 + 2),                    # fp32 window read, bf16 model input written
            "mi_sw_accumulate_cl": calls * batch * t * (2 * c + 4 + 8 * c),        # bf16 prediction, map, accumulator read and written
            "mi_sw_diffusion_step": n * c * v * 4 * 4 + 4 * v}                     # acc and x read and written, the weight sum read


def timed_ms(fn, runs):
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def per_step(run, sch, steps, runs):
    """run(): one sampling run with the scheduler's current step count -> (ms per step, ms of per-run set-up, spread of the K runs)."""
    out = {}
    for k in (steps, 2 * steps):
        sch.set_timesteps(k)
        run()  # warm-up at this step count (the first one also plans and captures)
        out[k] = timed_ms(run, runs)
    step = (out[2 * steps][0] - out[steps][0]) / steps
    return step, out[steps][0] - steps * step, out[steps][1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--case", type=int, nargs=3, default=[96, 160, 160])
    ap.add_argument("--roi", type=int, default=64)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--overlap", type=float, default=0.25)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiled_sampling.py measures on an MI355X: no GPU found")
    _lib.load()
    torch.manual_seed(0)
    net = DiffusionModelUNet(**C4).cuda().eval()
    case, roi = tuple(args.case), (args.roi,) * 3
    plan = WindowPlan(case, roi, args.overlap)
    calls = plan.rows(1, args.batch).shape[0]
    sch = DDIMScheduler(1000)
    inf = DiffusionInferer(sch)
    win = SlidingWindowInferer(roi, args.batch, args.overlap, "gaussian")
    g = torch.Generator(device="cuda").manual_seed(0)
    x0 = torch.randn((1, 1) + case, device="cuda", generator=g)
    p0 = torch.randn((args.batch, 1) + roi, device="cuda", generator=g)

    tiled = per_step(lambda: inf.sample(x0, net, sch, verbose=False, window_inferer=win), sch, args.steps, args.runs)
    plain = per_step(lambda: inf.sample(p0, net, sch, verbose=False), sch, args.steps, args.runs)

    # one eager step under device events: the voxel passes against the rest (the U-Net)
    sch.set_timesteps(args.steps)
    loop = next(l for l in inf._loops.values() if hasattr(l, "plan"))
    graph, loop.graph = loop.graph, None
    loop._step()  # warm
    with _lib.profile_calls() as prof:
        loop._step()
    ms = prof.summary()
    loop.graph = graph
    total = sum(ms.values())
    nbytes = pass_bytes(1, 1, case, roi, args.batch, calls)
    passes = {name: {"ms": round(ms.get(name, 0.0), 4), "bytes": nbytes[name],
                     "GBps": round(nbytes[name] / (ms[name] * 1e-3) / 1e9, 1) if ms.get(name) else None} for name in PASSES}
    outside = sum(ms.get(name, 0.0) for name in PASSES)
    print(json.dumps({
        "config": {"net": "C4", "case": case, "roi": roi, "overlap": args.overlap, "sw_batch_size": args.batch, "windows": plan.num_windows,
                   "calls_per_step": calls, "scheduler": "DDIM eta 0", "steps": [args.steps, 2 * args.steps], "runs": args.runs},
        "tiled_step_ms": round(tiled[0], 3), "tiled_run_setup_ms": round(tiled[1], 3), "tiled_run_min_max_ms": [round(v, 2) for v in tiled[2]],
        "plain_step_ms_at_window_batch": round(plain[0], 3), "plain_run_min_max_ms": [round(v, 2) for v in plain[2]],
        "ratio_tiled_over_calls_x_plain": round(tiled[0] / (calls * plain[0]), 4),
        "eager_step_device_ms": round(total, 3), "voxel_passes_device_ms": round(outside, 4),
        "share_outside_unet_device_time": round(outside / total, 4), "passes": passes}))


if __name__ == "__main__":
    main()
