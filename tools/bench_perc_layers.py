"""Per-layer time and TF/s of the 13 VGG16 3x3 convs of the perceptual term at C3a (fake 3-D, ratio 0.2: 51 slices of 128^2 per axis),
forward and data gradient on the library's 2-D conv plans, timed with HIP events around each launch (eager, after warm-up).
usage: python tools/bench_perc_layers.py [slices] [side] [reps]  ->  one JSON line per layer and pass, then a total line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from medical_image_generation_amd import hipops as ops
from medical_image_generation_amd.perceptual import VGG_LEVELS, PerceptualLoss

s = int(sys.argv[1]) if len(sys.argv) > 1 else 51
side = int(sys.argv[2]) if len(sys.argv) > 2 else 128
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
dev = torch.device("cuda")
pl = PerceptualLoss(spatial_dims=3, fake_3d_ratio=0.2, pretrained=False).to(dev)
total = {"fwd": 0.0, "dgrad": 0.0}
flops_total = 0
hw = side
for k, level in enumerate(VGG_LEVELS):
    if k > 0:
        hw //= 2
    for i, cin, cout in level:
        cin = 8 if i == 0 else cin
        plan = pl._plan(i, cin, cout, s, hw, hw)
        wt, bias = pl._weight(i)
        plan.pack(wt)
        x = torch.randn((s, 1, hw, hw, cin), device=dev).to(torch.bfloat16)
        y = plan.fwd(x, addvec=bias)
        dy = torch.randn_like(y.float()).to(torch.bfloat16)
        flops = 2 * s * hw * hw * cout * (3 if i == 0 else cin) * 9  # algorithmic (conv1_1: the 3 real input channels)
        flops_total += flops
        for name, fn in (("fwd", lambda: plan.fwd(x, addvec=bias)), ("dgrad", lambda: plan.dgrad(dy))):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            total[name] += ms
            print(json.dumps({"layer": f"features.{i}", "pass": name, "slices": s, "hw": hw, "cin": cin, "cout": cout, "ms": round(ms, 4),
                              "tflops": round(flops / ms / 1e9, 1)}), flush=True)
print(json.dumps({"total_ms_fwd_one_branch_one_axis": round(total["fwd"], 3), "total_ms_dgrad_one_axis": round(total["dgrad"], 3),
                  "fwd_tflops": round(flops_total / total["fwd"] / 1e9, 1), "dgrad_tflops": round(flops_total / total["dgrad"] / 1e9, 1),
                  "step_estimate_ms": round(3 * (2 * total["fwd"] + total["dgrad"]), 2)}), flush=True)
