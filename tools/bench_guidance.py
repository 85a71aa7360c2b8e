"""Time one classifier-free-guidance sample step (one forward at batch 2N + one guided update launch) against the two unguided steps
it replaces, at the latent U-Net test shape: `unet_ldm` rebuilt with in_channels=9 / out_channels=8 (one label channel, mode="concat"),
sample 2 x 8 x 8^3, DDIM.

    guided     one replay of the guided loop's captured step
    unguided   one replay of the unguided loop's captured step (the comparison is against TWO of them)
    *_eager    the same steps launched from Python

Every figure is the median of `--steps` steps after `--warmup` steps, each step fenced with torch.cuda.synchronize() (the practice of
tools/bench_validate.py); a step includes the two device-scalar fills the loop does before it.  One JSON line.

    python tools/bench_guidance.py [--steps 50] [--warmup 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    import torch
    from medical_image_generation_amd.inferer import DDIMScheduler, DiffusionInferer
    from medical_image_generation_amd.unet import DiffusionModelUNet
    kw = dict(spatial_dims=3, in_channels=9, out_channels=8, num_res_blocks=1, num_channels=(32, 64, 96), attention_levels=(False, True, True),
              num_head_channels=(0, 64, 96), norm_num_groups=32, strides=[[1] * 3, [2] * 3, [2] * 3], kernel_sizes=[[3] * 3] * 3,
              paddings=[[1] * 3] * 3)
    torch.manual_seed(0)
    net = DiffusionModelUNet(**kw)
    for p in net.parameters():  # zero_module'd tensors: a zero output is not a measurement of anything
        if float(p.detach().abs().max()) == 0:
            torch.nn.init.normal_(p, std=0.02)
    net = net.cuda().eval()
    shape = (2, 8, 8, 8, 8)
    x = torch.randn(shape, device="cuda")
    label = (torch.rand((2, 1, 8, 8, 8), device="cuda") > 0.5).float()
    sch = DDIMScheduler(1000, "linear_beta", beta_start=1e-4, beta_end=2e-3)
    sch.set_timesteps(4)
    inf = DiffusionInferer(sch)
    inf.sample(x, net, sch, conditioning=label, mode="concat", verbose=False)                      # builds and captures the unguided loop
    inf.sample(x, net, sch, conditioning=label, mode="concat", verbose=False, guidance_scale=2.0)  # ... and the guided one
    loops = {l.guided: l for l in inf._loops.values()}
    rec = dict(shape=list(shape), steps=a.steps, warmup=a.warmup)
    for name, loop in (("unguided", loops[False]), ("guided", loops[True])):
        assert loop.graph is not None

        def replay(loop=loop):
            loop.t.fill_(0)
            loop.tn.fill_(500)
            loop.graph.replay()

        def eager(loop=loop):
            loop.t.fill_(0)
            loop.tn.fill_(500)
            loop._step()

        rec[name + "_ms"] = _median_ms(replay, a.steps, a.warmup)
        rec[name + "_eager_ms"] = _median_ms(eager, a.steps, a.warmup)
    rec["guided_over_two_unguided"] = round(rec["guided_ms"] / (2 * rec["unguided_ms"]), 3)
    rec["guided_over_two_unguided_eager"] = round(rec["guided_eager_ms"] / (2 * rec["unguided_eager_ms"]), 3)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
