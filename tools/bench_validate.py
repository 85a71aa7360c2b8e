"""Time one validation step of the fused trainers (trainer.validate_graph / validate) against what the loop needs without them.

Shapes: C4 (the bench.py net, 1 x 1 x 128^3: LDM.validate_epoch's batch, train_ldm.py:206-229) and C3a (the planner's AutoencoderKL,
2 x 1 x 128^3: AutoEncoder.validate_one_epoch's batch, train_autoencoder.py:447-456).  Per shape, one child process per path:

    graph   validate_graph(): one hipGraph replay per batch
    eager   validate(): the same kernels launched from Python
    torch   the loop without the trainer's validation: torch q-sample + the drop-in module under torch.no_grad() (fp32 NCDHW in and
            out) + F.mse_loss(pred.float(), target)  [AE: model(images) + F.l1_loss], measured three times over (run-to-run spread)
    train   for orientation: the captured train step and one eager forward_backward at the same shape

and one child for the three reductions alone (achieved GB/s, bytes = both operands once, beside mi_mse_fwd_bwd / mi_l1_fwd_bwd
without a gradient tensor on the same operands).

Every figure is a median of `--steps` steps after `--warmup` steps.  `ms` fences every step with torch.cuda.synchronize(); `ms_item`
reads the batch loss on the host every step (`.item()`, what the reference's loop does) and `ms_loop` is the whole loop with ONE
synchronisation at its end divided by the step count (what a ValidationMeter allows).  peak_MiB: torch.cuda.max_memory_allocated over
the timed steps minus what was resident before them.

Each child runs under its own `timeout`; the driver stops at the first child that does not exit with status 0.

    python tools/bench_validate.py [--steps 20] [--warmup 5] [--only c4|c3a|kernels]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD_TIMEOUT_S = 240


def _measure(fn, steps, warmup, item=None):
    """fn() -> device loss.  -> dict(ms, ms_item, ms_loop, peak_MiB)."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    item = item or (lambda loss: loss.item())

    def fenced(read):
        out = []
        for _ in range(steps):
            t0 = time.perf_counter()
            loss = fn()
            if read:
                item(loss)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    ms, ms_item = fenced(False), fenced(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = fn()
    torch.cuda.synchronize()
    ms_loop = (time.perf_counter() - t0) * 1e3 / steps
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    return dict(ms=round(ms, 3), ms_item=round(ms_item, 3), ms_loop=round(ms_loop, 3), peak_MiB=round(peak, 1), loss=float(loss))


def _c4():
    import torch
    import bench
    from medical_image_generation_amd.trainer import DDPMTrainer
    from medical_image_generation_amd.unet import DiffusionModelUNet
    torch.manual_seed(0)
    net = DiffusionModelUNet(**bench.C4)
    for p in net.parameters():  # zero_module'd tensors: a zero output is not a measurement of anything
        if float(p.detach().abs().max()) == 0:
            torch.nn.init.normal_(p, std=0.02)
    net = net.cuda()
    shape = (1, 1, 128, 128, 128)
    x0 = bench.synthetic_volume(shape, 3, torch.device("cuda"))
    noise = torch.randn(shape, device="cuda")
    t = torch.tensor([500], device="cuda")
    return net, DDPMTrainer(net, lr=2e-5), (x0, noise, t)


def _c3a():
    import torch
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    from medical_image_generation_amd.trainer import AETrainer
    down = [[[1] * 3, [3] * 3, [1] * 3], [[2] * 3, [3] * 3, [1] * 3], [[2] * 3, [3] * 3, [1] * 3]]
    kw = dict(spatial_dims=3, in_channels=1, out_channels=1, latent_channels=8, num_res_blocks=2, num_channels=[32, 64, 128],
              attention_levels=[False] * 3, norm_num_groups=16, with_encoder_nonlocal_attn=False, with_decoder_nonlocal_attn=False,
              downsample_parameters=down, upsample_parameters=list(reversed(down))[:-1])
    torch.manual_seed(0)
    net = AutoencoderKL(**kw).cuda()
    x = torch.rand((2, 1, 128, 128, 128), device="cuda")
    eps = torch.randn((2, 8, 32, 32, 32), device="cuda")
    return net, AETrainer(net, lr=5e-5, kl_weight=1e-7), (x, eps)


def child(shape, path, steps, warmup):
    import torch
    import torch.nn.functional as F
    net, tr, args = (_c4 if shape == "c4" else _c3a)()
    rec = dict(shape=shape, path=path)
    if path == "graph":
        tr.capture_validate(*args)
        rec.update(_measure(lambda: tr.validate_graph(), steps, warmup))
    elif path == "eager":
        rec.update(_measure(lambda: tr.validate(*args), steps, warmup))
    elif path == "torch":
        if shape == "c4":
            x0, noise, t = args
            sa, so = tr.schedule.sqrt_acp, tr.schedule.sqrt_1macp

            def fn():
                with torch.no_grad():
                    noisy = sa[t].view(-1, 1, 1, 1, 1) * x0 + so[t].view(-1, 1, 1, 1, 1) * noise
                    return F.mse_loss(net(noisy, t).float(), noise)
        else:
            x, eps = args
            net.sampling = lambda mu, sigma: mu + eps * sigma  # the same noise every step, like the other paths

            def fn():
                with torch.no_grad():
                    return F.l1_loss(net(x)[0].float(), x)
        reps = [_measure(fn, steps, warmup if k == 0 else 1) for k in range(3)]
        rec.update(reps[0])
        for key in ("ms", "ms_item", "ms_loop"):
            vals = [r[key] for r in reps]
            rec[key + "_reps"] = vals
            rec[key] = statistics.median(vals)
            rec[key + "_spread"] = round(max(vals) - min(vals), 3)
    elif path == "train":
        fb = _measure(lambda: (tr.forward_backward(*args), tr.loss)[1], max(3, steps // 4), 2)
        rec.update(forward_backward_ms=fb["ms"], forward_backward_peak_MiB=fb["peak_MiB"])
        tr.capture(*args)
        g = _measure(lambda: tr.step_graph(), steps, warmup)
        rec.update(step_graph_ms=g["ms"], loss=g["loss"])
    print(json.dumps(rec), flush=True)


def child_kernels(steps, warmup):
    """The reductions alone on operands large enough to leave the launch floor: GB/s = (bf16 + fp32 operand bytes) / time."""
    import torch
    from medical_image_generation_amd._lib import call, ptr
    from medical_image_generation_amd.trainer import ValidationMeter
    m = ValidationMeter("cuda")
    loss = torch.zeros(1, device="cuda")

    def timed(fn):
        for _ in range(warmup):
            fn()
        out = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return statistics.median(out)

    for n, c, v in ((1, 1, 128 ** 3), (8, 1, 128 ** 3), (2, 8, 128 ** 3), (2, 8, 32 ** 3)):
        pred = torch.randn(n, v, c, device="cuda").to(torch.bfloat16)
        target = torch.randn(n, c, v, device="cuda")
        sigma = torch.rand(n, v, c, device="cuda").add_(0.5).to(torch.bfloat16)
        e = n * c * v
        runs = {
            "mi_mse_eval": (lambda: call("mi_mse_eval", ptr(pred), ptr(target), ptr(m.acc), n, c, v), 6 * e),
            "mi_l1_eval": (lambda: call("mi_l1_eval", ptr(pred), ptr(target), ptr(m.acc), n, c, v), 6 * e),
            "mi_kl_eval": (lambda: call("mi_kl_eval", ptr(pred), ptr(sigma), ptr(m.acc), n, c, v), 4 * e),
            "mi_mse_fwd_bwd (no gradient tensor)": (lambda: call("mi_mse_fwd_bwd", ptr(pred), ptr(target), None, ptr(loss), n, c, v, 1.0), 6 * e),
            "mi_l1_fwd_bwd (no gradient tensor)": (lambda: call("mi_l1_fwd_bwd", ptr(pred), ptr(target), None, ptr(loss), n, c, v, 0), 6 * e),
        }
        for name, (fn, byts) in runs.items():
            ms = timed(fn)
            print(json.dumps(dict(kernel=name, N=n, C=c, V=v, MB=round(byts / 1e6, 1), us=round(ms * 1e3, 1), GBps=round(byts / ms / 1e6, 1))),
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["c4", "c3a", "kernels"])
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "PATH"))
    a = ap.parse_args()
    if a.steps < 20 or a.warmup < 5:
        ap.error("medians of >= 20 steps after >= 5 warm-up steps")
    if a.child:
        if a.child[0] == "kernels":
            child_kernels(a.steps, a.warmup)
        else:
            child(a.child[0], a.child[1], a.steps, a.warmup)
        return
    jobs = [(s, p) for s in ("c4", "c3a") for p in ("graph", "eager", "torch", "train")] + [("kernels", "all")]
    for shape, path in jobs:
        if a.only and shape != a.only:
            continue
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--child", shape, path]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(f"bench_validate: `{shape} {path}` exited with status {rc}; stopping here", file=sys.stderr, flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    main()
