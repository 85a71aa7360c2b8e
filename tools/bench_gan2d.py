"""Time the 2-D GAN step of train_autoencoder.py (T-AE:371-435) with the native 2-D PatchDiscriminator against the route 2-D users had
before it existed.

Configuration: the planner's `'2D'` section -- AutoencoderKL(spatial_dims=2, latent 8, 2 res blocks, channels [32, 64, 128], 16 groups),
PatchDiscriminator(spatial_dims=2, num_channels=64, num_layers_d=3), kl_weight 1e-6, adv_weight 0.01, Adam 5e-5 / 5e-5, clip 1 -- on
16 x 1 x 256 x 256.  One child process per path, the two step paths alternating (`--reps` times each) on the same card:

    native   AEGANTrainer.step_graph(): generator and discriminator graphs, both networks on the HIP path
    torch    AETrainer(extra_loss=...) with the torch discriminator (oracle/disc.py restates upstream's) under bf16 autocast for the
             generator's adversarial term, and the discriminator step (two forwards, backward, clip, torch Adam) on the caller's side:
             eager, fp32 NCHW round trip per step, not capturable
    profile  one eager native step with device events around every library call: GPU milliseconds and calls per entry point
    kernels  the three MFMA kernels of csrc/disc2d.hip alone at 64->128 @128^2 (stride 2) and 256->512 @32^2 (stride 1), batch 16:
             device-event time and TF/s with flops = 2 * pixels * Cout * 16 * Cin per kernel

Every figure is a median of `--steps` fenced steps after `--warmup` steps.  Each child runs under its own `timeout`; the driver stops
at the first child that does not exit with status 0.

    python tools/bench_gan2d.py [--steps 20] [--warmup 5] [--reps 2] [--only step|kernels]
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
SHAPE = (16, 1, 256, 256)
AEKW = dict(spatial_dims=2, in_channels=1, out_channels=1, latent_channels=8, num_res_blocks=2, num_channels=[32, 64, 128],
            attention_levels=[False] * 3, norm_num_groups=16, with_encoder_nonlocal_attn=False, with_decoder_nonlocal_attn=False,
            downsample_parameters=[[1, 3, 1], [2, 3, 1], [2, 3, 1]], upsample_parameters=[[2, 3, 1], [2, 3, 1]])
DKW = dict(spatial_dims=2, num_channels=64, in_channels=1, out_channels=1, num_layers_d=3)
KLW, ADVW, LR = 1e-6, 0.01, 5e-5


def _fenced(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        loss = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(out), 3), ms_min=round(min(out), 3), ms_max=round(max(out), 3), loss=float(loss))


def _inputs():
    import torch
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    torch.manual_seed(0)
    ae = AutoencoderKL(**AEKW).cuda()
    x = torch.rand(SHAPE, device="cuda")
    with torch.no_grad():
        zshape = tuple(ae.encode(x[:1])[0].shape[1:])
    eps = torch.randn((SHAPE[0],) + zshape, device="cuda")
    return ae, x, eps


def child_step(path, steps, warmup):
    import torch
    from medical_image_generation_amd.trainer import AEGANTrainer, AETrainer
    ae, x, eps = _inputs()
    rec = dict(path=path, shape=list(SHAPE))
    if path == "native":
        from medical_image_generation_amd.discriminator import PatchDiscriminator
        d = PatchDiscriminator(**DKW).cuda()
        tr = AEGANTrainer(ae, d, adv_weight=ADVW, kl_weight=KLW, lr=LR, d_lr=LR)
        eager = _fenced(lambda: tr.step(x, eps), max(3, steps // 4), 2)
        rec.update(eager_step_ms=eager["ms"])
        tr.capture(x, eps)
        rec.update(_fenced(lambda: tr.step_graph(), steps, warmup))
        rec.update(gen_loss=float(tr.gen_loss), disc_loss=float(tr.disc_loss))
    else:
        from oracle import disc as odisc
        d = odisc.PatchDiscriminator(**DKW).cuda().train()
        adv = odisc.PatchAdversarialLoss()
        opt_d = torch.optim.Adam(d.parameters(), lr=LR)

        def extra(recon, images):  # T-AE:416-419
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = d(recon.contiguous().float())[-1]
            return adv(logits, True) * ADVW

        tr = AETrainer(ae, lr=LR, kl_weight=KLW, extra_loss=extra)

        def step():
            for p in d.parameters():  # T-AE:401-402
                p.requires_grad_(False)
            loss = tr.step(x, eps)
            for p in d.parameters():
                p.requires_grad_(True)
            opt_d.zero_grad(set_to_none=True)  # T-AE:371-397
            with torch.autocast("cuda", dtype=torch.bfloat16):
                lf = adv(d(tr.reconstruction.contiguous().detach())[-1], False)
                lr = adv(d(x.contiguous().detach())[-1], True)
                ld = (lf + lr) * 0.5 * ADVW
            ld.backward()
            torch.nn.utils.clip_grad_norm_(d.parameters(), 1.0)
            opt_d.step()
            return loss

        rec.update(_fenced(step, steps, warmup))
    print(json.dumps(rec), flush=True)


def child_profile():
    """GPU milliseconds per library entry point of ONE eager native step (device events around every call: _lib.profile_calls)."""
    from medical_image_generation_amd import _lib
    from medical_image_generation_amd.discriminator import PatchDiscriminator
    from medical_image_generation_amd.trainer import AEGANTrainer
    ae, x, eps = _inputs()
    tr = AEGANTrainer(ae, PatchDiscriminator(**DKW).cuda(), adv_weight=ADVW, kl_weight=KLW, lr=LR, d_lr=LR)
    for _ in range(3):
        tr.step(x, eps)
    with _lib.profile_calls() as prof:
        tr.step(x, eps)
    ms = prof.summary()
    calls = {}
    for name, _, _ in prof.records:
        calls[name] = calls.get(name, 0) + 1
    top = sorted(ms.items(), key=lambda kv: -kv[1])
    print(json.dumps(dict(path="profile", total_ms=round(sum(ms.values()), 3),
                          by_entry_point={k: [round(v, 3), calls[k]] for k, v in top if v >= 0.02})), flush=True)


def child_kernels(steps, warmup):
    import torch
    from medical_image_generation_amd._lib import call, call_raw, ptr
    bf16 = torch.bfloat16

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

    for n, cin, cout, h, w, s in ((16, 64, 128, 128, 128, 2), (16, 256, 512, 32, 32, 1)):
        ho, wo = (h - 2) // s + 1, (w - 2) // s + 1
        dims = (n, h, w, cin, cout, s)
        x = torch.randn(n, h, w, cin, device="cuda").to(bf16)
        dy = torch.randn(n, ho, wo, cout, device="cuda").to(bf16)
        wt = torch.randn(cout, cin, 4, 4, device="cuda") * 0.02
        wf, wd = torch.empty(cout, 16 * cin, dtype=bf16, device="cuda"), torch.empty(16 * cin * cout, dtype=bf16, device="cuda")
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        dw = torch.zeros_like(wt)
        splits = call_raw("mi_conv2d_k4_wgrad_splits", *dims)
        ws = torch.empty(splits * 16 * cin * cout, device="cuda")
        call("mi_conv2d_k4_pack", ptr(wt), ptr(wf), ptr(wd), cin, cout, s)
        flops = 2.0 * n * ho * wo * cout * 16 * cin
        runs = {
            "mi_conv2d_k4_fwd": lambda: call("mi_conv2d_k4_fwd", ptr(x), ptr(wf), ptr(y), *dims),
            "mi_conv2d_k4_dgrad": lambda: call("mi_conv2d_k4_dgrad", ptr(dy), ptr(wd), ptr(dx), *dims),
            "mi_conv2d_k4_wgrad (with its fold)": lambda: call("mi_conv2d_k4_wgrad", ptr(x), ptr(dy), ptr(dw), ptr(ws), *dims),
            "mi_conv2d_k4_pack": lambda: call("mi_conv2d_k4_pack", ptr(wt), ptr(wf), ptr(wd), cin, cout, s),
        }
        for name, fn in runs.items():
            ms = timed(fn)
            rec = dict(kernel=name, layer=f"{cin}->{cout} @{h}x{w} s{s} n{n}", us=round(ms * 1e3, 1))
            if "pack" not in name:
                rec.update(GFLOP=round(flops / 1e9, 2), TFps=round(flops / ms / 1e9, 1), splits=splits if "wgrad" in name else None)
            print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", choices=["step", "kernels"])
    ap.add_argument("--child", metavar="PATH")
    a = ap.parse_args()
    if a.steps < 20 or a.warmup < 5:
        ap.error("medians of >= 20 steps after >= 5 warm-up steps")
    if a.child:
        if a.child == "kernels":
            child_kernels(a.steps, a.warmup)
        elif a.child == "profile":
            child_profile()
        else:
            child_step(a.child, a.steps, a.warmup)
        return
    jobs = []
    if a.only != "kernels":
        jobs += ["native", "torch"] * a.reps + ["profile"]
    if a.only != "step":
        jobs += ["kernels"]
    for path in jobs:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--child", path]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(f"bench_gan2d: `{path}` exited with status {rc}; stopping here", file=sys.stderr, flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    main()
