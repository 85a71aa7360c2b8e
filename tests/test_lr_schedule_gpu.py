"""torch LR schedulers and checkpoints on the fused optimizer, eager and under hipGraph replay (train_ldm.py:124-130, 466-505, 551-553;
train_autoencoder.py:478-486, 533-591, 632-638): mi_adam_step_dev against mi_adam_step bit for bit, a captured step that follows a
schedule like torch.optim.AdamW does, a checkpoint loaded into an already-captured trainer, and GAN checkpoints that resume both
networks."""
import pytest
import torch

from oracle import cases, disc as odisc, nets, synth

pytestmark = pytest.mark.gpu
S = cases.SEED
dev = torch.device("cuda")
DKW = dict(spatial_dims=3, num_channels=16, in_channels=1, out_channels=1, num_layers_d=3)


@pytest.mark.parametrize("n", [10007, 4096])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("decoupled,wd", [(1, 0.01), (0, 0.1)])
def test_device_hparam_adam_is_bit_identical(n, grad_scale, clip, decoupled, wd):
    from medical_image_generation_amd._lib import call, ptr
    g = torch.Generator().manual_seed(3)
    p0, m0, v0 = torch.randn(n, generator=g), 0.01 * torch.randn(n, generator=g), 1e-4 * torch.rand(n, generator=g)
    grads = [(torch.randn(n, generator=g) * (3.0 if k == 0 else 0.01)).to(dev) for k in range(3)]
    lr, b1, b2, eps, max_norm = 1.5e-3, 0.85, 0.995, 1e-7, 1.0
    hp = torch.tensor([lr, b1, b2, eps, wd, max_norm, 0.0, 0.0], dtype=torch.float32, device=dev)
    state = [[t.clone().to(dev) for t in (p0, m0, v0)] + [torch.full((1,), 2.0, device=dev)] for _ in range(2)]
    sumsq = torch.zeros(1, device=dev)
    for gd in grads:
        if clip:
            call("mi_sumsq_f32", ptr(gd), n, ptr(sumsq), 0)
        (p, m, v, st), (pd, md, vd, std) = state
        call("mi_adam_step", ptr(p), ptr(gd), ptr(m), ptr(v), n, lr, b1, b2, eps, wd, decoupled, ptr(sumsq) if clip else None, max_norm,
             grad_scale, ptr(st))
        call("mi_adam_step_dev", ptr(pd), ptr(gd), ptr(md), ptr(vd), n, ptr(hp), decoupled, ptr(sumsq) if clip else None, grad_scale, ptr(std))
    torch.cuda.synchronize()
    (p, m, v, st), (pd, md, vd, std) = state
    assert float(st) == float(std) == 5.0
    assert not torch.equal(p.cpu(), p0)
    for a, b, what in ((p, pd, "param"), (m, md, "exp_avg"), (v, vd, "exp_avg_sq")):
        assert torch.equal(a, b), what


# ---------------------------------------------------------------------------------------------------------------- DDPM trainer
def _unet():
    from medical_image_generation_amd.unet import DiffusionModelUNet
    c = cases.UNET_CASES["unet3d"]
    ref = nets.DiffusionModelUNet(**c["kwargs"])
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    net = DiffusionModelUNet(**c["kwargs"])
    net.load_state_dict(sd)
    return c, net.cuda()


def _inputs(c, k):
    return (synth.ellipsoid_volume(S, "x0", c["shape"]).cuda(), synth.tensor(S, f"noise{k}", c["shape"]).cuda(),
            ((torch.tensor(c["timesteps"]) + 37 * k) % 1000).cuda())


def _trainable(tr):
    return [n for n, _, t in tr.model._entries if t]


def _params(tr, names):
    return torch.cat([tr.arena.view(n).detach().flatten() for n in names])


def test_captured_step_follows_linear_lr_like_torch_adamw():
    """capture(), then LinearLR on trainer.optimizer and 4 x (step_graph, scheduler.step()): the parameters track torch.optim.AdamW +
    clip_grad_norm_ + the same LinearLR on a copy, fed the trainer's own gradients.  A graph that kept the lr of capture time would
    be off by the schedule's factors."""
    from medical_image_generation_amd.trainer import DDPMTrainer
    c, net = _unet()
    tr = DDPMTrainer(net, lr=cases.STEP_LR, optimizer="AdamW", max_grad_norm=1.0)
    names = _trainable(tr)
    tr.capture(*_inputs(c, 0))
    ref = [tr.arena.view(n).detach().clone().requires_grad_(True) for n in names]
    opt = torch.optim.AdamW(ref, lr=cases.STEP_LR)
    sched_ref = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.1, total_iters=3)
    sched = torch.optim.lr_scheduler.LinearLR(tr.optimizer, start_factor=0.1, total_iters=3)
    for k in range(4):
        assert tr.lr == opt.param_groups[0]["lr"]
        tr.step_graph(*_inputs(c, k + 1))
        for n, p in zip(names, ref):
            p.grad = tr.arena.gview(n).detach().clone()
        torch.nn.utils.clip_grad_norm_(ref, 1.0)
        opt.step()
        sched.step(), sched_ref.step()
        hip, want = _params(tr, names), torch.cat([p.detach().flatten() for p in ref])
        e = float((hip - want).norm() / want.norm())
        print(f"\n[LinearLR under replay] step {k + 1} lr {opt.param_groups[0]['lr']:.3e}: parameter rel-L2 vs torch AdamW {e:.2e}")
        assert e <= 1e-6
    assert float(tr.step_count) == 4.0


def test_zero_lr_from_a_lambda_schedule_freezes_the_replay():
    from medical_image_generation_amd.trainer import DDPMTrainer
    c, net = _unet()
    tr = DDPMTrainer(net, lr=cases.STEP_LR, optimizer="AdamW", max_grad_norm=1.0)
    tr.capture(*_inputs(c, 0))
    sched = torch.optim.lr_scheduler.LambdaLR(tr.optimizer, lambda e: 1.0 if e == 0 else 0.0)
    p0 = tr.arena.data.clone()
    tr.step_graph()
    sched.step()
    p1 = tr.arena.data.clone()
    assert not torch.equal(p1, p0)
    tr.step_graph()
    torch.cuda.synchronize()
    assert torch.equal(tr.arena.data, p1) and float(tr.step_count) == 2.0
    tr.max_grad_norm = None  # the captured graph computes the clip norm: switching clipping off needs a new capture
    with pytest.raises(RuntimeError, match="capture again"):
        tr.step_graph()


def test_checkpoint_loaded_after_capture_drives_the_next_replay(tmp_path):
    """A checkpoint (another lr, non-zero moments) loaded into an already-captured trainer gives the same next update as the same file
    loaded into an eager one."""
    from medical_image_generation_amd import checkpoint as ck
    from medical_image_generation_amd.trainer import DDPMTrainer
    c, net = _unet()
    src = DDPMTrainer(net, lr=cases.STEP_LR, optimizer="AdamW", max_grad_norm=1.0)
    sched = torch.optim.lr_scheduler.LinearLR(src.optimizer, start_factor=0.5, total_iters=4)
    for k in range(2):
        src.step(*_inputs(c, k))
        sched.step()
    path = ck.save_model(src, str(tmp_path), epoch=1, validation_loss=0.5, scheduler=sched)
    lr_saved = src.lr
    ups = []
    for graph in (False, True):
        _, net2 = _unet()
        tr = DDPMTrainer(net2, lr=123.0, optimizer="AdamW", max_grad_norm=1.0)
        if graph:
            tr.capture(*_inputs(c, 5))
        s2 = torch.optim.lr_scheduler.LinearLR(tr.optimizer, start_factor=0.5, total_iters=4)
        assert ck.load_model(tr, path, lr_scheduler=s2, for_training=True) == 2
        assert tr.lr == lr_saved and s2.last_epoch == 2 and float(tr.step_count) == 2.0
        before = tr.arena.data.clone()
        tr.step_graph(*_inputs(c, 2)) if graph else tr.step(*_inputs(c, 2))
        torch.cuda.synchronize()
        ups.append((tr.arena.data - before)[:tr.arena.n_trainable].cpu())
    eager, replay = ups
    cos = float(torch.dot(eager, replay) / (eager.norm() * replay.norm()))
    ratio = float(replay.norm() / eager.norm())
    print(f"\n[load after capture] update cosine {cos:.5f}, norm ratio {ratio:.4f}")
    assert cos >= 0.99 and abs(ratio - 1) <= 0.02


# ---------------------------------------------------------------------------------------------------------------- GAN trainer
def _gan():
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    from medical_image_generation_amd.discriminator import PatchDiscriminator
    from medical_image_generation_amd.trainer import AEGANTrainer
    c = cases.AEKL_CASES["aekl_c3a"]
    ae_ref = nets.AutoencoderKL(**c["kwargs"])
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ae_ref.state_dict().items()}, S)
    ae = AutoencoderKL(**c["kwargs"])
    ae.load_state_dict(sd)
    d_ref = odisc.PatchDiscriminator(**DKW)
    dsd = {k: v.clone() for k, v in d_ref.state_dict().items()}
    g = torch.Generator().manual_seed(S)
    for k, v in dsd.items():
        if v.dtype.is_floating_point and "running" not in k:
            dsd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    d = PatchDiscriminator(**DKW)
    d.load_state_dict(dsd)
    x = synth.ellipsoid_volume(S, "x", (2, 1, 32, 32, 32))
    with torch.no_grad():
        zshape = tuple(ae_ref.encode(x)[0].shape)
    tr = AEGANTrainer(ae.cuda(), d.cuda(), adv_weight=0.5, kl_weight=1e-3, lr=cases.STEP_LR, d_lr=cases.STEP_LR, max_grad_norm=1.0)
    return tr, x.cuda(), [synth.tensor(S, f"eps{k}", zshape).cuda() for k in range(4)]


def _bn(tr):
    return [b.clone() for b in tr.D.buffers()]


def test_gan_schedules_freeze_one_network_under_replay():
    tr, x, eps = _gan()
    tr.step(x, eps[0])  # BatchNorm statistics away from their initial values
    bn = _bn(tr)
    tr.capture(x, eps[1])
    assert all(torch.equal(a, b) for a, b in zip(bn, tr.D.buffers())), "capture() moved the discriminator's BatchNorm buffers"
    g_s = torch.optim.lr_scheduler.LambdaLR(tr.optimizer, lambda e: 1.0 if e == 0 else 0.0)
    d_s = torch.optim.lr_scheduler.LambdaLR(tr.d_optimizer, lambda e: 0.0 if e == 0 else 1.0)
    assert tr.d_lr == 0.0 and tr.lr == cases.STEP_LR
    nd = tr.d_arena.n_trainable
    g0, d0 = tr.arena.data.clone(), tr.d_arena.data[:nd].clone()
    tr.step_graph(x, eps[2])
    torch.cuda.synchronize()
    assert torch.equal(tr.d_arena.data[:nd], d0) and not torch.equal(tr.arena.data, g0)
    assert float(tr.d_step_count) == 2.0 and float(tr.step_count) == 2.0
    g_s.step(), d_s.step()
    g1 = tr.arena.data.clone()
    tr.step_graph(x, eps[3])
    torch.cuda.synchronize()
    assert torch.equal(tr.arena.data, g1) and not torch.equal(tr.d_arena.data[:nd], d0)
    assert float(tr.d_step_count) == 3.0 and float(tr.step_count) == 3.0


def test_gan_checkpoint_resumes_both_networks(tmp_path):
    """2 steps, save_model, a fresh trainer, load_model, a 3rd step: the same 3rd step as the uninterrupted run (up to the float-atomics
    noise of two backward passes); the discriminator, its BatchNorm buffers, its Adam state and both schedulers round-trip, and the
    file loads into the torch discriminator."""
    from medical_image_generation_amd import checkpoint as ck
    tr, x, eps = _gan()
    g_s = torch.optim.lr_scheduler.LinearLR(tr.optimizer, start_factor=0.5, total_iters=4)
    d_s = torch.optim.lr_scheduler.LinearLR(tr.d_optimizer, start_factor=0.25, total_iters=4)
    for k in range(2):
        tr.step(x, eps[k])
        g_s.step(), d_s.step()
    path = ck.save_model(tr, str(tmp_path), epoch=1, validation_loss=0.5, scheduler=g_s, disc_scheduler=d_s)
    ckpt = torch.load(path, weights_only=True)
    ref = odisc.PatchDiscriminator(**DKW)
    ref.load_state_dict(ckpt["discriminator_state_dict"], strict=True)
    torch.optim.Adam(ref.parameters(), lr=1.0).load_state_dict(ckpt["disc_optimizer_state_dict"])

    fresh, _, _ = _gan()
    f_g = torch.optim.lr_scheduler.LinearLR(fresh.optimizer, start_factor=0.5, total_iters=4)
    f_d = torch.optim.lr_scheduler.LinearLR(fresh.d_optimizer, start_factor=0.25, total_iters=4)
    assert ck.load_model(fresh, path, lr_scheduler=f_g, disc_scheduler=f_d, for_training=True) == 2
    nd = tr.d_arena.n_trainable
    assert torch.equal(fresh.arena.data[:tr.arena.n_trainable], tr.arena.data[:tr.arena.n_trainable])
    assert torch.equal(fresh.d_arena.data[:nd], tr.d_arena.data[:nd])
    assert all(torch.equal(a, b) for a, b in zip(fresh.D.buffers(), tr.D.buffers()))
    assert float(fresh.d_step_count) == 2.0 and float(fresh.step_count) == 2.0
    sa, sb = fresh.d_optimizer.state_dict(), tr.d_optimizer.state_dict()
    assert all(torch.equal(sa["state"][i][k], sb["state"][i][k]) for i in sb["state"] for k in ("exp_avg", "exp_avg_sq"))
    assert f_g.last_epoch == g_s.last_epoch == 2 and f_d.last_epoch == 2 and fresh.lr == tr.lr and fresh.d_lr == tr.d_lr
    before_g, before_d = tr.arena.data.clone(), tr.d_arena.data[:nd].clone()
    tr.step(x, eps[2])
    fresh.step(x, eps[2])
    torch.cuda.synchronize()
    for what, a, b, b0 in (("generator", tr.arena.data, fresh.arena.data, before_g), ("discriminator", tr.d_arena.data[:nd], fresh.d_arena.data[:nd], before_d)):
        ua, ub = (a - b0).cpu(), (b - b0).cpu()
        cos = float(torch.dot(ua, ub) / (ua.norm() * ub.norm()))
        ratio = float(ub.norm() / ua.norm())
        print(f"\n[GAN resume] {what} 3rd-step update cosine {cos:.5f}, norm ratio {ratio:.4f}")
        assert cos >= 0.98 and abs(ratio - 1) <= 0.05
