"""Host side of FusedAdam (the torch.optim face of the fused optimizer) and of the GAN checkpoints: torch LR schedulers bind to it, its
device hyperparameter block follows the parameter group, its state_dict is torch.optim.Adam[W]'s (plus what a scheduler adds), and
a GAN trainer's checkpoint carries the discriminator in the layout train_autoencoder.py:533-553 writes.  CPU tensors stand in for the
device buffers; the GPU tests run the kernels (tests/test_lr_schedule_gpu.py)."""
import pytest
import torch

from oracle import cases, disc as odisc

DKW = dict(spatial_dims=3, num_channels=8, in_channels=1, out_channels=1, num_layers_d=3)
ADAMW_GROUP_KEYS = set(torch.optim.AdamW([torch.zeros(1, requires_grad=True)]).state_dict()["param_groups"][0])


def _fused(net, lr=1e-3, step=0, decoupled=True, max_grad_norm=1.0):
    from medical_image_generation_amd.optim import FusedAdam
    a = net.arena(torch.device("cpu"))
    n = a.n_trainable
    g = torch.Generator().manual_seed(0)
    m, v = torch.randn(n, generator=g), torch.rand(n, generator=g)
    return FusedAdam(net, a, m, v, torch.tensor([float(step)]), lr, (0.9, 0.999), 1e-8, 0.01 if decoupled else 0.0, decoupled, max_grad_norm)


def _same_state(a, b):
    """Equal torch-layout optimizer states (the flat buffers also hold alignment padding that belongs to no parameter)."""
    sa, sb = a.state_dict()["state"], b.state_dict()["state"]
    return set(sa) == set(sb) and all(torch.equal(sa[i][k], sb[i][k]) for i in sa for k in ("step", "exp_avg", "exp_avg_sq"))


def _unet():
    from medical_image_generation_amd.unet import DiffusionModelUNet
    return DiffusionModelUNet(**cases.UNET_CASES["unet_c1"]["kwargs"])


def test_scheduler_drives_the_device_block():
    opt = _fused(_unet(), lr=1e-3)
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 1
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.1, total_iters=3)
    want = [1e-3 * 0.1]
    for _ in range(4):
        opt.push()
        assert opt.hparams[0].item() == torch.tensor(opt.param_groups[0]["lr"], dtype=torch.float32).item()
        assert tuple(opt.hparams[1:6].tolist()) == tuple(torch.tensor([0.9, 0.999, 1e-8, 0.01, 1.0]).tolist())
        sched.step()
        want.append(sched.get_last_lr()[0])
    assert all(isinstance(x, float) for x in sched.get_last_lr()) and abs(want[-1] - 1e-3) < 1e-12
    opt.max_grad_norm = None  # no clipping: the block's max_norm reads 0
    opt.push()
    assert opt.hparams[5].item() == 0.0
    # the same schedule on torch.optim.AdamW gives the same Python floats
    p = torch.zeros(3, requires_grad=True)
    t = torch.optim.AdamW([p], lr=1e-3)
    ts = torch.optim.lr_scheduler.LinearLR(t, start_factor=0.1, total_iters=3)
    got = [t.param_groups[0]["lr"]]
    for _ in range(4):
        ts.step()
        got.append(ts.get_last_lr()[0])
    assert got == want


def test_one_group_only_and_float_lr():
    opt = _fused(_unet())
    with pytest.raises(ValueError, match="one parameter group"):
        opt.add_param_group({"params": [torch.zeros(1, requires_grad=True)]})
    opt.param_groups[0]["lr"] = torch.tensor(1e-3)
    with pytest.raises(TypeError):
        opt.push()


def test_state_dict_is_torch_layout_and_carries_initial_lr():
    net = _unet()
    opt = _fused(net, lr=2e-3, step=3)
    sd = opt.state_dict()
    assert set(sd["param_groups"][0]) == ADAMW_GROUP_KEYS  # no scheduler: exactly torch's keys
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.5, total_iters=4)
    sched.step()
    sd = opt.state_dict()
    assert set(sd["param_groups"][0]) == ADAMW_GROUP_KEYS | {"initial_lr"} and sd["param_groups"][0]["initial_lr"] == 2e-3
    # the reference's resume order (optimizer, scheduler, then their states) on torch.optim.AdamW
    t = torch.optim.AdamW(net.parameters(), lr=1.0)
    ts = torch.optim.lr_scheduler.LinearLR(t, start_factor=0.5, total_iters=4)
    t.load_state_dict(sd)
    ts.load_state_dict(sched.state_dict())
    ts.step(), sched.step()
    assert ts.get_last_lr() == sched.get_last_lr()
    # and back: a torch optimizer's state (with initial_lr) into a fresh FusedAdam, whose own scheduler then resumes
    fresh = _fused(net, lr=9.0)
    fs = torch.optim.lr_scheduler.LinearLR(fresh, start_factor=0.5, total_iters=4)
    fresh.load_state_dict(t.state_dict())
    fs.load_state_dict(ts.state_dict())
    assert fresh.param_groups[0]["lr"] == t.param_groups[0]["lr"] and fresh.param_groups[0]["initial_lr"] == 2e-3
    assert float(fresh.step_count) == 3.0 and _same_state(fresh, opt)
    fs.step(), ts.step()
    assert fs.get_last_lr() == ts.get_last_lr()


def test_trainer_hyperparameters_are_views_of_the_group():
    from medical_image_generation_amd.trainer import DDPMTrainer
    tr = DDPMTrainer(_unet(), lr=3e-4, optimizer="AdamW", max_grad_norm=1.0, device="cpu")
    assert tr.optimizer.param_groups[0]["lr"] == 3e-4 and tr.lr == 3e-4 and tr.weight_decay == 0.01
    torch.optim.lr_scheduler.LinearLR(tr.optimizer, start_factor=0.25, total_iters=2)
    assert tr.lr == 3e-4 * 0.25
    tr.lr, tr.betas, tr.eps, tr.max_grad_norm = 1e-5, (0.5, 0.9), 1e-6, 2.0
    g = tr.optimizer.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], tr.optimizer.max_grad_norm) == (1e-5, (0.5, 0.9), 1e-6, 2.0)


def _gan(d_lr=2e-4):
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    from medical_image_generation_amd.discriminator import PatchDiscriminator
    from medical_image_generation_amd.trainer import AEGANTrainer
    ae = AutoencoderKL(**cases.AEKL_CASES["aekl_c3a"]["kwargs"])
    return AEGANTrainer(ae, PatchDiscriminator(**DKW), d_lr=d_lr, lr=1e-4, device="cpu")


def test_gan_checkpoint_loads_into_torch_discriminator(tmp_path):
    """What save_model writes for a GAN trainer is what the reference's load_model (T-AE:566-588) reads: the discriminator loads
    strictly into the torch module, its optimizer state into torch.optim.Adam, its scheduler state into LinearLR."""
    from medical_image_generation_amd import checkpoint as ck
    tr = _gan()
    g = torch.Generator().manual_seed(1)
    for b in tr.D.buffers():  # BatchNorm statistics as a run leaves them
        b.copy_(b + (torch.randint(1, 9, b.shape, generator=g) if b.dtype == torch.long else torch.rand(b.shape, generator=g)))
    tr.d_exp_avg.copy_(torch.randn(tr.d_exp_avg.shape, generator=g))
    tr.d_exp_avg_sq.copy_(torch.rand(tr.d_exp_avg_sq.shape, generator=g))
    tr.d_step_count.fill_(5.0)
    gs = torch.optim.lr_scheduler.LinearLR(tr.optimizer, start_factor=0.5, total_iters=4)
    ds = torch.optim.lr_scheduler.LinearLR(tr.d_optimizer, start_factor=0.1, total_iters=4)
    ds.step()
    path = ck.save_model(tr, str(tmp_path), epoch=2, validation_loss=0.5, scheduler=gs, disc_scheduler=ds)
    ckpt = torch.load(path, weights_only=True)
    assert {"discriminator_state_dict", "disc_optimizer_state_dict", "disc_scheduler_state_dict", "scheduler_state_dict"} <= set(ckpt)
    ref = odisc.PatchDiscriminator(**DKW)
    ref.load_state_dict(ckpt["discriminator_state_dict"], strict=True)
    for (n, a), (_, b) in zip(ref.state_dict().items(), tr.D.state_dict().items()):
        assert torch.equal(a, b), n
    opt = torch.optim.Adam(ref.parameters(), lr=1.0)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.1, total_iters=4)
    opt.load_state_dict(ckpt["disc_optimizer_state_dict"])
    sched.load_state_dict(ckpt["disc_scheduler_state_dict"])
    assert opt.param_groups[0]["lr"] == tr.d_lr and opt.param_groups[0]["weight_decay"] == 0.0 and sched.last_epoch == 1
    names = [n for n, _ in ref.named_parameters()]
    for i, (n, p) in enumerate(ref.named_parameters()):
        st = opt.state[p]
        assert float(st["step"]) == 5.0 and torch.equal(st["exp_avg"], tr.d_arena.view(n, tr.d_exp_avg)), n
    assert len(names) == len(opt.state)
    # ... and the reverse: that torch state resumes on a fresh GAN trainer
    fresh = _gan(d_lr=7.0)
    fds = torch.optim.lr_scheduler.LinearLR(fresh.d_optimizer, start_factor=0.1, total_iters=4)
    assert ck.load_model(fresh, path, disc_scheduler=fds, for_training=True) == 3
    assert fresh.d_lr == tr.d_lr and fds.last_epoch == 1 and float(fresh.d_step_count) == 5.0
    assert _same_state(fresh.d_optimizer, tr.d_optimizer)
    for (n, a), (_, b) in zip(fresh.D.state_dict().items(), tr.D.state_dict().items()):
        assert torch.equal(a, b), n


def test_non_gan_checkpoint_keys_unchanged(tmp_path):
    from medical_image_generation_amd import checkpoint as ck
    from medical_image_generation_amd.trainer import DDPMTrainer
    tr = DDPMTrainer(_unet(), device="cpu")
    ckpt = torch.load(ck.save_model(tr, str(tmp_path), 0, 1.0, disc_scheduler=object()), weights_only=True)
    assert set(ckpt) == {"epoch", "network_state_dict", "optimizer_state_dict", "validation_loss"}


def test_replayed_step_counts_as_optimizer_step():
    """step(replay=graph) pushes the group, replays the graph and counts as optimizer.step() for the scheduler's order check."""
    import warnings
    opt = _fused(_unet(), lr=1e-3)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.5, total_iters=2)

    class Graph:
        calls = 0

        def replay(self):
            Graph.calls += 1

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for _ in range(2):
            opt.step(replay=Graph())
            sched.step()
    assert Graph.calls == 2 and opt.hparams[0].item() == torch.tensor(0.75e-3).item()
