"""Averaged weights on the GPU: the shadow update fused into the Adam launch (mi_adam_ema_step_dev) against mi_adam_step_dev bit for bit
and against the fp64 recurrence, the in-place exchange (mi_swap_f32), and the trainers' use of both -- eager, under hipGraph replay with
a decay changed between replays, under gradient accumulation, inside `ema_weights()` (validation, sampling, refusals) and through
checkpoints.

The recurrence is always evaluated in fp64 over the parameters the code under test itself produced (never against a twin trainer:
k_sumsq accumulates with float atomics, so two runs need not agree in the last bit), with the decay as the fp32 value the device
block holds.  Bound, elementwise: |e - ref| <= 6 K M 2^-24 for K steps and M = max(|p|_inf, |e0|_inf): one step rounds three times in
fp32 (p - e, the product, the sum), each by at most M 2^-24 while 1 - d <= 0.5 (|p - e| <= 2M); doubled for the fp32 evaluation of the
warm-up ratio; and errors do not grow from step to step because d <= 1."""
import functools

import pytest
import torch

from oracle import cases, nets, synth

pytestmark = pytest.mark.gpu
S = cases.SEED
dev = torch.device("cuda")
U = 2.0 ** -24


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _decay(decay, warmup, t):
    """d of the step whose incremented count is t, in fp64 from the fp32 hyperparameter."""
    d = _f32(decay)
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def _recur(e, p, d):
    e = e.double()
    return e + (1.0 - d) * (p.double() - e)


def _check(e, ref, k, m, what=""):
    err = float((e.double() - ref).abs().max())
    bound = 6 * k * m * U
    print(f"\n[ema {what}] K {k} M {m:.3f}: max |e - ref| {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


# ---------------------------------------------------------------------------------------------------------------- kernels
@functools.lru_cache(maxsize=None)
def _kernel_inputs(n):
    """The inputs of test_device_hparam_adam_is_bit_identical (tests/test_lr_schedule_gpu.py), then a shadow away from the parameters."""
    g = torch.Generator().manual_seed(3)
    p0, m0, v0 = torch.randn(n, generator=g), 0.01 * torch.randn(n, generator=g), 1e-4 * torch.rand(n, generator=g)
    grads = [(torch.randn(n, generator=g) * (3.0 if k == 0 else 0.01)).to(dev) for k in range(3)]
    e0 = p0 + 0.5 * torch.randn(n, generator=g)
    return p0.to(dev), m0.to(dev), v0.to(dev), grads, e0.to(dev)


@pytest.mark.parametrize("start", [0, 2])
@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("decay", [0.5, 0.9999])
@pytest.mark.parametrize("decoupled,wd", [(1, 0.01), (0, 0.1)])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("n", [4096, 10007, 2 * 4096 * 256 + 5])  # the last: every thread loops twice and the end is ragged
def test_fused_shadow_update(n, clip, decoupled, wd, decay, warmup, start):
    from medical_image_generation_amd._lib import call, ptr
    p0, m0, v0, grads, e0 = _kernel_inputs(n)
    lr, b1, b2, eps, max_norm, grad_scale = 1.5e-3, 0.85, 0.995, 1e-7, 1.0, 0.5
    hp = torch.tensor([lr, b1, b2, eps, wd, max_norm, decay, float(warmup)], dtype=torch.float32, device=dev)
    old, new = ([t.clone() for t in (p0, m0, v0)] + [torch.full((1,), float(start), device=dev)] for _ in range(2))
    e = e0.clone()
    sumsq = torch.zeros(1, device=dev)
    ref, m_inf = e0.double(), float(e0.abs().max())
    for k, gd in enumerate(grads):
        if clip:
            call("mi_sumsq_f32", ptr(gd), n, ptr(sumsq), 0)
        sq = ptr(sumsq) if clip else None
        call("mi_adam_step_dev", ptr(old[0]), ptr(gd), ptr(old[1]), ptr(old[2]), n, ptr(hp), decoupled, sq, grad_scale, ptr(old[3]))
        call("mi_adam_ema_step_dev", ptr(new[0]), ptr(gd), ptr(new[1]), ptr(new[2]), ptr(e), n, ptr(hp), decoupled, sq, grad_scale, ptr(new[3]))
        ref = _recur(ref, new[0], _decay(decay, warmup, start + k + 1))
        m_inf = max(m_inf, float(new[0].abs().max()))
    torch.cuda.synchronize()
    assert float(old[3]) == float(new[3]) == start + 3.0
    assert not torch.equal(new[0], p0)
    for a, b, what in zip(old[:3], new[:3], ("param", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), what
    assert not torch.equal(e, e0) and not torch.equal(e, new[0])
    _check(e, ref, 3, m_inf, f"kernel n={n} decay={decay} warmup={warmup} start={start}")


@pytest.mark.parametrize("n", [4, 10007])
def test_swap_exchanges_in_place(n):
    from medical_image_generation_amd._lib import HipError, call, ptr
    g = torch.Generator().manual_seed(5)
    a0, b0 = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    a0[0], b0[-1] = float("nan"), -0.0  # bit for bit: payloads and signed zeros travel too
    # fenced: one float more on either side would show
    fa, fb = torch.full((n + 8,), 7.0, device=dev), torch.full((n + 8,), 9.0, device=dev)
    a, b = fa[4:4 + n], fb[4:4 + n]
    a.copy_(a0), b.copy_(b0)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    call("mi_swap_f32", ptr(a), ptr(b), n)
    assert torch.equal(bits(a), bits(b0)) and torch.equal(bits(b), bits(a0))
    call("mi_swap_f32", ptr(a), ptr(b), n)
    assert torch.equal(bits(a), bits(a0)) and torch.equal(bits(b), bits(b0))
    assert float(fa[:4].min()) == float(fa[-4:].max()) == 7.0 and float(fb[:4].min()) == float(fb[-4:].max()) == 9.0
    for x, y in ((fa[5:], b), (a, fb[5:])):
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            call("mi_swap_f32", ptr(x), ptr(y), 3)


# ---------------------------------------------------------------------------------------------------------------- DDPM trainer
def _unet(kwargs=None):
    from medical_image_generation_amd.unet import DiffusionModelUNet
    c = cases.UNET_CASES["unet3d"]
    kw = kwargs or c["kwargs"]
    ref = nets.DiffusionModelUNet(**kw)
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    net = DiffusionModelUNet(**kw)
    net.load_state_dict(sd)
    return c, net.cuda()


def _inputs(c, k):
    return (synth.ellipsoid_volume(S, "x0", c["shape"]).cuda(), synth.tensor(S, f"noise{k}", c["shape"]).cuda(),
            ((torch.tensor(c["timesteps"]) + 37 * k) % 1000).cuda())


def _ddpm(**kw):
    from medical_image_generation_amd.trainer import DDPMTrainer
    c, net = _unet()
    return c, DDPMTrainer(net, lr=cases.STEP_LR, optimizer="AdamW", max_grad_norm=1.0, **kw)


def _p(tr):
    return tr.arena.data[:tr.arena.n_trainable].clone()


class _Follow:
    """The fp64 recurrence next to a trainer: after(d) advances it with the trainer's current parameters and checks the shadow."""

    def __init__(self, tr, what):
        self.tr, self.what, self.k = tr, what, 0
        self.ref = tr.ema.double()
        self.m = float(tr.ema.abs().max())

    def after(self, decay):
        p = _p(self.tr)
        self.k += 1
        self.ref = _recur(self.ref, p, _decay(decay, False, self.k))
        self.m = max(self.m, float(p.abs().max()))
        _check(self.tr.ema, self.ref, self.k, self.m, f"{self.what} step {self.k}")


def test_eager_steps_move_the_shadow():
    c, tr = _ddpm(ema_decay=0.5)
    n = tr.arena.n_trainable
    assert tr.ema_decay == 0.5 and tr.ema.shape == (n,) and torch.equal(tr.ema, tr.arena.data[:n])
    e0, f = tr.ema.clone(), _Follow(tr, "eager")
    for k in range(3):
        tr.step(*_inputs(c, k))
        f.after(0.5)
    assert not torch.equal(tr.ema, e0) and not torch.equal(tr.ema, tr.arena.data[:n])


def test_replayed_graph_follows_a_changed_decay():
    c, tr = _ddpm(ema_decay=0.5)
    tr.capture(*_inputs(c, 0))
    f = _Follow(tr, "graph")
    assert torch.equal(tr.ema, tr.arena.data[:tr.arena.n_trainable])  # capture() itself does not run the optimizer
    for k in range(4):
        if k == 2:
            tr.ema_decay = 0.9
        tr.step_graph(*_inputs(c, k + 1))
        f.after(0.5 if k < 2 else 0.9)
    assert float(tr.step_count) == 4.0


def test_shadow_moves_on_boundary_micro_steps_only():
    c, tr = _ddpm(ema_decay=0.5, grad_accumulate_step=2)
    f = _Follow(tr, "accumulate")
    for k in range(4):
        before = tr.ema.clone()
        tr.step(*_inputs(c, k))
        if k % 2 == 0:
            assert torch.equal(tr.ema, before), f"micro-step {k + 1} moved the shadow"
        else:
            f.after(0.5)
    assert float(tr.step_count) == 2.0


def test_ema_weights_context():
    from medical_image_generation_amd.inferer import DDPMScheduler, DiffusionInferer
    from medical_image_generation_amd.trainer import DDPMTrainer
    c, tr = _ddpm(ema_decay=0.5)
    a, n = tr.arena, tr.arena.n_trainable
    assert a.numel > n, "unet3d has statically unused tensors behind the trainable prefix"
    for k in range(3):
        tr.step(*_inputs(c, k))
    tr.capture(*_inputs(c, 3))
    val = _inputs(c, 7)
    p0, e0, tail0 = _p(tr), tr.ema.clone(), a.data[n:].clone()
    assert not torch.equal(p0, e0)

    # the reference loss: a fresh network holding ema_state_dict(), validated twice (the forward's own run-to-run spread)
    _, fresh_net = _unet()
    fresh_net.load_state_dict(tr.ema_state_dict())
    fresh = DDPMTrainer(fresh_net, lr=cases.STEP_LR)
    want, again = float(fresh.validate(*val)), float(fresh.validate(*val))
    tol = max(1e-6, 10 * abs(want - again) / abs(want))
    raw = float(tr.validate(*val))

    sch = DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205)
    sch.set_timesteps(2)
    x0 = synth.tensor(S, "sample_noise", c["shape"]).cuda()
    zs = [synth.tensor(S, f"sample_z{i}", c["shape"]).cuda() for i in range(2)]
    sample = lambda: DiffusionInferer(sch).sample(x0, tr.model, sch, verbose=False, noises=zs, use_graph=False)  # noqa: E731
    outside = sample()

    with tr.ema_weights() as inside:
        assert inside is tr
        assert torch.equal(a.data[:n], e0) and torch.equal(tr.ema, p0) and torch.equal(a.data[n:], tail0)
        got = float(tr.validate(*val))
        averaged = sample()
        sd = {k: v.detach().cpu() for k, v in tr.model.state_dict().items()}
        for call_, name in ((lambda: tr.step(*val), "step"), (lambda: tr.step_graph(*val), "step_graph"), (tr.optimizer_step, "optimizer_step"),
                            (lambda: tr.capture(*val), "capture"), (lambda: tr.ema_weights().__enter__(), "ema_weights")):
            with pytest.raises(RuntimeError, match="ema_weights"):
                call_()
        assert torch.equal(a.data[:n], e0) and torch.equal(tr.ema, p0), "a refused call moved a buffer"
    torch.cuda.synchronize()
    assert torch.equal(a.data[:n], p0) and torch.equal(tr.ema, e0) and torch.equal(a.data[n:], tail0)
    want_sd = tr.ema_state_dict()
    assert all(torch.equal(sd[k], want_sd[k]) for k in want_sd), "state_dict() inside the context is ema_state_dict()"

    print(f"\n[ema_weights] validate: averaged {got:.8f} fresh {want:.8f} (again {again:.8f}, tol {tol:.1e}), raw {raw:.8f}")
    assert abs(raw - want) / abs(want) >= 100 * tol, "the inputs do not separate raw from averaged weights: raise the step count or lr"
    assert abs(got - want) / abs(want) <= tol
    assert torch.isfinite(averaged).all() and averaged.shape == outside.shape and not torch.equal(averaged, outside)

    class Boom(Exception):
        pass

    with pytest.raises(Boom):
        with tr.ema_weights():
            raise Boom
    assert torch.equal(a.data[:n], p0) and torch.equal(tr.ema, e0)
    tr.step_graph(*_inputs(c, 4))  # training goes on after the context
    assert not torch.equal(a.data[:n], p0)

    tr.model.float().cuda()  # _apply: the arena is rebuilt lazily, the shadow belongs to the old buffers
    tr.model.arena(tr.device)
    with pytest.raises(RuntimeError, match="rebuilt"):
        with tr.ema_weights():
            pass


def test_load_model_is_refused_inside_the_context(tmp_path):
    from medical_image_generation_amd import checkpoint as ck
    c, tr = _ddpm(ema_decay=0.5)
    path = ck.save_model(tr, str(tmp_path), epoch=0, validation_loss=1.0)
    with tr.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            ck.load_model(tr, path)


# ---------------------------------------------------------------------------------------------------------------- checkpoints
PLAIN_KEYS = {"epoch", "network_state_dict", "optimizer_state_dict", "validation_loss"}


def test_checkpoints_carry_the_shadow(tmp_path):
    from medical_image_generation_amd import checkpoint as ck
    c, src = _ddpm(ema_decay=0.5)
    for k in range(2):
        src.step(*_inputs(c, k))
    path = ck.save_model(src, str(tmp_path / "shadow"), epoch=1, validation_loss=0.5)
    ckpt = torch.load(path, weights_only=True)
    assert set(ckpt) == PLAIN_KEYS | {"ema_state_dict", "ema_decay"} and ckpt["ema_decay"] == 0.5
    net_sd, ema_sd = ckpt["network_state_dict"], ckpt["ema_state_dict"]
    assert list(ema_sd) == list(net_sd) and all(ema_sd[k].shape == net_sd[k].shape for k in net_sd)
    assert any(not torch.equal(ema_sd[k], net_sd[k]) for k in net_sd)

    _, plain = _ddpm()
    plain.step(*_inputs(c, 5))
    plain_path = ck.save_model(plain, str(tmp_path / "plain"), epoch=0, validation_loss=0.7)
    assert set(torch.load(plain_path, weights_only=True)) == PLAIN_KEYS
    plain_p = _p(plain)
    assert ck.load_model(plain, path, for_training=True) == 2  # the extra keys are ignored
    assert plain.ema is None and torch.equal(_p(plain), _p(src))

    for captured in (False, True):
        _, tr = _ddpm(ema_decay=0.9)
        if captured:
            tr.capture(*_inputs(c, 6))
        held = tr.ema
        ck.load_model(tr, path)
        assert tr.ema is held and torch.equal(tr.ema, src.ema) and torch.equal(_p(tr), _p(src)) and tr.ema_decay == 0.9
        if captured:
            f = _Follow(tr, "load after capture")
            tr.step_graph(*_inputs(c, 2))
            f.after(0.9)
            assert float(tr.step_count) == 3.0
        else:
            ck.load_model(tr, plain_path)  # no shadow in the file: the average restarts at the loaded parameters
            assert torch.equal(_p(tr), plain_p) and torch.equal(tr.ema, plain_p)


# ---------------------------------------------------------------------------------------------------------------- the other trainers
def _ae():
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    name = min(cases.AEKL_CASES, key=lambda k: sum(v.numel() for v in nets.AutoencoderKL(**cases.AEKL_CASES[k]["kwargs"]).state_dict().values()))
    c = cases.AEKL_CASES[name]
    ref = nets.AutoencoderKL(**c["kwargs"])
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    net = AutoencoderKL(**c["kwargs"])
    net.load_state_dict(sd)
    return c, ref, net.cuda()


def _ae_inputs(ref, shape, count):
    x = synth.ellipsoid_volume(S, "x", shape)
    with torch.no_grad():
        zshape = tuple(ref.encode(x)[0].shape)
    return x.cuda(), [synth.tensor(S, f"eps{k}", zshape).cuda() for k in range(count)], zshape


def test_autoencoder_trainer_keeps_a_shadow():
    from medical_image_generation_amd.trainer import AETrainer
    c, ref, net = _ae()
    x, eps, _ = _ae_inputs(ref, c["shape"], 2)
    tr = AETrainer(net, lr=cases.STEP_LR, kl_weight=1e-3, ema_decay=0.5)
    f = _Follow(tr, "AETrainer")
    for k in range(2):
        tr.step(x, eps[k])
        f.after(0.5)
    assert not torch.equal(tr.ema, _p(tr))


def test_gan_trainer_averages_the_autoencoder_only():
    from medical_image_generation_amd.discriminator import PatchDiscriminator
    from medical_image_generation_amd.trainer import AEGANTrainer
    c, ref, net = _ae()
    # 16^3: one stride-2 layer of the discriminator (k4) leaves 8 -> 7 -> 6 voxels per axis for its two stride-1 layers
    x, eps, _ = _ae_inputs(ref, (1, 1, 16, 16, 16), 2)
    torch.manual_seed(0)
    d = PatchDiscriminator(spatial_dims=3, num_channels=16, in_channels=1, num_layers_d=1).cuda()
    tr = AEGANTrainer(net, d, adv_weight=0.5, kl_weight=1e-3, lr=cases.STEP_LR, d_lr=cases.STEP_LR, ema_decay=0.5)
    assert tr.d_optimizer.ema is None and tr.optimizer.ema is tr.ema
    f = _Follow(tr, "AEGANTrainer")
    d0 = tr.d_arena.data.clone()
    for k in range(2):
        tr.step(x, eps[k])
        f.after(0.5)
    assert not torch.equal(tr.d_arena.data, d0) and float(tr.d_step_count) == 2.0


def test_latent_diffusion_trainer_keeps_a_shadow():
    from medical_image_generation_amd.trainer import LDMTrainer
    c, ref, ae = _ae()
    # unet3d on the autoencoder's latent channels; 32 x 32 x 8 voxels give a 16 x 16 x 8 latent, so the UNet's coarsest level (4 x 4 x 2)
    # still has more than one voxel per axis
    lc = c["kwargs"]["latent_channels"]
    _, unet = _unet(dict(cases.UNET_CASES["unet3d"]["kwargs"], in_channels=lc, out_channels=lc))
    x, eps, zshape = _ae_inputs(ref, (1, 1, 32, 32, 8), 2)
    tr = LDMTrainer(unet, ae, scale_factor=0.8, lr=cases.STEP_LR, ema_decay=0.5)
    ae0 = tr.ae_arena.data.clone()
    f = _Follow(tr, "LDMTrainer")
    for k in range(2):
        tr.step(x, eps[k], synth.tensor(S, f"lnoise{k}", zshape).cuda(), torch.tensor([250 + 400 * k]).cuda())
        f.after(0.5)
    assert torch.equal(tr.ae_arena.data, ae0) and not torch.equal(tr.ema, _p(tr))
