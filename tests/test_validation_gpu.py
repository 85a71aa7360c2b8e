"""Native validation passes of the fused trainers (trainer.validate / capture_validate / validate_graph, ValidationMeter, the
mi_mse_eval / mi_l1_eval / mi_kl_eval reductions): the loop bodies of LDM.validate_epoch (train_ldm.py:193-239),
AutoEncoder.validate_one_epoch (train_autoencoder.py:438-467) and adapt_kl_loss_weight (train_autoencoder.py:295-328), against the
oracle's restatement of the same losses, against the training path of the same trainers and, kernel by kernel, against fp64 torch."""
import pytest
import torch

from oracle import cases, nets, step, synth

pytestmark = pytest.mark.gpu
S = cases.SEED


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def _unet(name, seed=S, kwargs=None):
    from medical_image_generation_amd.unet import DiffusionModelUNet
    kw = kwargs or cases.UNET_CASES[name]["kwargs"]
    ref = nets.DiffusionModelUNet(**kw)
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, seed)
    ref.load_state_dict(sd)
    net = DiffusionModelUNet(**kw)
    net.load_state_dict(sd)
    return ref, net.cuda()


def _ae(name="aekl_c3a"):
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    c = cases.AEKL_CASES[name]
    ref = nets.AutoencoderKL(**c["kwargs"])
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    ref.load_state_dict(sd)
    net = AutoencoderKL(**c["kwargs"])
    net.load_state_dict(sd)
    return c, ref, net.cuda()


# ------------------------------------------------------------------------------------------------ trainer cases
# name -> (trainer, validate inputs on the GPU, oracle loss as a callable, tolerance against the oracle).  The tolerances are the ones
# tests/test_trainer_gpu.py applies to the SAME trainer's training loss against the SAME oracle (the forward is the same bf16 network):
# 1e-2 for the DDPM trainers, 1.5e-2 for the LDM trainer (test_ldm_step_matches_oracle_composition), 2e-2 for the autoencoder
# (test_ae_three_train_steps).
def _ddpm_case(name, prediction_type="epsilon"):
    from medical_image_generation_amd.trainer import DDPMSchedule, DDPMTrainer
    sched = step.DDPMSchedule(prediction_type=prediction_type)
    cond = labels = context = None
    if name == "unet_c5":  # the concat-conditioned case of test_concat_conditioned_step_matches_oracle: batch 2, 8 + 1 channels at 12^3
        shape, t = (2, 8, 12, 12, 12), torch.tensor([42, 873])
        x0 = synth.tensor(S, "latents", shape)
        cond = (synth.ellipsoid_volume(S, "label", (2, 1, 12, 12, 12)) > 0).float()
    else:
        c = cases.UNET_CASES[name]
        shape, t = c["shape"], torch.tensor(c["timesteps"])
        x0 = synth.ellipsoid_volume(S, "x0", shape)
        labels = torch.tensor(c["class_labels"]) if "class_labels" in c else None
        context = synth.tensor(S, "context", c["context"]) if "context" in c else None
    noise = synth.tensor(S, "noise0", shape)
    ref, net = _unet(name)
    tr = DDPMTrainer(net, lr=cases.STEP_LR, schedule=DDPMSchedule(prediction_type=prediction_type))

    def oracle():
        with torch.no_grad():
            if labels is None and context is None:
                return float(step.ddpm_loss(ref, sched, x0, noise, t, condition=cond)[0])
            noisy = sched.add_noise(x0, noise, t)  # ddpm_loss has no class_labels / context arguments: the same three lines
            pred = ref(noisy, t, context=context, class_labels=labels)
            return float(torch.nn.functional.mse_loss(pred.float(), noise.float()))

    dev = lambda v: None if v is None else v.cuda()  # noqa: E731
    return tr, (x0.cuda(), noise.cuda(), t.cuda(), dev(labels), dev(context), dev(cond)), oracle, 1e-2


def _ldm_case():
    from medical_image_generation_amd.trainer import LDMTrainer
    _, ae_ref, ae = _ae("aekl_c3a")
    u_ref, unet = _unet("unet_ldm", seed=S + 1)
    x = synth.ellipsoid_volume(S, "x", (2, 1, 32, 32, 32))
    with torch.no_grad():
        mu, sigma = ae_ref.encode(x)
    eps, noise = synth.tensor(S, "eps", mu.shape), synth.tensor(S, "lnoise", mu.shape)
    t = torch.tensor([250, 750])
    with torch.no_grad():
        z = mu + eps * sigma
    scale = float(1 / torch.std(z))
    tr = LDMTrainer(unet, ae, scale_factor=scale, lr=1e-4)

    def oracle():  # encoder -> scale -> ddpm_loss (train_ldm.py:206-229)
        with torch.no_grad():
            return float(step.ddpm_loss(u_ref, step.DDPMSchedule(), z * scale, noise, t)[0])

    return tr, (x.cuda(), eps.cuda(), noise.cuda(), t.cuda()), oracle, 1.5e-2


def _ae_case(trainer="ae"):
    from medical_image_generation_amd.trainer import AEGANTrainer, AETrainer
    c, ref, net = _ae("aekl_c3a")
    x = synth.ellipsoid_volume(S, "x", c["shape"])
    with torch.no_grad():
        zshape = tuple(ref.encode(x)[0].shape)
    eps = synth.tensor(S, "eps0", zshape)
    if trainer == "ae":
        tr = AETrainer(net, lr=cases.STEP_LR, kl_weight=0.0)  # kl_weight = 0, no perceptual term: the training loss is the L1 term alone
    else:
        from medical_image_generation_amd.discriminator import PatchDiscriminator
        torch.manual_seed(0)
        tr = AEGANTrainer(net, PatchDiscriminator(spatial_dims=3, num_channels=8, in_channels=1).cuda(), lr=cases.STEP_LR, adversarial=True)

    def oracle():  # ae_loss(..., kl_weight=0) is the L1 term alone (train_autoencoder.py:447-456)
        with torch.no_grad():
            return float(step.ae_loss(ref, x, eps, 0.0)[0])

    return tr, (x.cuda(), eps.cuda()), oracle, 2e-2


_CASES = {
    "unet3d_eps": lambda: _ddpm_case("unet3d"),
    "unet3d_vpred": lambda: _ddpm_case("unet3d", "v_prediction"),
    "c5_concat": lambda: _ddpm_case("unet_c5"),
    "unet2d_class": lambda: _ddpm_case("unet2d_class"),
    "unet2d_xattn": lambda: _ddpm_case("unet2d_xattn"),
    "ldm": _ldm_case,
    "ae_c3a": _ae_case,
}


@pytest.mark.parametrize("case", list(_CASES))
def test_validate_loss_matches_oracle(case):
    tr, args, oracle, tol = _CASES[case]()
    got, want = float(tr.validate(*args)), oracle()
    print(f"\n[validate vs oracle {case}] {got:.7f} vs {want:.7f}: rel {_rel(got, want):.3e} (tolerance {tol})")
    assert _rel(got, want) <= tol


@pytest.mark.parametrize("case", list(_CASES))
def test_validate_loss_equals_training_path_loss(case):
    """Same forward kernels; only the last reduction differs (fp64 fold instead of fp32 atomics): <= 1e-5 relative."""
    tr, args, _, _ = _CASES[case]()
    tr.forward_backward(*args)
    train = float(tr.loss)
    got = float(tr.validate(*args))
    print(f"\n[validate vs training path {case}] {got:.9f} vs {train:.9f}: rel {_rel(got, train):.3e}")
    assert float(tr.loss) == train  # (validate does not write self.loss)
    assert _rel(got, train) <= 1e-5


def test_kl_meter_matches_oracle():
    """adapt_kl_loss_weight's number (train_autoencoder.py:295-318): kl_meter.mean() against oracle.step.kl_loss(z_mu, z_sigma) of the
    fp32 oracle model.  There is no earlier bound for this value, so it is taken from the training path's own kernel: on the same bf16
    mu / sigma, mi_reparam_kl_fwd with kl_weight = 1 into a zeroed loss differs from the oracle by d_train (bf16 drift of the encoder);
    the new path is gated at 3 x d_train.  Measured on MI355X (aekl_c3a, 1 x 1 x 32^3): d_train 4.276e-3 (5108.2686 vs 5086.5200),
    new path 4.276e-3 (5108.2681): the two kernels agree to 8e-8."""
    from medical_image_generation_amd import engine as E
    from medical_image_generation_amd import hipops as ops
    from medical_image_generation_amd._lib import call, ptr
    from medical_image_generation_amd.trainer import ValidationMeter, kl_weight_from_mean
    tr, (x, eps), _, _ = _ae_case()
    c, ref, _ = _ae("aekl_c3a")
    with torch.no_grad():
        z_mu, z_sigma = ref.encode(x.cpu())
        want = float(step.kl_loss(z_mu, z_sigma))
    m = tr.model
    ctx = E.Ctx(tr.arena, m._plans, grad_enabled=False, prepacked=m.pack_all())
    mu, sigma = m._encode_run(ctx, ops.to_channels_last(x), need_dx=False)
    n, lc = mu.shape[0], mu.shape[-1]
    loss = torch.zeros(1, device="cuda")
    call("mi_reparam_kl_fwd", ptr(mu), ptr(sigma), ptr(eps), ptr(torch.empty_like(mu)), ptr(loss), n, lc, mu.numel() // (n * lc), 1.0)
    d_train = _rel(loss, want)
    meter, klm = ValidationMeter("cuda"), ValidationMeter("cuda")
    tr.validate(x, eps, meter=meter, kl_meter=klm)
    got = klm.mean()
    print(f"\n[kl meter] oracle {want:.6f}; training-path kernel {float(loss):.6f} (rel {d_train:.3e}); kl_meter {got:.6f} (rel {_rel(got, want):.3e})")
    assert d_train <= 2e-2  # (the reference point itself is sane: the AE's training loss tolerance)
    assert _rel(got, want) <= 3 * d_train
    assert kl_weight_from_mean(got) == kl_weight_from_mean(want)
    with pytest.raises(ValueError):
        tr.validate(x, eps, meter=meter, kl_meter=meter)  # one block cannot account two values


# ------------------------------------------------------------------------------------------------ kernels
def _operands(n, c, v, seed, offset=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    pred = torch.randn(n * v * c + offset, device="cuda", generator=g).to(torch.bfloat16)[offset:].view(n, v, c)
    target = torch.randn(n, c, v, device="cuda", generator=g)
    return pred, target


_SHAPES = [(1, 1, 1), (4, 8, 1), (3, 3, 7), (2, 3, 343), (4, 8, 343), (3, 1, 33 * 32 * 31), (2, 3, 33 * 32 * 31), (1, 8, 33 * 32 * 31),
           (1, 2, 4096), (2, 4, 4096), (1, 5, 4096), (1, 1, 128 ** 3), (4, 1, 128 ** 3), (2, 3, 128 ** 3), (1, 8, 128 ** 3)]


@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("n,c,v", _SHAPES)
def test_eval_kernels_against_fp64(kind, n, c, v):
    """fp32 sums over chains of 8, fp64 from there on: <= 1e-6 relative to fp64 torch on the bf16-rounded operands; a second run on the
    same data leaves a bit-identical block; the running sum and the count advance."""
    from medical_image_generation_amd._lib import call, ptr
    from medical_image_generation_amd.trainer import ValidationMeter
    pred, target = _operands(n, c, v, 7 * n + 3 * c + v % 1000)
    d = pred.permute(0, 2, 1).double() - target.double()
    want = float((d * d).mean() if kind == "mse" else d.abs().mean())
    m = ValidationMeter("cuda")
    blocks = []
    for _ in range(2):
        m.reset()
        call(f"mi_{kind}_eval", ptr(pred), ptr(target), ptr(m.acc), n, c, v)
        blocks.append(m.acc.clone())
    got = float(m.last)
    print(f"\n[mi_{kind}_eval N{n} C{c} V{v}] {got:.12e} vs {want:.12e}: rel {_rel(got, want):.2e}")
    assert _rel(got, want) <= 1e-6
    assert torch.equal(blocks[0], blocks[1])
    call(f"mi_{kind}_eval", ptr(pred), ptr(target), ptr(m.acc), n, c, v)
    assert float(m.acc[2]) == 2.0 and float(m.acc[1]) == 2 * got and m.mean() == got


@pytest.mark.parametrize("n,c,v", _SHAPES)
def test_kl_eval_kernel_against_fp64(n, c, v):
    from medical_image_generation_amd._lib import call, ptr
    from medical_image_generation_amd.trainer import ValidationMeter
    g = torch.Generator(device="cuda").manual_seed(11 * n + c + v % 1000)
    mu = torch.randn(n, v, c, device="cuda", generator=g).to(torch.bfloat16)
    sigma = torch.exp(0.5 * torch.randn(n, v, c, device="cuda", generator=g)).to(torch.bfloat16)
    md, sd = mu.double(), sigma.double()
    want = float(0.5 * (md * md + sd * sd - torch.log(sd * sd) - 1).sum() / n)
    m = ValidationMeter("cuda")
    blocks = []
    for _ in range(2):
        m.reset()
        call("mi_kl_eval", ptr(mu), ptr(sigma), ptr(m.acc), n, c, v)
        blocks.append(m.acc.clone())
    got = float(m.last)
    print(f"\n[mi_kl_eval N{n} C{c} V{v}] {got:.12e} vs {want:.12e}: rel {_rel(got, want):.2e}")
    assert _rel(got, want) <= 1e-6
    assert torch.equal(blocks[0], blocks[1])


def test_eval_kernels_unaligned_operands_and_bad_arguments():
    """Operands that do not start on a 16-byte boundary take the scalar path (same value); null pointers and empty shapes are refused."""
    from medical_image_generation_amd._lib import HipError, call, ptr
    from medical_image_generation_amd.trainer import ValidationMeter
    n, c, v = 2, 3, 4096
    pred, target = _operands(n, c, v, 5, offset=1)
    assert pred.data_ptr() % 16 != 0
    d = pred.permute(0, 2, 1).double() - target.double()
    m = ValidationMeter("cuda")
    call("mi_mse_eval", ptr(pred), ptr(target), ptr(m.acc), n, c, v)
    assert _rel(m.last, (d * d).mean()) <= 1e-6
    call("mi_l1_eval", ptr(pred), ptr(target), ptr(m.acc), n, c, v)
    assert _rel(m.last, d.abs().mean()) <= 1e-6
    sigma = (pred.abs() + 0.5).to(torch.bfloat16).flatten()[1:]
    mu = pred.flatten()[1:]
    md, sd = mu.double(), sigma.double()
    call("mi_kl_eval", ptr(mu), ptr(sigma), ptr(m.acc), 1, 1, mu.numel())
    assert _rel(m.last, 0.5 * (md * md + sd * sd - torch.log(sd * sd) - 1).sum()) <= 1e-6
    for bad in ((None, ptr(target), ptr(m.acc), n, c, v), (ptr(pred), ptr(target), None, n, c, v), (ptr(pred), ptr(target), ptr(m.acc), 0, c, v)):
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            call("mi_mse_eval", *bad)


# ------------------------------------------------------------------------------------------------ meter
def test_meter_accumulates_batches_eager_and_graph():
    from medical_image_generation_amd.trainer import ValidationMeter
    tr, (x0, _, t, *_), _, _ = _ddpm_case("unet3d")
    noises = [synth.tensor(S, f"vnoise{k}", tuple(x0.shape)).cuda() for k in range(5)]
    m = ValidationMeter("cuda")
    with pytest.raises(ValueError):
        m.mean()
    eager = [float(tr.validate(x0, nz, (t + 13 * k) % 1000, meter=m)) for k, nz in enumerate(noises)]
    assert len(set(eager)) == 5
    assert _rel(m.mean(), sum(eager) / 5) <= 1e-6
    m.reset()
    with pytest.raises(ValueError):
        m.mean()
    tr.capture_validate(x0, noises[0], t, meter=m)
    with pytest.raises(ValueError):
        m.mean()  # capturing (and its warm-up passes) accounted nothing
    graph = [float(tr.validate_graph(x0, nz, (t + 13 * k) % 1000, meter=m)) for k, nz in enumerate(noises)]
    assert _rel(m.mean(), sum(graph) / 5) <= 1e-6
    for a, b in zip(graph, eager):
        assert _rel(a, b) <= 1e-6
    with pytest.raises(ValueError):
        tr.validate_graph(meter=ValidationMeter("cuda"))  # only the captured meter
    # the default meter: validate() without meter= accounts into the trainer's own
    tr.validate(x0, noises[1], (t + 13) % 1000)
    assert _rel(tr._val_meter.mean(), eager[1]) <= 1e-6


# ------------------------------------------------------------------------------------------------ no side effects
def _training_state(tr):
    st = {"data": tr.arena.data, "grad": tr.arena.grad, "exp_avg": tr.exp_avg, "exp_avg_sq": tr.exp_avg_sq, "step_count": tr.step_count,
          "loss": tr.loss, "_accum": tr._accum}
    for k in ("perc_loss", "reconstruction", "gen_loss", "disc_loss", "d_exp_avg", "d_exp_avg_sq", "d_step_count"):
        st[k] = getattr(tr, k, None)
    if hasattr(tr, "D"):
        st.update({"D." + k: v for k, v in tr.D.state_dict().items()})  # weights and running_mean / running_var / num_batches_tracked
        st["d_data"], st["d_grad"] = tr.d_arena.data, tr.d_arena.grad
    if hasattr(tr, "ae_arena"):
        st["ae_data"], st["ae_grad"] = tr.ae_arena.data, tr.ae_arena.grad
    return {k: v for k, v in st.items() if v is not None}


@pytest.mark.parametrize("case", ["ddpm_accumulate", "ldm", "ae", "aegan"])
def test_validation_leaves_training_state_bit_identical(case):
    if case == "ddpm_accumulate":  # two micro-steps (one optimizer step: moments non-zero), then a third: the middle of a cycle
        from medical_image_generation_amd.trainer import DDPMTrainer
        _, net = _unet("unet3d")
        tr = DDPMTrainer(net, lr=cases.STEP_LR, grad_accumulate_step=2)
        _, args, _, _ = _ddpm_case("unet3d")
        for _ in range(3):
            tr.step(*args)
        assert tr._micro == 1 and tr._accum is not None and float(tr.step_count) == 1.0
    else:
        tr, args, _, _ = {"ldm": _ldm_case, "ae": _ae_case, "aegan": lambda: _ae_case("aegan")}[case]()
        tr.step(*args)
        assert float(tr.step_count) == 1.0
    torch.cuda.synchronize()
    state = _training_state(tr)
    if case == "aegan":
        assert any(k.endswith("running_mean") for k in state) and any(k.endswith("num_batches_tracked") for k in state)
        assert float(tr.d_step_count) == 1.0
    before = {k: v.clone() for k, v in state.items()}
    micro = tr._micro
    opts = dict(return_recon=True) if case in ("ae", "aegan") else {}
    for _ in range(2):
        tr.validate(*args, **opts)
    tr.capture_validate(*args, **opts)
    for _ in range(2):
        tr.validate_graph(*args)
    torch.cuda.synchronize()
    assert tr._micro == micro
    after = _training_state(tr)
    assert set(after) == set(before)
    for k in before:
        assert after[k].data_ptr() == state[k].data_ptr(), k  # not re-bound either
        assert torch.equal(after[k], before[k]), f"{case}: validation changed {k}"
    assert float(before["exp_avg"].abs().max()) > 0 and float(before["grad"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ graphs coexist
@pytest.mark.parametrize("order", ["train_first", "validate_first"])
def test_training_and_validation_graphs_coexist(order, golden):
    """capture() and capture_validate() at ANOTHER batch size on one trainer, in both orders, then alternating replays: the training
    losses still meet the tolerance of test_three_train_steps[unet3d-True] against the golden oracle losses, every validation loss
    equals the eager validate() on the same inputs and parameters."""
    from medical_image_generation_amd.trainer import DDPMTrainer
    g, meta = golden("unet3d_steps")
    c = cases.UNET_CASES["unet3d"]
    _, net = _unet("unet3d")
    tr = DDPMTrainer(net, lr=cases.STEP_LR, optimizer=meta["optimizer"], max_grad_norm=1.0)
    x0 = synth.ellipsoid_volume(S, "x0", c["shape"]).cuda()
    t = torch.tensor(c["timesteps"])
    noise = [synth.tensor(S, f"noise{k}", c["shape"]).cuda() for k in range(cases.STEP_COUNT)]
    vshape = (5,) + tuple(c["shape"][1:3]) + (24, 24)  # another batch size and another patch shape: new plans, a larger workspace
    vx = synth.ellipsoid_volume(S, "vx", vshape).cuda()
    vnoise = [synth.tensor(S, f"vnoise{k}", vshape).cuda() for k in range(cases.STEP_COUNT)]
    vt = torch.tensor([5, 250, 500, 750, 995]).cuda()
    if order == "train_first":
        tr.capture(x0, noise[0], t.cuda())
        tr.capture_validate(vx, vnoise[0], vt)
    else:
        tr.capture_validate(vx, vnoise[0], vt)
        tr.capture(x0, noise[0], t.cuda())
    import gc
    gc.collect()
    ref_losses = g["losses"].tolist()
    for k in range(cases.STEP_COUNT):
        loss = float(tr.step_graph(x0, noise[k], ((t + 37 * k) % 1000).cuda()))
        vg = float(tr.validate_graph(vx, vnoise[k], vt))
        ve = float(tr.validate(vx, vnoise[k], vt))
        print(f"\n[coexist {order} step {k}] train {loss:.6f} vs {ref_losses[k]:.6f}; validate graph {vg:.7f} eager {ve:.7f} (rel {_rel(vg, ve):.2e})")
        assert abs(loss - ref_losses[k]) <= 1e-2 * abs(ref_losses[k])
        assert _rel(vg, ve) <= 1e-6


# ------------------------------------------------------------------------------------------------ memory
@pytest.mark.parametrize("case", ["unet3d_32", "ae_c3a"])
def test_validate_peak_memory_below_forward_backward(case):
    """No tape is kept: the peak of one eager validate() is strictly below the peak of one forward_backward() at the same shape (after
    a warm-up call of each, so plans and workspaces exist)."""
    if case == "unet3d_32":
        from medical_image_generation_amd.trainer import DDPMTrainer
        _, net = _unet("unet3d")
        tr = DDPMTrainer(net, lr=cases.STEP_LR)
        shape = (2, 1, 32, 32, 32)
        args = (synth.ellipsoid_volume(S, "x0", shape).cuda(), synth.tensor(S, "noise0", shape).cuda(), torch.tensor([100, 800]).cuda())
    else:
        tr, args, _, _ = _ae_case()
    peaks = {}
    for name, fn in (("validate", tr.validate), ("forward_backward", tr.forward_backward)):
        fn(*args)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn(*args)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
    print(f"\n[peak memory above the resident state, {case}] validate {peaks['validate'] / 2**20:.1f} MiB, forward_backward "
          f"{peaks['forward_backward'] / 2**20:.1f} MiB (ratio {peaks['validate'] / peaks['forward_backward']:.3f})")
    assert 0 < peaks["validate"] < peaks["forward_backward"]


# ------------------------------------------------------------------------------------------------ return_recon
def test_return_recon_equals_module_forward():
    """validate(..., return_recon=True) hands back what the module's own no-grad forward gives for the same eps (encode -> z = mu + eps *
    sigma -> decode): fp32 NCDHW, equal bit for bit or to one bf16 ulp (the module forms z in fp32 torch, the trainer in one fused
    kernel)."""
    tr, (x, eps), _, _ = _ae_case()
    loss, recon = tr.validate(x, eps, return_recon=True)
    with torch.no_grad():
        mu, sigma = tr.model.encode(x)
        want = tr.model.decode(mu + eps * sigma)
    assert recon.dtype == torch.float32 and recon.shape == x.shape and recon.is_contiguous()
    ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want)[1] - 8)  # |x| in [2^(e-1), 2^e): 8 significant bits -> ulp 2^(e-8)
    worst = float(((recon - want).abs() / ulp).max())
    print(f"\n[return_recon] max difference {worst:.3f} bf16 ulp; bit-equal: {torch.equal(recon, want)}")
    assert worst <= 1.0
    assert _rel(loss, torch.nn.functional.l1_loss(recon.double(), x.double())) <= 1e-6
    # the graph form returns the reconstruction in a static buffer
    tr.capture_validate(x, eps, return_recon=True)
    loss_g, recon_g = tr.validate_graph(x, eps)
    assert torch.equal(recon_g, recon) and _rel(loss_g, loss) <= 1e-6
