"""Reverse-diffusion sampling (medical_image_generation_amd/inferer.py) against the CPU restatement: the fused update kernel against
DDPMSchedule.step (oracle/step.py; third-party closed form, parity unpinned -- see its docstring), and the whole sample loop
(UNet forward + update, hipGraph-replayed) against the same loop on the oracle's UNet with the per-step noise pinned."""
import pytest
import torch

from oracle import cases, nets, step, synth

pytestmark = pytest.mark.gpu
S = cases.SEED


def test_ddpm_step_kernel_matches_closed_form():
    from medical_image_generation_amd import hipops as ops
    from medical_image_generation_amd._lib import call, ptr
    from medical_image_generation_amd.inferer import DDPMScheduler
    sch = DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205)
    ref = step.DDPMSchedule()
    assert torch.allclose(sch._coef, ref.step_coefficients(), rtol=1e-6, atol=1e-7)
    shape = (2, 3, 4, 6, 5)
    for t in (999, 500, 1, 0):
        x, z = synth.tensor(S, f"x{t}", shape) * 1.5, synth.tensor(S, f"z{t}", shape)
        eps = synth.tensor(S, f"e{t}", shape).bfloat16().float()
        want, _ = ref.step(eps, t, x, z, clip_sample=True)
        xd, zd = x.cuda(), z.cuda()
        eps_cl = ops.to_channels_last(eps.cuda())
        x_cl = torch.empty_like(eps_cl)
        td = torch.tensor([t], device="cuda")
        call("mi_diffusion_step", ptr(xd), ptr(eps_cl), ptr(zd), ptr(sch.coefficients("cuda")), ptr(td), None, None, None, None, None, ptr(x_cl),
             shape[1], shape[0], shape[1], 4 * 6 * 5, 1, 0)
        assert float((xd.cpu() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
        assert float((ops.to_channels_first(x_cl).cpu() - want).abs().max()) <= 1e-2 * float(want.abs().max())
    # v-prediction: the model output is the velocity
    schv = DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205, prediction_type="v_prediction")
    refv = step.DDPMSchedule(prediction_type="v_prediction")
    want, _ = refv.step(eps, 500, x, z, clip_sample=True)
    xd, td = x.cuda(), torch.tensor([500], device="cuda")
    call("mi_diffusion_step", ptr(xd), ptr(eps_cl), ptr(zd), ptr(schv.coefficients("cuda")), ptr(td), None, None, None, None, None, None, 0,
         shape[0], shape[1], 4 * 6 * 5, 3, 0)
    assert float((xd.cpu() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    pv, _ = schv.step(eps, 0, x)
    wv, _ = refv.step(eps, 0, x, None)
    assert torch.allclose(pv, wv, atol=1e-5)
    # upstream's tensor-level step() signature
    prev, x0 = sch.step(eps, 0, x)
    w_prev, w_x0 = ref.step(eps, 0, x, None)
    assert torch.allclose(prev, w_prev, atol=1e-5) and torch.allclose(x0, w_x0, atol=1e-5)
    sch.set_timesteps(10)
    assert sch.timesteps.tolist() == [900, 800, 700, 600, 500, 400, 300, 200, 100, 0]
    with pytest.raises(ValueError):
        sch.set_timesteps(2000)


@pytest.mark.parametrize("graph", [False, True])
def test_sample_loop_matches_oracle(graph):
    from medical_image_generation_amd.inferer import DDPMScheduler, DiffusionInferer
    from medical_image_generation_amd.unet import DiffusionModelUNet
    c = cases.UNET_CASES["unet3d"]
    ref = nets.DiffusionModelUNet(**c["kwargs"])
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    ref.load_state_dict(sd)
    net = DiffusionModelUNet(**c["kwargs"])
    net.load_state_dict(sd)
    net = net.cuda().eval()
    sch = DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205)
    sch.set_timesteps(5)
    steps = sch.timesteps.tolist()
    shape = c["shape"]
    x0 = synth.tensor(S, "sample_noise", shape)
    zs = [synth.tensor(S, f"sample_z{i}", shape) for i in range(len(steps))]
    oracle = step.DDPMSchedule()
    x = x0.clone()
    with torch.no_grad():
        for i, t in enumerate(steps):
            eps = ref(x, torch.full((shape[0],), t, dtype=torch.int64))
            x, _ = oracle.step(eps, t, x, zs[i], clip_sample=True)
    got = DiffusionInferer(sch).sample(x0.cuda(), net, sch, verbose=False, noises=[z.cuda() for z in zs], use_graph=graph)
    err = float((got.cpu() - x).norm() / x.norm())
    print(f"\n[sample loop graph={graph}] rel-L2 after {len(steps)} steps: {err:.3e}")
    assert torch.isfinite(got).all() and err <= 3e-2  # bf16 UNet forward, 5 steps (same budget as the forward parity tests)


@pytest.mark.parametrize("graph", [False, True])
def test_sample_loop_with_concat_conditioning_matches_oracle(graph):
    """sample(conditioning=, mode="concat"): model_input = cat([image, conditioning], dim=1) at every step (upstream
    `generative.inferers.DiffusionInferer.sample`, source absent: PARITY UNPINNED; restated here as the loop below); only the
    image channels are denoised, the condition channels stay as given."""
    from medical_image_generation_amd.inferer import DDPMScheduler, DiffusionInferer
    from medical_image_generation_amd.unet import DiffusionModelUNet
    kw = dict(cases.UNET_CASES["unet_ldm"]["kwargs"], in_channels=9, out_channels=8)
    ref = nets.DiffusionModelUNet(**kw)
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    ref.load_state_dict(sd)
    net = DiffusionModelUNet(**kw)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    sch = DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205)
    sch.set_timesteps(5)
    steps = sch.timesteps.tolist()
    shape = (2, 8, 8, 8, 8)
    x0 = synth.tensor(S, "sample_noise", shape)
    label = (synth.ellipsoid_volume(S, "label", (2, 1, 8, 8, 8)) > 0).float()
    zs = [synth.tensor(S, f"sample_z{i}", shape) for i in range(len(steps))]
    oracle = step.DDPMSchedule()
    x = x0.clone()
    with torch.no_grad():
        for i, t in enumerate(steps):
            eps = ref(torch.cat([x, label], dim=1), torch.full((shape[0],), t, dtype=torch.int64))
            x, _ = oracle.step(eps, t, x, zs[i], clip_sample=True)
    inf = DiffusionInferer(sch)
    got = inf.sample(x0.cuda(), net, sch, conditioning=label.cuda(), mode="concat", verbose=False, noises=[z.cuda() for z in zs], use_graph=graph)
    err = float((got.cpu() - x).norm() / x.norm())
    print(f"\n[concat-conditioned sample loop graph={graph}] rel-L2 after {len(steps)} steps: {err:.3e}")
    assert got.shape == shape and torch.isfinite(got).all() and err <= 3e-2
    with pytest.raises(ValueError):
        inf.sample(x0.cuda(), net, sch, verbose=False)  # 8 channels into a 9-channel net
    with pytest.raises(NotImplementedError):
        inf.sample(x0.cuda(), net, sch, conditioning=label.cuda(), mode="film", verbose=False)


def test_sample_loop_with_crossattn_conditioning_matches_oracle():
    """sample(conditioning=context, mode="crossattn") on a with_conditioning=True net (train_ldm.py:349-365's call shape with a
    context): the context is the model's `context=` at every step."""
    from medical_image_generation_amd.inferer import DDPMScheduler, DiffusionInferer
    from medical_image_generation_amd.unet import DiffusionModelUNet
    c = cases.UNET_CASES["unet2d_xattn"]
    ref = nets.DiffusionModelUNet(**c["kwargs"])
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    ref.load_state_dict(sd)
    net = DiffusionModelUNet(**c["kwargs"])
    net.load_state_dict(sd)
    net = net.cuda().eval()
    sch = DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205)
    sch.set_timesteps(4)
    steps = sch.timesteps.tolist()
    shape = c["shape"]
    x0 = synth.tensor(S, "sample_noise", shape)
    context = synth.tensor(S, "context", c["context"])
    zs = [synth.tensor(S, f"sample_z{i}", shape) for i in range(len(steps))]
    oracle = step.DDPMSchedule()
    x = x0.clone()
    with torch.no_grad():
        for i, t in enumerate(steps):
            eps = ref(x, torch.full((shape[0],), t, dtype=torch.int64), context=context)
            x, _ = oracle.step(eps, t, x, zs[i], clip_sample=True)
    inf = DiffusionInferer(sch)
    for graph in (False, True):
        got = inf.sample(x0.cuda(), net, sch, conditioning=context.cuda(), verbose=False, noises=[z.cuda() for z in zs], use_graph=graph)
        err = float((got.cpu() - x).norm() / x.norm())
        print(f"\n[cross-attention-conditioned sample loop graph={graph}] rel-L2 after {len(steps)} steps: {err:.3e}")
        assert torch.isfinite(got).all() and err <= 3e-2
    with pytest.raises(ValueError):
        inf.sample(x0.cuda(), net, sch, verbose=False)  # a conditioned net needs its context


def test_latent_inferer_decodes_through_the_autoencoder():
    """LatentDiffusionInferer.sample = latent sample loop, then autoencoder.decode_stage_2_outputs(latents / scale_factor)
    (train_ldm.py:112, 362-364)."""
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    from medical_image_generation_amd.inferer import DDPMScheduler, DiffusionInferer, LatentDiffusionInferer
    from medical_image_generation_amd.unet import DiffusionModelUNet
    ae_c = cases.AEKL_CASES["aekl_c3a"]
    ae = AutoencoderKL(**ae_c["kwargs"])
    ae.load_state_dict(synth.state_dict({k: tuple(v.shape) for k, v in ae.state_dict().items()}, S))
    ae = ae.cuda().eval()
    kw = dict(spatial_dims=3, in_channels=8, out_channels=8, num_res_blocks=1, num_channels=(32, 64), attention_levels=(False, True),
              num_head_channels=(0, 32), norm_num_groups=16, strides=[[1] * 3, [2] * 3], kernel_sizes=[[3] * 3] * 2, paddings=[[1] * 3] * 2)
    net = DiffusionModelUNet(**kw)
    net.load_state_dict(synth.state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, S))
    net = net.cuda().eval()
    sch = DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205)
    sch.set_timesteps(4)
    z = synth.tensor(S, "latent_noise", (1, 8, 8, 8, 8)).cuda()
    zs = [synth.tensor(S, f"latent_z{i}", (1, 8, 8, 8, 8)).cuda() for i in range(4)]
    scale = 0.7
    lat = DiffusionInferer(sch).sample(z, net, sch, verbose=False, noises=zs)
    img = LatentDiffusionInferer(sch, scale_factor=scale).sample(z, ae, net, sch, verbose=False, noises=zs)
    with torch.no_grad():
        want = ae.decode_stage_2_outputs(lat / scale)
    assert img.shape == (1, 1, 32, 32, 32) and torch.isfinite(img).all()
    assert torch.equal(img, want)
    img2, inter = LatentDiffusionInferer(sch, scale_factor=scale).sample(z, ae, net, sch, save_intermediates=True, intermediate_steps=250,
                                                                        verbose=False, noises=zs)
    assert torch.equal(img2, want) and len(inter) == 4 and inter[-1].shape == img.shape
