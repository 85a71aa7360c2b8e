"""The 2-D PatchDiscriminator (csrc/disc2d.hip) and the 2-D GAN step of train_autoencoder.py (T-AE:371-435, the planner's `'2D'` section)
on the HIP path against the torch restatement in oracle/disc.py -- the 2-D mirror of test_discriminator_gpu.py, with its budgets.

Drift of torch's own bf16 autocast of the restatement against its fp32 self on these cases (CPU): input gradient rel-L2 7.0e-2 / 8.8e-2
(cosine 0.9976 / 0.9961), parameter gradient 5.2e-2 / 7.6e-2 (0.9986 / 0.9975), per-layer outputs <= 1.2e-2; of the GAN-step
composition: losses 0.07 % / 0.4 % / 0.2 %, autoencoder gradient cosine 0.9960 (norm ratio 1.008), discriminator gradient 7.6e-2
(cosine 0.9971).  The 3-D budgets keep at least 1.5x that margin.  ((2, 1, 64, 64) and a GAN step on 32x32 are ill-conditioned --
torch's bf16 alone drifts 0.72 there -- and are not used.)"""
import pytest
import torch

from oracle import cases, disc as odisc, nets, step, synth

pytestmark = pytest.mark.gpu
S = cases.SEED
DKW = dict(spatial_dims=2, num_channels=16, in_channels=1, out_channels=1, num_layers_d=3)
AEKW = dict(spatial_dims=2, in_channels=1, out_channels=1, latent_channels=4, num_res_blocks=1, num_channels=[16, 32, 64],
            attention_levels=[False] * 3, norm_num_groups=8, with_encoder_nonlocal_attn=False, with_decoder_nonlocal_attn=False,
            downsample_parameters=[[1, 3, 1], [2, 3, 1], [2, 3, 1]], upsample_parameters=[[2, 3, 1], [2, 3, 1]])
IMG = (2, 1, 40, 56)


def _pair(kw=DKW, seed=S):
    from medical_image_generation_amd.discriminator import PatchDiscriminator
    torch.manual_seed(seed)
    ref = odisc.PatchDiscriminator(**kw)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    for k, v in sd.items():  # the reference initialisation, redrawn so that biases / BatchNorm offsets are not zero
        if v.dtype.is_floating_point and "running" not in k:
            sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    ref.load_state_dict(sd)
    net = PatchDiscriminator(**kw)
    net.load_state_dict(sd)
    return ref, net.cuda()


def _ae_pair():
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    ref = nets.AutoencoderKL(**AEKW)
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    ref.load_state_dict(sd)
    ae = AutoencoderKL(**AEKW)
    assert {k: tuple(v.shape) for k, v in ae.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    ae.load_state_dict(sd)
    return ref, ae.cuda()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


FB_CASES = {
    "c16_2x1x48x48": (DKW, (2, 1, 48, 48), [(2, 16, 24, 24), (2, 32, 12, 12), (2, 64, 6, 6), (2, 128, 5, 5), (2, 1, 4, 4)]),
    # the planner's width on an odd, anisotropic two-channel input
    "c64_1x2x40x56": (dict(DKW, num_channels=64, in_channels=2), (1, 2, 40, 56),
                      [(1, 64, 20, 28), (1, 128, 10, 14), (1, 256, 5, 7), (1, 512, 4, 6), (1, 1, 3, 5)]),
}


@pytest.mark.parametrize("case", list(FB_CASES))
def test_discriminator2d_forward_backward_matches_oracle(case):
    from medical_image_generation_amd.discriminator import PatchAdversarialLoss
    kw, shape, out_shapes = FB_CASES[case]
    ref, net = _pair(kw)
    assert list(net.state_dict()) == list(ref.state_dict())
    x = synth.ellipsoid_volume(S, "dx", shape)
    xr = x.clone().requires_grad_(True)
    outs_r = ref(xr)
    adv = odisc.PatchAdversarialLoss()
    loss_r = adv(outs_r[-1], True) + 0.5 * adv(outs_r[2], False)
    loss_r.backward()
    xh = x.cuda().requires_grad_(True)
    outs_h = net(xh)
    assert [tuple(o.shape) for o in outs_h] == [tuple(o.shape) for o in outs_r] == out_shapes
    for i, (a, b) in enumerate(zip(outs_h, outs_r)):
        e = rel_l2(a.detach().cpu(), b.detach())
        print(f"\n  layer {i}: rel-L2 {e:.3e}", end="")
        assert e <= 3e-2, f"layer {i}: rel-L2 {e:.3e}"
    advh = PatchAdversarialLoss()
    loss_h = advh(outs_h[-1], True) + 0.5 * advh(outs_h[2], False)
    assert abs(float(loss_h) - float(loss_r)) <= 2e-2 * abs(float(loss_r))
    loss_h.backward()
    e = rel_l2(xh.grad.cpu(), xr.grad)
    cosx = float(torch.dot(xh.grad.cpu().flatten(), xr.grad.flatten()) / (xh.grad.norm().cpu() * xr.grad.norm()))
    print(f"\n[PatchDiscriminator 2-D {case}] loss {float(loss_h):.5f} vs {float(loss_r):.5f}; input-gradient rel-L2 {e:.3e}, cosine {cosx:.4f}")
    pr, ph = dict(ref.named_parameters()), dict(net.named_parameters())
    for n in pr:
        print(f"    {n:28s} grad rel-L2 {rel_l2(ph[n].grad.cpu(), pr[n].grad):.3e}  |g| {float(pr[n].grad.norm()):.3e}")
    g_ref = torch.cat([pr[n].grad.flatten() for n in pr])
    g_hip = torch.cat([ph[n].grad.cpu().flatten() for n in pr])
    eg = rel_l2(g_hip, g_ref)
    cosp = float(torch.dot(g_hip, g_ref) / (g_hip.norm() * g_ref.norm()))
    print(f"  parameter-gradient rel-L2 {eg:.3e}, cosine {cosp:.4f}")
    assert e <= 1.5e-1 and cosx >= 0.99
    assert eg <= 1.2e-1 and cosp >= 0.99
    for k, v in ref.state_dict().items():  # BatchNorm buffers after ONE training-mode forward
        if "running" in k:
            assert torch.allclose(net.state_dict()[k].cpu(), v, rtol=3e-2, atol=3e-3), k
        if "num_batches_tracked" in k:
            assert int(net.state_dict()[k]) == int(v) == 1


def test_autoencoder2d_forward_backward_matches_oracle():
    """Nothing else runs the 2-D AutoencoderKL on the GPU: forward / backward against oracle.nets on the GAN step's shape, with the budgets
    of test_aekl_gpu.py (outputs 3e-2, loss 2e-2, global gradient 6e-2)."""
    ref, ae = _ae_pair()
    x = synth.ellipsoid_volume(S, "x", IMG)
    xd = x.cuda()
    z_mu, z_sigma = ae.encode(xd)
    eps = synth.tensor(S, "eps", tuple(z_mu.shape))
    recon = ae.decode(z_mu + eps.cuda() * z_sigma)
    klw = 1e-3
    loss = torch.nn.functional.l1_loss(recon, xd) + step.kl_loss(z_mu, z_sigma) * klw
    loss.backward()
    lr, rrecon, rmu, rsig = step.ae_loss(ref, x, eps, klw)
    lr.backward()
    assert recon.shape == x.shape
    e = {k: rel_l2(a.detach().cpu(), b.detach()) for k, a, b in (("z_mu", z_mu, rmu), ("z_sigma", z_sigma, rsig), ("recon", recon, rrecon))}
    rg = {n: p.grad for n, p in ref.named_parameters() if p.grad is not None}
    hg = {n: p.grad.cpu() for n, p in ae.named_parameters() if p.grad is not None}
    assert sorted(hg) == sorted(rg)
    e_glob = rel_l2(torch.cat([hg[n].flatten() for n in sorted(rg)]), torch.cat([rg[n].flatten() for n in sorted(rg)]))
    print(f"\n[aekl 2-D] rel-L2: {e}  loss {float(loss):.6f} vs {float(lr):.6f}  grads(global) {e_glob:.3e}")
    assert all(v <= 3e-2 for v in e.values())
    assert abs(float(loss) - float(lr)) <= 2e-2 * float(lr)
    assert e_glob <= 6e-2


def _perc():
    from medical_image_generation_amd.perceptual import PerceptualLoss
    torch.manual_seed(3)
    return PerceptualLoss(spatial_dims=2, network_type="vgg", is_fake_3d=True, fake_3d_ratio=0.2, pretrained=False).cuda()


@pytest.mark.parametrize("graph", [False, True])
def test_gan_step2d_matches_oracle_composition(graph):
    """AEGANTrainer on a 2-D autoencoder and the 2-D discriminator: generator step with the adversarial term through the frozen
    discriminator, then the discriminator step on the same reconstruction -- losses and the gradients of BOTH networks against the same
    composition of the CPU restatements."""
    from medical_image_generation_amd.trainer import AEGANTrainer
    ae_ref, ae = _ae_pair()
    d_ref, d = _pair()
    x = synth.ellipsoid_volume(S, "x", IMG)
    with torch.no_grad():
        zshape = tuple(ae_ref.encode(x)[0].shape)
    eps = synth.tensor(S, "eps0", zshape)
    klw, advw = 1e-3, 0.5
    adv = odisc.PatchAdversarialLoss()
    d_ref.train()
    for p in d_ref.parameters():
        p.requires_grad_(False)
    loss_g, recon, gen = odisc.generator_loss(ae_ref, d_ref, adv, x, eps, klw, advw)
    loss_g.backward()
    for p in d_ref.parameters():
        p.requires_grad_(True)
    loss_d = odisc.discriminator_loss(d_ref, adv, x, recon, advw)
    loss_d.backward()
    tr = AEGANTrainer(ae, d, adv_weight=advw, kl_weight=klw, lr=cases.STEP_LR, d_lr=cases.STEP_LR, max_grad_norm=1.0)
    xd, ed = x.cuda(), eps.cuda()
    if graph:
        tr.capture(xd, ed)
        tr._g_fb.replay()
        tr._g_d.replay()
    else:
        tr.forward_backward(xd, ed)
        tr.d_forward_backward(xd)
    print(f"\n[2-D GAN step graph={graph}] generator loss {float(tr.loss):.5f} vs {float(loss_g):.5f} (adv term {float(tr.gen_loss):.5f} vs "
          f"{float(gen):.5f}); discriminator loss {float(tr.disc_loss):.5f} vs {float(loss_d):.5f}")
    assert abs(float(tr.loss) - float(loss_g)) <= 2e-2 * abs(float(loss_g))
    assert abs(float(tr.gen_loss) - float(gen)) <= 5e-2 * abs(float(gen))
    assert abs(float(tr.disc_loss) - float(loss_d)) <= 5e-2 * abs(float(loss_d))
    sd_h = d.state_dict()
    for k, v in d_ref.state_dict().items():  # three training-mode forwards: D(recon) in the generator step, then D(recon), D(images)
        if "running" in k:
            assert torch.allclose(sd_h[k].cpu(), v, rtol=3e-2, atol=3e-3), k
        if "num_batches_tracked" in k:
            assert int(sd_h[k]) == int(v) == 3, k
    names = [n for n, p in ae_ref.named_parameters() if p.grad is not None]
    g_ref = torch.cat([dict(ae_ref.named_parameters())[n].grad.flatten() for n in names])
    g_hip = torch.cat([tr.arena.gview(n).cpu().flatten() for n in names])
    cos = float(torch.dot(g_ref, g_hip) / (g_ref.norm() * g_hip.norm()))
    print(f"  autoencoder gradient: cosine {cos:.4f}, norm ratio {float(g_hip.norm() / g_ref.norm()):.3f}")
    assert cos >= 0.98 and abs(float(g_hip.norm() / g_ref.norm()) - 1) <= 0.05
    dn = [n for n, p in d_ref.named_parameters()]
    gd_ref = torch.cat([dict(d_ref.named_parameters())[n].grad.flatten() for n in dn])
    gd_hip = torch.cat([tr.d_arena.gview(n).cpu().flatten() for n in dn])
    e = rel_l2(gd_hip, gd_ref)
    cosd = float(torch.dot(gd_hip, gd_ref) / (gd_hip.norm() * gd_ref.norm()))
    print(f"  discriminator gradient rel-L2 {e:.3e}, cosine {cosd:.4f}")
    if not graph:  # (the captured discriminator graph runs its optimizer behind the gradients, as in the 3-D test)
        assert e <= 1.2e-1 and cosd >= 0.99
    before_g, before_d = tr.arena.data.clone(), tr.d_arena.data.clone()
    loss = tr.step_graph(xd, ed) if graph else tr.step(xd, ed)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(tr.arena.data).all()) and bool(torch.isfinite(tr.d_arena.data).all())
    assert float((tr.arena.data - before_g).abs().max()) > 0 and float((tr.d_arena.data - before_d).abs().max()) > 0


def test_gan_step2d_with_perceptual_term_in_one_captured_graph():
    """perceptual=PerceptualLoss(spatial_dims=2) (random weights) in the same captured generator graph: the captured step's `loss` is
    L1 + KL + perc_loss + gen_loss of the device scalars (L1 + KL: the plain autoencoder step's loss on the same weights and noise)."""
    from medical_image_generation_amd.trainer import AEGANTrainer, AETrainer
    _, ae = _ae_pair()
    _, d = _pair()
    x = synth.ellipsoid_volume(S, "x", IMG).cuda()
    with torch.no_grad():
        zshape = tuple(ae.encode(x)[0].shape)
    eps = synth.tensor(S, "eps0", zshape).cuda()
    klw = 1e-3
    base = AETrainer(ae, lr=cases.STEP_LR, kl_weight=klw)
    base.forward_backward(x, eps)
    l1_kl = float(base.loss)
    tr = AEGANTrainer(ae, d, adv_weight=0.5, kl_weight=klw, lr=cases.STEP_LR, d_lr=cases.STEP_LR, perceptual=_perc(), perc_weight=0.125)
    tr.capture(x, eps)
    tr._g_fb.replay()
    torch.cuda.synchronize()
    loss, perc, gen = float(tr.loss), float(tr.perc_loss), float(tr.gen_loss)
    print(f"\n[2-D GAN step + perceptual, captured] loss {loss:.6f} = L1 + KL {l1_kl:.6f} + perceptual {perc:.6f} + adversarial {gen:.6f}")
    assert perc > 0 and gen > 0
    assert abs(loss - (l1_kl + perc + gen)) <= 1e-5 * abs(loss)
    before_g, before_d = tr.arena.data.clone(), tr.d_arena.data.clone()
    out = tr.step_graph(x, eps)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(tr.arena.data).all()) and bool(torch.isfinite(tr.d_arena.data).all())
    assert float((tr.arena.data - before_g).abs().max()) > 0 and float((tr.d_arena.data - before_d).abs().max()) > 0
    # capture() leaves the buffers as they were; since then: two replays of the generator graph (one forward each), one discriminator step (two)
    assert int(d.state_dict()["0.adn.N.num_batches_tracked"]) == 4
