"""VQAETrainer: the VQ-VAE train step (L1 + q_weight * quantization loss, EMA codebook update inside the step) against the torch
restatement given the device's indices, eager against captured, validation, and the refusals.  Bounds: those of
tests/test_trainer_gpu.py::test_ae_three_train_steps (loss 2e-2, update cosine >= 0.85, update norm within 5 %)."""
import pytest
import torch

from tests import vqvae_ref as R
from tests.test_vqvae_gpu import BASE, TUPLES, _images, rel_l2

pytestmark = pytest.mark.gpu
LR = 1e-3
QW = 0.7


def _nets(seed=0):
    from medical_image_generation_amd.vqvae import VQVAE
    kw = dict(BASE, **TUPLES["k4s2"])
    torch.manual_seed(seed)
    ref = R.VQVAE(**kw)
    net = VQVAE(**kw)
    net.load_state_dict(ref.state_dict())
    return ref, net.cuda()


def test_one_step_matches_restatement_given_the_device_indices():
    from medical_image_generation_amd import hipops as ops, vqvae as V
    from medical_image_generation_amd.trainer import VQAETrainer
    ref, net = _nets()
    ref.train(), net.train()
    sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
    x = _images(4)
    xd = x.cuda()
    with torch.no_grad():  # the indices the step will pick: the device's own encoder output against the initial codebook
        idx = V.vq_assign(ops.to_channels_last(net.encode(xd)), net.codebook.data.clone()).cpu()
    tr = VQAETrainer(net, q_weight=QW, lr=LR, max_grad_norm=1.0)
    arena_names = {n for n, _, _ in net._entries}
    assert not any(n.startswith("quantizer") for n in arena_names)  # the codebook is absent from the arena
    assert tr.arena.n_trainable == sum(p.numel() + (-p.numel()) % 4 for n, p in net.named_parameters() if not n.startswith("quantizer"))
    loss = float(tr.step(xd))
    opt = torch.optim.Adam([p for p in ref.parameters() if p.requires_grad], lr=LR)
    recon_r, ql_r = ref(x, forced_idx=idx)
    loss_r = torch.nn.functional.l1_loss(recon_r, x) + QW * ql_r
    loss_r.backward()
    torch.nn.utils.clip_grad_norm_([p for p in ref.parameters() if p.requires_grad], 1.0)
    opt.step()
    print(f"\n[vq step] loss hip {loss:.6f} ref {float(loss_r.detach()):.6f}  q_loss hip {float(tr.q_loss):.6f} ref {float(ql_r.detach()):.6f}")
    loss_r, ql_r = float(loss_r.detach()), float(ql_r.detach())
    assert abs(loss - loss_r) <= 2e-2 * loss_r and abs(float(tr.q_loss) - ql_r) <= 2e-2 * ql_r
    names = [n for n, p in ref.named_parameters() if p.grad is not None]
    upd_ref = torch.cat([(ref.state_dict()[n] - sd0[n]).flatten() for n in names])
    upd_hip = torch.cat([(net.state_dict()[n].cpu() - sd0[n]).flatten() for n in names])
    cos = float(torch.dot(upd_ref, upd_hip) / (upd_ref.norm() * upd_hip.norm()))
    print(f"  update cosine {cos:.4f}  |upd| ref {float(upd_ref.norm()):.4f} hip {float(upd_hip.norm()):.4f}")
    assert cos >= 0.85 and abs(float(upd_hip.norm()) / float(upd_ref.norm()) - 1) <= 0.05
    qd, qr = net.quantizer.quantizer, ref.quantizer.quantizer
    for a, b in ((qd.embedding.weight, qr.embedding.weight), (qd.ema_w, qr.ema_w), (qd.ema_cluster_size, qr.ema_cluster_size)):
        assert rel_l2(a.cpu(), b) <= 3e-2  # (bf16 tokens against fp32 tokens; the counts are exact)
    assert torch.equal(qd.ema_cluster_size.cpu(), qr.ema_cluster_size)
    assert not torch.equal(qd.embedding.weight.cpu(), sd0["quantizer.quantizer.embedding.weight"])


def test_three_captured_steps_are_bit_equal_to_eager_and_validate_changes_nothing():
    from medical_image_generation_amd.trainer import VQAETrainer
    runs = []
    for graph in (False, True):
        _, net = _nets()
        net.train()
        tr = VQAETrainer(net, q_weight=QW, lr=LR)
        losses = []
        for k in range(3):
            xd = _images(10 + k).cuda()
            if graph and k == 0:
                sd = {n: v.clone() for n, v in net.state_dict().items()}
                perp = net.quantizer.perplexity.clone()
                tr.capture(xd)  # warm-up passes and capture: no optimizer step, and the codebook the warm-up moved is put back
                assert all(torch.equal(sd[n], v) for n, v in net.state_dict().items()) and torch.equal(perp, net.quantizer.perplexity)
            if k == 2:
                tr.q_weight = 0.3  # a device scalar: the captured graph follows it
            losses.append((tr.step_graph(xd) if graph else tr.step(xd)).clone())
        runs.append((losses, {n: v.clone() for n, v in net.state_dict().items()}, net.quantizer.perplexity.clone(), tr, net))
    (la, sa, pa, _, _), (lb, sb, pb, tr, net) = runs
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    assert all(torch.equal(sa[n], sb[n]) for n in sa) and torch.equal(pa, pb)
    # validate: eval-mode forward, nothing the train step owns is written, no codebook update
    state = {n: v.clone() for n, v in net.state_dict().items()}
    moments = (tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.step_count.clone(), tr.loss.clone(), tr.q_loss.clone())
    net.eval()
    xd = _images(20).cuda()
    val, recon = tr.validate(xd, return_recon=True)
    with torch.no_grad():
        want = torch.nn.functional.l1_loss(net(xd)[0], xd)
    assert abs(float(val) - float(want)) <= 1e-5 * float(want) and recon.shape == xd.shape
    net.train()
    assert all(torch.equal(state[n], v) for n, v in net.state_dict().items())
    assert all(torch.equal(a, b) for a, b in zip(moments, (tr.exp_avg, tr.exp_avg_sq, tr.step_count, tr.loss, tr.q_loss)))


def test_checkpoint_round_trips_the_quantiser_tensors(tmp_path):
    from medical_image_generation_amd import checkpoint
    from medical_image_generation_amd.trainer import VQAETrainer
    _, net = _nets()
    net.train()
    tr = VQAETrainer(net, lr=LR)
    tr.step(_images(30).cuda())
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    assert {k for k in sd if k.startswith("quantizer")} == {"quantizer.quantizer.embedding.weight", "quantizer.quantizer.ema_cluster_size",
                                                          "quantizer.quantizer.ema_w"}
    path = checkpoint.save_model(tr, str(tmp_path), 0, 1.0)
    _, other = _nets(seed=9)
    tr2 = VQAETrainer(other, lr=LR)
    checkpoint.load_model(tr2, path)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in other.state_dict().items())


def test_refusals():
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    from medical_image_generation_amd.discriminator import PatchDiscriminator
    from medical_image_generation_amd.trainer import AEGANTrainer, AETrainer, VQAETrainer
    _, net = _nets()
    with pytest.raises(TypeError, match="VQAETrainer"):
        AETrainer(net)
    with pytest.raises(TypeError, match="VQAETrainer"):
        AEGANTrainer(net, PatchDiscriminator(3, 8, 1).cuda())
    ae = AutoencoderKL(3, 1, 1, num_res_blocks=1, num_channels=(32, 32), attention_levels=(False, False), latent_channels=8,
                       with_encoder_nonlocal_attn=False, with_decoder_nonlocal_attn=False).cuda()
    with pytest.raises(TypeError, match="VQVAE"):
        VQAETrainer(ae)
    tr = VQAETrainer(net)
    with pytest.raises(ValueError):
        tr.step(torch.zeros(1, 2, 16, 16, 16, device="cuda"))
    with pytest.raises(RuntimeError):
        tr.step(torch.zeros(1, 1, 16, 16, 16))


def _unet(seed=3):
    from oracle import cases, synth
    from medical_image_generation_amd.unet import DiffusionModelUNet
    ukw = dict(cases.UNET_CASES["unet_ldm"]["kwargs"])  # in / out 8 = the VQVAE's embedding_dim
    net = DiffusionModelUNet(**ukw)
    net.load_state_dict(synth.state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed))
    return net.cuda()


def test_ldm_trainer_vq_mode_equals_ddpm_step_on_the_normalised_latents():
    """LDMTrainer(autoencoder=VQVAE): latents = encode(images) without gradient or quantisation, x0 = 2 (z - min) / (max - min) - 1 with
    the codebook's range, then the DDPM step -- against DDPMTrainer fed that x0 computed in torch.  Bounds of
    tests/test_trainer_gpu.py::test_ldm_step_matches_oracle_composition (loss 1.5e-2, gradient rel-L2 5e-2)."""
    from medical_image_generation_amd.trainer import DDPMTrainer, LDMTrainer
    _, ae = _nets()
    ae.eval()
    x = _images(40, (2, 1, 32, 32, 32)).cuda()
    with torch.no_grad():
        z = ae.encode(x)
    cb = ae.codebook.data
    lo, hi = float(cb.min()), float(cb.max())
    x0 = 2 * (z - lo) / (hi - lo) - 1
    g = torch.Generator().manual_seed(41)
    noise = torch.randn(z.shape, generator=g).cuda()
    t = torch.tensor([250, 750]).cuda()
    ref = DDPMTrainer(_unet(), lr=1e-4)
    ref.forward_backward(x0.contiguous(), noise, t)
    before = {n: v.clone() for n, v in ae.state_dict().items()}
    tr = LDMTrainer(_unet(), ae, lr=1e-4)
    assert tr.latent_space_type == "vq" and (tr.codebook_min, tr.codebook_max) == (lo, hi)
    tr.forward_backward(x, None, noise, t)
    n = tr.arena.n_trainable
    e = rel_l2(tr.arena.grad[:n].cpu(), ref.arena.grad[:n].cpu())
    print(f"\n[LDM vq step] loss {float(tr.loss):.6f} vs {float(ref.loss):.6f}; gradient rel-L2 {e:.3e}")
    assert abs(float(tr.loss) - float(ref.loss)) <= 1.5e-2 * float(ref.loss) and e <= 5e-2
    assert float(tr.ae_arena.grad.abs().max()) == 0.0  # the autoencoder is frozen
    assert all(torch.equal(before[k], v) for k, v in ae.state_dict().items())  # and its codebook is not updated
    with pytest.raises(ValueError, match="eps must be None"):
        tr.forward_backward(x, torch.zeros_like(z), noise, t)
    # the range lives in device scalars: a captured step follows refresh_codebook_range()
    tr.capture(x, None, noise, t)
    l1 = float(tr.step_graph())
    assert abs(l1 - float(ref.loss)) <= 1.5e-2 * float(ref.loss)
    with pytest.raises(RuntimeError):
        tr.estimate_scale_factor(x, None)
    with pytest.raises(TypeError):
        LDMTrainer(_unet(), ae, latent_space_type="vae")


def test_vq_latent_inferer_sample_is_the_hand_composition():
    """VQLatentDiffusionInferer.sample over 3 DDIM steps = DiffusionInferer.sample on the latent shape, denormalize, quantize (no update),
    decode -- bit for bit through public methods; denormalize / normalize against the torch formulas."""
    from medical_image_generation_amd.inferer import DDIMScheduler, DiffusionInferer, VQLatentDiffusionInferer
    _, ae = _nets()
    ae.train()  # sampling must not move the codebook even in training mode
    before = {n: v.clone() for n, v in ae.state_dict().items()}
    unet = _unet()
    sched = DDIMScheduler(1000, "scaled_linear_beta", beta_start=0.0015, beta_end=0.0205)
    sched.set_timesteps(3)
    start = torch.randn((2, 8, 8, 8, 8), generator=torch.Generator().manual_seed(7)).cuda()
    inf = VQLatentDiffusionInferer(sched, ae)
    image = inf.sample(start, unet, use_graph=True)
    assert image.shape == (2, 1, 32, 32, 32)
    assert all(torch.equal(before[k], v) for k, v in ae.state_dict().items())
    latent = DiffusionInferer(sched).sample(start, unet, use_graph=True)
    z = inf.denormalize(latent)
    ae.eval()
    with torch.no_grad():
        q, _ = ae.quantize(z)
        hand = ae.decode(q)
    assert torch.equal(image, hand)
    lo, hi = inf.codebook_min, inf.codebook_max
    want = (latent.double() + 1) / 2 * (hi - lo) + lo
    assert float((z.double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max() + abs(lo) + abs(hi))
    back = inf.normalize(z)
    assert float((back - latent).abs().max()) <= 16 * 2.0 ** -24 * float(latent.abs().max() + 1)
    from medical_image_generation_amd.sliding import SlidingWindowInferer
    with pytest.raises(NotImplementedError):
        inf.sample(start, unet, window_inferer=SlidingWindowInferer((4, 4, 4)))
    with pytest.raises(NotImplementedError):
        inf.sample(start, unet, decode_inferer=SlidingWindowInferer((4, 4, 4)))
    # the training-side call: normalised no-grad encoding, then DiffusionInferer.__call__
    x = _images(50, (2, 1, 32, 32, 32)).cuda()
    noise = torch.randn((2, 8, 8, 8, 8), generator=torch.Generator().manual_seed(8)).cuda()
    t = torch.tensor([100, 600]).cuda()
    with torch.no_grad():
        pred = inf(x, unet, noise, t)
        want = DiffusionInferer(sched)(inf.normalize(ae.encode(x)), unet, noise, t)
    assert torch.equal(pred, want)
