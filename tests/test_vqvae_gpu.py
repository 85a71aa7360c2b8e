"""The HIP VQVAE against the fp32 torch restatement (tests/vqvae_ref.py; upstream is not installed: PARITY UNPINNED).  Everything behind
the nearest-code search is discontinuous in the index, so the encoder output is compared first, then the indices given the device's own
z, then the decoder and every gradient given the device's indices.  Bounds: the per-tensor-class bf16 bounds tests/test_aekl_gpu.py
applies to the AutoencoderKL (activations 3e-2 rel-L2, loss 2e-2, gradients 6e-2 global rel-L2)."""
import pytest
import torch

from tests import vqvae_ref as R

pytestmark = pytest.mark.gpu

BASE = dict(spatial_dims=3, in_channels=1, out_channels=1, num_channels=(16, 32), num_res_layers=1, num_res_channels=(16, 32),
            num_embeddings=32, embedding_dim=8)
TUPLES = {"k4s2": dict(downsample_parameters=((2, 4, 1, 1),) * 2, upsample_parameters=((2, 4, 1, 1, 0),) * 2),
          "k3s2": dict(downsample_parameters=((2, 3, 1, 1),) * 2, upsample_parameters=((2, 3, 1, 1, 1),) * 2)}
Q_WEIGHT = 1.0


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _images(seed=0, shape=(2, 1, 16, 16, 16)):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _pair(name, seed=0, **extra):
    from medical_image_generation_amd.vqvae import VQVAE
    kw = dict(BASE, **TUPLES[name])
    torch.manual_seed(seed)
    ref = R.VQVAE(**kw)
    net = VQVAE(**dict(kw, **extra))
    net.load_state_dict(ref.state_dict())
    return ref, net.cuda()


@pytest.mark.parametrize("name", list(TUPLES))
def test_vqvae_matches_restatement(name):
    from medical_image_generation_amd import hipops as ops, vqvae as V
    ref, net = _pair(name)
    ref.train(), net.train()
    x = _images()
    xd = x.cuda().requires_grad_()
    xr = x.clone().requires_grad_()
    # 1. encoder
    z = net.encode(xd)
    zr = ref.encode(xr)
    assert z.shape == zr.shape == (2, 8, 4, 4, 4)
    e_z = rel_l2(z.detach().cpu(), zr.detach())
    # 2. indices given the device's own z (fp64 argmin, the assign test's criterion)
    cb0 = net.codebook.detach().clone()
    idx = V.vq_assign(ops.to_channels_last(z.detach()), cb0)
    tok = z.detach().cpu().permute(0, 2, 3, 4, 1).reshape(-1, 8).double()
    d = (tok * tok).sum(1, keepdim=True) - 2 * tok @ cb0.cpu().double().t() + (cb0.cpu().double() ** 2).sum(1)[None]
    best = R.nearest_code(tok, cb0.cpu().double())
    got = idx.cpu().long().reshape(-1)
    tau = R.assign_tolerance(tok, cb0.cpu())
    near = (d.topk(2, dim=1, largest=False).values[:, 1] - d.min(1).values) < tau
    assert bool(((got == best) | (near & (d.gather(1, got[:, None])[:, 0] - d.min(1).values <= tau))).all())
    # 3. decoder, loss and every gradient given the device's indices
    q, q_loss = net.quantize(z)
    recon = net.decode(q)
    loss = torch.nn.functional.l1_loss(recon, xd) + Q_WEIGHT * q_loss
    loss.backward()
    qr, q_loss_r = ref.quantize(zr, forced_idx=idx.cpu())
    recon_r = ref.decode(qr)
    loss_r = torch.nn.functional.l1_loss(recon_r, xr) + Q_WEIGHT * q_loss_r
    loss_r.backward()
    assert recon.shape == x.shape
    e_rec, e_q = rel_l2(recon.detach().cpu(), recon_r.detach()), rel_l2(q.detach().cpu(), qr.detach())
    rg = {n: p.grad for n, p in ref.named_parameters() if p.grad is not None}
    hg = {n: p.grad.cpu() for n, p in net.named_parameters() if p.grad is not None}
    assert sorted(hg) == sorted(rg) and not any(n.startswith("quantizer") for n in hg)
    e_glob = rel_l2(torch.cat([hg[n].flatten() for n in sorted(rg)]), torch.cat([rg[n].flatten() for n in sorted(rg)]))
    e_dx = rel_l2(xd.grad.cpu(), xr.grad)
    # every parameter gradient by itself: a small tensor (a bias through the fixed-order column sums, a ConvTranspose or patch-matrix conv
    # weight through the padded unpack) must not hide inside the norm of the large k3 weight gradients
    per = {n: (rel_l2(hg[n], rg[n]), float(torch.nn.functional.cosine_similarity(hg[n].flatten().double(), rg[n].flatten().double(), dim=0)))
           for n in sorted(rg)}
    worst = max(per, key=lambda n: per[n][0])
    print(f"\n[vqvae {name}] per-tensor gradients: worst rel-L2 {per[worst][0]:.3e} ({worst}), min cosine {min(c for _, c in per.values()):.5f}")
    for n, (e, c) in per.items():
        assert e <= 6e-2 and (c >= 0.99 or rg[n].numel() == 1), (n, e, c)
    qd, qref = net.quantizer.quantizer, ref.quantizer.quantizer
    e_cb = max(rel_l2(qd.embedding.weight.cpu(), qref.embedding.weight), rel_l2(qd.ema_w.cpu(), qref.ema_w),
               rel_l2(qd.ema_cluster_size.cpu(), qref.ema_cluster_size))
    print(f"\n[vqvae {name}] rel-L2: z {e_z:.3e} q {e_q:.3e} recon {e_rec:.3e} dx {e_dx:.3e} grads(global) {e_glob:.3e} codebook {e_cb:.3e}  "
          f"loss {float(loss.detach()):.6f} vs {float(loss_r.detach()):.6f}  q_loss {float(q_loss.detach()):.6f} vs {float(q_loss_r.detach()):.6f}")
    assert e_z <= 3e-2 and e_q <= 3e-2 and e_rec <= 3e-2 and e_cb <= 3e-2
    loss, loss_r, q_loss, q_loss_r = (float(v.detach()) for v in (loss, loss_r, q_loss, q_loss_r))
    assert abs(loss - loss_r) <= 2e-2 * loss_r and abs(q_loss - q_loss_r) <= 2e-2 * q_loss_r
    assert e_glob <= 6e-2 and e_dx <= 6e-2
    assert not torch.equal(qd.embedding.weight, cb0)  # training mode: the codebook moved
    assert abs(float(net.quantizer.perplexity) - float(qref.perplexity)) <= 1e-4 * float(qref.perplexity)


def test_methods_compose_and_eval_mode_keeps_the_codebook():
    from medical_image_generation_amd import hipops as ops, vqvae as V
    ref, net = _pair("k4s2")
    net.eval()
    q0 = net.quantizer.quantizer
    before = [t.detach().clone() for t in (q0.embedding.weight, q0.ema_cluster_size, q0.ema_w)]
    x = _images(1).cuda()
    with torch.no_grad():
        z = net.encode(x)
        q, q_loss = net.quantize(z)
        recon = net.decode(q)
        out, out_loss = net(x)
        assert torch.equal(out, recon) and torch.equal(out_loss, q_loss) and q_loss.shape == ()
        idx = net.index_quantize(x)
        assert idx.dtype == torch.int64 and idx.shape == (2, 4, 4, 4)
        assert torch.equal(idx, V.vq_assign(ops.to_channels_last(z), net.codebook.data).long())
        emb = net.codebook.data[idx].permute(0, 4, 1, 2, 3).contiguous()
        assert torch.equal(net.decode_samples(idx), net.decode(emb))
        assert torch.equal(net.encode_stage_2_inputs(x), z)
        assert torch.equal(net.decode_stage_2_outputs(z), recon)
    after = (q0.embedding.weight, q0.ema_cluster_size, q0.ema_w)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    # state_dict round trip with the restatement
    sd = net.state_dict()
    assert all(torch.equal(sd[k].cpu(), v) for k, v in ref.state_dict().items())
    ref.load_state_dict({k: v.cpu() for k, v in sd.items()})
    with pytest.raises(ValueError):
        net.encode(torch.zeros(1, 2, 16, 16, 16, device="cuda"))


def test_checkpoint_file_round_trips_the_quantiser_tensors(tmp_path):
    """The three quantiser tensors are in state_dict(), so the checkpoint module carries them like any parameter."""
    _, net = _pair("k4s2")
    net.train()
    with torch.no_grad():
        net(_images(2).cuda())  # one EMA update: the buffers differ from their initial values
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    names = [k for k in sd if k.startswith("quantizer.quantizer.")]
    assert sorted(names) == ["quantizer.quantizer.ema_cluster_size", "quantizer.quantizer.ema_w", "quantizer.quantizer.embedding.weight"]
    path = tmp_path / "vq.pth"
    torch.save(net.state_dict(), path)
    _, other = _pair("k4s2", seed=5)
    other.load_state_dict(torch.load(path, map_location="cuda"))
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in other.state_dict().items())


def test_use_checkpointing_gradients_are_bit_equal():
    grads = []
    for ck in (False, True):
        _, net = _pair("k4s2", use_checkpointing=ck)
        net.train()
        x = _images(3).cuda().requires_grad_()
        recon, q_loss = net(x)
        (torch.nn.functional.l1_loss(recon, x.detach()) + q_loss).backward()
        grads.append([x.grad.clone()] + [p.grad.clone() for _, p in sorted(net.named_parameters()) if p.grad is not None])
    assert len(grads[0]) == len(grads[1]) > 10 and all(torch.equal(a, b) for a, b in zip(*grads))
