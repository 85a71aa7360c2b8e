"""CPU side of the VQ-VAE: the torch restatement (tests/vqvae_ref.py) against hand-computed numbers, the product's constructor
surface and state_dict names against it, the header's new entry points, and the near-tie shares of the GPU tests' inputs."""
import math

import pytest
import torch

from tests import abi_header, vqvae_ref as R

SMALL = dict(spatial_dims=3, in_channels=1, out_channels=1, num_channels=(16, 32), num_res_layers=1, num_res_channels=(16, 32),
             downsample_parameters=((2, 4, 1, 1),) * 2, upsample_parameters=((2, 4, 1, 1, 0),) * 2, num_embeddings=32, embedding_dim=8)


def test_quantiser_two_codes_by_hand():
    q = R.Quantizer(2, 2, commitment_cost=0.25, decay=0.5, epsilon=0.0, dtype=torch.float64)
    with torch.no_grad():
        q.embedding.weight.copy_(torch.tensor([[0.0, 0.0], [2.0, 2.0]]))
        q.ema_w.copy_(q.embedding.weight)
    # tokens (channels-last order): (0.5, 0.5) -> code 0, (1.5, 2) -> code 1, (1, 1) -> a tie, lowest index 0
    z = torch.tensor([[0.5, 0.5], [1.5, 2.0], [1.0, 1.0]], dtype=torch.float64).t().reshape(1, 2, 3, 1, 1).requires_grad_()
    q.train()
    loss, out, idx = q(z)
    assert idx.flatten().tolist() == [0, 1, 0]
    # loss = 0.25 * mean over 6 elements of (q - z)^2 = 0.25 * (0.25 + 0.25 + 0.25 + 0 + 1 + 1) / 6
    assert float(loss.detach()) == pytest.approx(0.25 * 2.75 / 6, rel=1e-15)
    # q came from the OLD codebook
    assert out.permute(0, 2, 3, 4, 1).reshape(3, 2).tolist() == [[0.0, 0.0], [2.0, 2.0], [0.0, 0.0]]
    # one EMA step: counts (2, 1); cluster = 0.5 * 1 + 0.5 * counts = (1.5, 1); n = 2.5, eps = 0 -> w = cluster
    assert q.ema_cluster_size.tolist() == [1.5, 1.0]
    # dw = ((1.5, 1.5), (1.5, 2)); ema_w = 0.5 * old + 0.5 * dw = ((0.75, 0.75), (1.75, 2)); embedding = ema_w / w
    assert q.ema_w.tolist() == [[0.75, 0.75], [1.75, 2.0]]
    assert torch.allclose(q.embedding.weight, torch.tensor([[0.5, 0.5], [1.75, 2.0]], dtype=torch.float64), rtol=1e-15, atol=0)
    p = torch.tensor([2 / 3, 1 / 3], dtype=torch.float64)
    assert float(q.perplexity) == pytest.approx(float(torch.exp(-(p * torch.log(p + 1e-10)).sum())), rel=1e-15)
    # straight-through: d(out)/dz = 1, d(loss)/dz = 2 cc (z - q) / numel
    (out.sum() + 3 * loss).backward()
    zl = z.detach().permute(0, 2, 3, 4, 1).reshape(3, 2)
    want = 1 + 3 * 2 * 0.25 * (zl - torch.tensor([[0.0, 0.0], [2.0, 2.0], [0.0, 0.0]])) / 6
    assert torch.allclose(z.grad.permute(0, 2, 3, 4, 1).reshape(3, 2), want, rtol=0, atol=1e-15)


def test_ema_recurrence_three_steps_by_hand():
    """One code, one channel, decay 0.5, eps 1e-5, three batches: the recurrences in Python floats beside the restatement."""
    K, eps, decay = 1, 1e-5, 0.5
    emb, cl, ew = torch.tensor([[1.0]], dtype=torch.float64), torch.ones(1, dtype=torch.float64), torch.tensor([[1.0]], dtype=torch.float64)
    c, e = 1.0, 1.0
    for x in ([2.0, 4.0], [1.0], [3.0, 3.0, 3.0]):
        xt = torch.tensor(x, dtype=torch.float64)[:, None]
        emb, cl, ew, perp, counts, dw = R.ema_update(xt, torch.zeros(len(x), dtype=torch.long), emb, cl, ew, decay, eps)
        c = decay * c + (1 - decay) * len(x)
        e = decay * e + (1 - decay) * sum(x)
        w = (c + eps) / (c + K * eps) * c  # one code: n = c, so w = c
        assert float(cl) == pytest.approx(c, rel=1e-15) and float(ew) == pytest.approx(e, rel=1e-15)
        assert float(emb) == pytest.approx(e / w, rel=1e-14) and float(perp) == pytest.approx(math.exp(-math.log(1 + 1e-10)), rel=1e-12)
    assert (c, e) == (0.5 * (0.5 * (0.5 + 1) + 0.5) + 1.5, 0.5 * (0.5 * (0.5 + 3) + 0.5) + 4.5)
    # an unused code follows the same formulas: its ema_w and cluster size decay, eps keeps w > 0
    emb2, cl2, ew2, *_ = R.ema_update(torch.ones(4, 1, dtype=torch.float64), torch.zeros(4, dtype=torch.long), torch.ones(2, 1, dtype=torch.float64),
                                      torch.zeros(2, dtype=torch.float64), torch.ones(2, 1, dtype=torch.float64), 0.5, 1e-5)
    assert float(cl2[1]) == 0.0 and float(ew2[1]) == 0.5 and torch.isfinite(emb2).all()


def test_constructor_errors():
    from medical_image_generation_amd.vqvae import VQVAE
    for cls in (VQVAE, R.VQVAE):
        with pytest.raises(ValueError):
            cls(**dict(SMALL, num_res_channels=(16, 32, 64)))
        with pytest.raises(ValueError):
            cls(**dict(SMALL, downsample_parameters=((2, 4, 1, 1),) * 3))
        with pytest.raises(ValueError):
            cls(**dict(SMALL, upsample_parameters=((2, 4, 1, 1, 0),)))
        with pytest.raises(ValueError):
            cls(**dict(SMALL, downsample_parameters=((2, 4, 1),) * 2))
        with pytest.raises(ValueError):
            cls(**dict(SMALL, upsample_parameters=((2, 4, 1, 1),) * 2))
    assert VQVAE(**dict(SMALL, num_res_channels=16)).num_res_channels == (16, 16)
    for kw, word in ((dict(spatial_dims=2), "spatial_dims"), (dict(downsample_parameters=((2, 4, 2, 1),) * 2), "downsample_parameters"),
                     (dict(upsample_parameters=((2, 4, 2, 1, 0),) * 2), "upsample_parameters"), (dict(dropout=0.1), "dropout"),
                     (dict(act="PRELU"), "act"), (dict(output_act="tanh"), "output_act"),
                     (dict(downsample_parameters=((2, (4, 4, 3), 1, 1),) * 2), "cubic"),
                     (dict(upsample_parameters=((2, 4, 1, 1, 2),) * 2), "output_padding")):
        with pytest.raises(NotImplementedError, match=word):
            VQVAE(**dict(SMALL, **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VQVAE(**SMALL).encode(torch.zeros(1, 1, 16, 16, 16))


def test_state_dict_names_and_shapes():
    from medical_image_generation_amd.vqvae import VQVAE
    net, ref = VQVAE(**SMALL), R.VQVAE(**SMALL)
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert sorted(got) == sorted((k, tuple(v.shape)) for k, v in ref.state_dict().items())
    want = [("encoder.blocks.0.conv.weight", (16, 1, 4, 4, 4)), ("encoder.blocks.0.conv.bias", (16,)),
            ("encoder.blocks.1.conv1.conv.weight", (16, 16, 3, 3, 3)), ("encoder.blocks.1.conv1.conv.bias", (16,)),
            ("encoder.blocks.1.conv2.conv.weight", (16, 16, 3, 3, 3)), ("encoder.blocks.1.conv2.conv.bias", (16,)),
            ("encoder.blocks.2.conv.weight", (32, 16, 4, 4, 4)), ("encoder.blocks.2.conv.bias", (32,)),
            ("encoder.blocks.3.conv1.conv.weight", (32, 32, 3, 3, 3)), ("encoder.blocks.3.conv1.conv.bias", (32,)),
            ("encoder.blocks.3.conv2.conv.weight", (32, 32, 3, 3, 3)), ("encoder.blocks.3.conv2.conv.bias", (32,)),
            ("encoder.blocks.4.conv.weight", (8, 32, 3, 3, 3)), ("encoder.blocks.4.conv.bias", (8,)),
            ("decoder.blocks.0.conv.weight", (32, 8, 3, 3, 3)), ("decoder.blocks.0.conv.bias", (32,)),
            ("decoder.blocks.1.conv1.conv.weight", (32, 32, 3, 3, 3)), ("decoder.blocks.1.conv1.conv.bias", (32,)),
            ("decoder.blocks.1.conv2.conv.weight", (32, 32, 3, 3, 3)), ("decoder.blocks.1.conv2.conv.bias", (32,)),
            ("decoder.blocks.2.conv.weight", (32, 16, 4, 4, 4)), ("decoder.blocks.2.conv.bias", (16,)),
            ("decoder.blocks.3.conv1.conv.weight", (16, 16, 3, 3, 3)), ("decoder.blocks.3.conv1.conv.bias", (16,)),
            ("decoder.blocks.3.conv2.conv.weight", (16, 16, 3, 3, 3)), ("decoder.blocks.3.conv2.conv.bias", (16,)),
            ("decoder.blocks.4.conv.weight", (16, 1, 4, 4, 4)), ("decoder.blocks.4.conv.bias", (1,)),
            ("quantizer.quantizer.ema_cluster_size", (32,)), ("quantizer.quantizer.ema_w", (32, 8)),
            ("quantizer.quantizer.embedding.weight", (32, 8))]
    assert got == want
    q = net.quantizer.quantizer
    assert not q.embedding.weight.requires_grad and torch.equal(q.ema_w, q.embedding.weight) and bool((q.ema_cluster_size == 1).all())
    # the codebook and its EMA state are no optimizer state: not in the arena
    arena_names = {n for n, _, _ in net._entries}
    assert not any(n.startswith("quantizer") for n in arena_names) and len(arena_names) == len(want) - 3
    net.load_state_dict(ref.state_dict())
    ref.load_state_dict(net.state_dict())
    ku = VQVAE(**dict(SMALL, embedding_init="kaiming_uniform")).quantizer.quantizer.embedding.weight
    assert float(ku.abs().max()) <= math.sqrt(3.0 / 8) + 1e-6  # kaiming_uniform_(fan_in = 8, gain 1): bound sqrt(3 / fan_in)


def test_header_declares_the_quantiser_entries():
    from medical_image_generation_amd import _lib
    names = abi_header.names()
    new = {"mi_vq_assign", "mi_vq_gather_loss", "mi_vq_bwd", "mi_vq_ema_update", "mi_bias_act_bf16", "mi_fit_channels_bf16", "mi_axpy_dev_f32",
           "mi_l1_fwd_bwd_det", "mi_sumsq_det_f32", "mi_colsum_det_bf16", "mi_affine_dev_f32"}
    assert new <= names and new <= set(_lib.exported_symbols())
    import ctypes as C
    assert all(_lib.signature(n)[0] is C.c_int for n in new)
    c = _lib.constants()
    assert c["MI_ABI_VERSION"] == 20 and c["MI_CK_COUNT"] == 34
    assert (c["MI_VQ_PARTIALS"], c["MI_VQ_EMA_CHUNK"], c["MI_VQ_EMA_MAX_CHUNKS"]) == (1024, 1024, 256)
    from medical_image_generation_amd.vqvae import ema_workspace_bytes
    assert ema_workspace_bytes(1000, 37) == 8 + 4 * (37 + 74 + 1000) and ema_workspace_bytes(4099, 8) == 8 + 4 * (5 * 8 + 16 + 4099)
    assert ema_workspace_bytes(10 ** 6, 2) == 8 + 4 * (256 * 2 + 4 + 10 ** 6)


@pytest.mark.parametrize("shape", R.ASSIGN_SHAPES, ids=str)
def test_near_tie_share_of_the_gpu_inputs(shape):
    """The GPU assign test lets at most 1 % of tokens take the tolerance clause; the seeded inputs alone put at most 0.4 % of tokens
    within tau of a tie, and fp32 torch picks the fp64 argmin or a code within tau on all of them."""
    x, e = R.seeded_tokens(*shape)
    share = R.near_tie_share(x, e)
    assert share <= 0.004, share
    xd, ed = x.double(), e.double()
    d = (xd * xd).sum(1, keepdim=True) - 2 * xd @ ed.t() + (ed * ed).sum(1)[None]
    i32 = R.nearest_code(x.float(), e)
    assert bool((d.gather(1, i32[:, None])[:, 0] - d.min(1).values <= R.assign_tolerance(x, e)).all())


def test_more_than_one_rank_with_ddp_sync_is_refused(monkeypatch):
    """The all-reduce of the codebook counts and sums is not built: the trainer refuses at construction (before it touches a device),
    the module at the first training-mode quantisation."""
    import torch.distributed as dist
    from medical_image_generation_amd import trainer
    from medical_image_generation_amd.vqvae import VQVAE
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="ddp_sync"):
        trainer.VQAETrainer(VQVAE(**SMALL))
    net = VQVAE(**SMALL)
    net.train()
    monkeypatch.setattr("medical_image_generation_amd.vqvae.vq_assign", lambda z, cb: None)
    monkeypatch.setattr("medical_image_generation_amd.vqvae.vq_gather_loss", lambda *a: (None, None, None))
    with pytest.raises(NotImplementedError, match="ddp_sync"):
        net._quantize_cl(torch.zeros(1, 2, 2, 2, 8, dtype=torch.bfloat16))
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    with pytest.raises(TypeError):  # an inferer for VQ latents takes a VQVAE
        from medical_image_generation_amd.inferer import DDPMScheduler, VQLatentDiffusionInferer
        VQLatentDiffusionInferer(DDPMScheduler(), torch.nn.Identity())


def test_bf16_codes_flip_assignments_fp32_does_not():
    """Why the search is fp32: rounding the codes to bf16 (the tokens are bf16 already) moves the fp64 argmin of some of
    the seeded tokens, fp32 arithmetic moves none; and everything behind the index is discontinuous in it."""
    x, e = R.seeded_tokens(4096, 64, 512)
    exact = R.nearest_code(x.double(), e.double())
    flipped = int((R.nearest_code(x.double(), e.to(torch.bfloat16).double()) != exact).sum())
    print(f"\nbf16 codes flip {flipped} of 4096 assignments")
    assert flipped > 0 and bool((R.nearest_code(x.float(), e) == exact).all())
