"""The ResnetBlock skip conv fused with norm1 (csrc/conv1x1.hip, FUSE 1 / 2) against the separate passes it replaces.

Kernel level: mi_conv1x1_fwd_gn_apply against mi_gn_apply + the plan's forward, mi_conv1x1_dgrad_gn_bwd against the plan's data gradient +
mi_gn_bwd, on random bf16 data -- EQUAL BIT FOR BIT: both routes evaluate the same inline element function (csrc/gn_elem.h) on the same
bf16 operands in the same order, and xs / d_skip take the same MFMA sequence.  Block level: engine.resnet through blocks.ResnetBlock,
fused against unfused; bf16 tensors (y, dx) bit for bit, fp32 gradients (parameters, embedding) within the run-to-run noise of their
fp32-atomic reductions, measured in the same test by running the unfused route twice (as tests/test_checkpoint_gpu.py does)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
BF16 = torch.bfloat16

VOX_TILE = 32  # voxels per wave block of k_conv1x1 (one 32x32x16 MFMA column block); a workgroup takes 4 of them
# (N, dims): below one tile, exactly one, one + a ragged tail, and two images whose boundary (voxel 315) falls inside a tile -- the last
# one spans 20 tiles = 5 workgroups
SHAPES = [(1, (1, 3, 7)), (1, (1, 4, 8)), (1, (1, 5, 9)), (2, (5, 7, 9))]
assert [n * d * h * w for n, (d, h, w) in SHAPES[:3]] == [21, VOX_TILE, VOX_TILE + 13] and (5 * 7 * 9) % VOX_TILE != 0
# skip convs (Cin, Cout): 2, 3 and 6 input chunks; Cout > Cin = two cout blocks.  32 groups: 96 channels = 3 per group (an octet straddles groups)
CHANNELS = [(64, 32), (96, 32), (192, 64), (32, 64)]
GROUPS = 32


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rand(shape, gen, pitch=None, scale=1.0):
    """bf16 [N, D, H, W, C]; pitch: as the first C channels of a wider buffer (the skip-slot case of the encoder)"""
    c = shape[-1]
    full = (torch.randn(shape[:-1] + (pitch or c,), device=dev, generator=gen) * scale).to(BF16)
    return full[..., :c] if pitch else full


def _setup(n, dims, cin, cout, wide, seed):
    from medical_image_generation_amd import hipops as ops
    gen = torch.Generator(device=dev).manual_seed(seed)
    plan = ops.ConvPlan(n, dims, cin, cout, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    w = torch.randn((cout, cin, 1, 1, 1), device=dev, generator=gen) / cin ** 0.5
    plan.pack(w.contiguous())
    bias = torch.randn((cout,), device=dev, generator=gen)
    x = _rand((n,) + dims + (cin,), gen, pitch=cin + 32 if wide else None)
    gamma = 1.0 + 0.3 * torch.randn((cin,), device=dev, generator=gen)
    beta = 0.3 * torch.randn((cin,), device=dev, generator=gen)
    st = ops.gn_stats(x, GROUPS, 1e-6, gamma, beta)
    return ops, gen, plan, bias, x, gamma, st


@pytest.mark.parametrize("wide", [False, True], ids=["dense", "pitch"])
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("n,dims", SHAPES)
def test_forward_equals_apply_plus_conv(n, dims, cin, cout, wide):
    ops, gen, plan, bias, x, gamma, st = _setup(n, dims, cin, cout, wide, 11)
    assert ops.skip_fusable(1, plan, x)
    a1_ref = ops.gn_apply(x, st, True)
    xs_ref = plan.fwd(x, addvec=bias)
    assert plan.last_kernel() == 17  # MI_CK_1X1_STREAM: the reference is today's route
    xs, a1 = ops.conv1x1_fwd_gn_apply(plan, x, st, bias)
    torch.cuda.synchronize()
    assert a1.is_contiguous() and xs.is_contiguous()
    assert torch.equal(_bits(xs), _bits(xs_ref))
    assert torch.equal(_bits(a1), _bits(a1_ref))


@pytest.mark.parametrize("with_add2", [False, True], ids=["noadd2", "add2"])
@pytest.mark.parametrize("wide", [False, True], ids=["dense", "pitch"])
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("n,dims", SHAPES)
def test_backward_equals_dgrad_plus_gn_bwd(n, dims, cin, cout, wide, with_add2):
    ops, gen, plan, bias, x, gamma, st = _setup(n, dims, cin, cout, wide, 12)
    dout = _rand((n,) + dims + (cout,), gen, scale=0.5)
    g = _rand((n,) + dims + (cin,), gen, pitch=cin + 8 if wide else None, scale=0.5)  # g1 with its own pitch
    add2 = _rand((n,) + dims + (cin,), gen, pitch=2 * cin if wide else None, scale=0.5) if with_add2 else None
    assert ops.skip_fusable(2, plan, dout, g, x, add2)
    dg_ref, db_ref = torch.zeros(cin, device=dev), torch.zeros(cin, device=dev)
    d_skip = plan.dgrad(dout)
    assert plan.last_kernel() == 17
    # the tape queues the skip gradient last: (other branch, d_skip) -> add, add2
    dx_ref = ops.gn_bwd(g, x, st, gamma, True, dg_ref, db_ref, add=add2, add2=d_skip)
    dg, db = torch.zeros(cin, device=dev), torch.zeros(cin, device=dev)
    dx = ops.conv1x1_dgrad_gn_bwd(plan, dout, g, x, st, gamma, dg, db, add2=add2)
    torch.cuda.synchronize()
    assert dx.is_contiguous() and torch.equal(_bits(dx), _bits(dx_ref))
    # same partial / finalize launches on the same operands; at most two images add into a zeroed slot: order-free
    assert torch.equal(dg, dg_ref) and torch.equal(db, db_ref)


def _block_pass(blk, x, emb, gy):
    x = x.clone().requires_grad_(True)
    emb = emb.clone().requires_grad_(True)
    for p in blk.parameters():
        p.grad = None
    y = blk(x, emb)
    y.backward(gy)
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in blk.named_parameters() if p.grad is not None}
    return y.detach().clone(), x.grad.clone(), emb.grad.clone(), grads


def _blocks(cin, cout, seed, **kw):
    from medical_image_generation_amd.blocks import ResnetBlock
    torch.manual_seed(seed)
    a = ResnetBlock(3, cin, 64, cout, norm_num_groups=GROUPS, **kw)
    for p in a.parameters():  # (conv2 is zero-initialised: give every path signal)
        if float(p.detach().abs().max()) == 0:
            torch.nn.init.normal_(p, std=0.05)
    b = ResnetBlock(3, cin, 64, cout, norm_num_groups=GROUPS, **kw)
    b.load_state_dict(a.state_dict())
    return a.to(dev), b.to(dev)


@pytest.mark.parametrize("cin,cout,dims", [(64, 32, (8, 8, 8)), (32, 64, (6, 10, 12))])
def test_resnet_block_fused_equals_unfused(cin, cout, dims):
    from medical_image_generation_amd import _lib
    fused, plain = _blocks(cin, cout, 5)
    plain.fuse_skip = False
    gen = torch.Generator(device=dev).manual_seed(6)
    x = torch.randn((2, cin) + dims, device=dev, generator=gen)
    emb = torch.randn((2, 64), device=dev, generator=gen)
    gy = torch.randn((2, cout) + dims, device=dev, generator=gen)
    with _lib.profile_calls() as prof:
        y_f, dx_f, de_f, gr_f = _block_pass(fused, x, emb, gy)
    called = prof.summary()
    assert "mi_conv1x1_fwd_gn_apply" in called and "mi_conv1x1_dgrad_gn_bwd" in called and "mi_conv_dgrad" in called  # (conv1 / conv2's)
    y_a, dx_a, de_a, gr_a = _block_pass(plain, x, emb, gy)
    y_b, dx_b, de_b, gr_b = _block_pass(plain, x, emb, gy)
    assert torch.equal(y_f, y_a) and torch.equal(dx_f, dx_a)  # fp32 images of bf16 tensors
    assert sorted(gr_f) == sorted(gr_a) and {"norm1.weight", "norm1.bias", "skip_connection.conv.weight", "skip_connection.conv.bias"} <= set(gr_f)
    rel = lambda u, v: float((u.double() - v.double()).norm() / (v.double().norm() + 1e-30))
    worst = {}
    for k in list(gr_a) + ["d_emb"]:
        a, b, f = (de_a, de_b, de_f) if k == "d_emb" else (gr_a[k], gr_b[k], gr_f[k])
        noise, err = rel(b, a), rel(f, a)
        worst[k] = (err, noise)
        assert err <= max(4 * noise, 1e-6), (k, err, noise)
    print("\n[resnet %d->%d %s] fp32 gradients, fused vs unfused (unfused vs unfused): " % (cin, cout, dims) +
          "  ".join(f"{k} {e:.1e} ({n:.1e})" for k, (e, n) in worst.items()))


def test_ineligible_blocks_take_the_separate_passes():
    """Cin = 512 (the skip conv runs on the GEMM route) and a resampling block: none of the fused entry points, all of the separate ones."""
    from medical_image_generation_amd import _lib
    gen = torch.Generator(device=dev).manual_seed(8)
    for cin, cout, dims, kw in [(512, 256, (4, 4, 4), {}), (64, 32, (4, 4, 4), dict(up=True, stride=2))]:
        blk, _ = _blocks(cin, cout, 7, **kw)
        x = torch.randn((1, cin) + dims, device=dev, generator=gen)
        emb = torch.randn((1, 64), device=dev, generator=gen)
        with _lib.profile_calls() as prof:
            y = blk(x.requires_grad_(True), emb)
            y.backward(torch.randn(y.shape, device=dev, generator=gen))
        called = prof.summary()
        assert "mi_conv1x1_fwd_gn_apply" not in called and "mi_conv1x1_dgrad_gn_bwd" not in called, sorted(called)
        assert {"mi_gn_apply", "mi_conv_fwd", "mi_conv_dgrad", "mi_gn_bwd"} <= set(called), sorted(called)
