"""LPIPS-VGG perceptual loss on the HIP path (perceptual.py, csrc/perceptual.hip) against the torch fp32 restatement in
tests/perc_ref.py, random weights (He-normal convs, non-negative heads): kernels, the 2-D and fake-3D loss and input gradient, and the
AETrainer / AEGANTrainer generator step with the native term against the same step with the restatement as `extra_loss`."""
import copy

import pytest
import torch
import torch.nn.functional as F

from oracle import cases, nets, synth
from tests import perc_ref

pytestmark = pytest.mark.gpu
S = cases.SEED
BF16 = torch.bfloat16


def _ptr(t):
    return None if t is None else t.data_ptr()


def _perc(spatial_dims, seed=3, ratio=0.2):
    from medical_image_generation_amd.perceptual import PerceptualLoss
    torch.manual_seed(seed)
    return PerceptualLoss(spatial_dims=spatial_dims, network_type="vgg", is_fake_3d=True, fake_3d_ratio=ratio, pretrained=False).cuda()


def _cmp(name, got, want):
    cos = float(F.cosine_similarity(got.flatten().double(), want.flatten().double(), dim=0))
    rel = float((got.double() - want.double()).norm() / want.double().norm())
    print(f"  {name}: cosine {cos:.5f}, rel-L2 {rel:.4f}")
    return cos, rel


# ---------------------------------------------------------------------------------------------------------------- kernels
def test_relu_maxpool_fwd_bwd_with_ties():
    from medical_image_generation_amd._lib import call
    torch.manual_seed(0)
    n, h, w, c = 3, 7, 10, 16  # odd height: the last row is rectified but belongs to no pooling window
    z = torch.randint(-2, 3, (n, 1, h, w, c)).to(BF16)  # small integers: ties inside most windows, many zeros
    zc = z.float().squeeze(1).permute(0, 3, 1, 2).clone().requires_grad_(True)
    a_ref = F.relu(zc)
    p_ref = F.max_pool2d(a_ref, 2, 2)
    dp = torch.randn(p_ref.shape)
    dadd = torch.randn(a_ref.shape)
    ((p_ref * dp).sum() + (a_ref * dadd).sum()).backward()
    a = z.cuda()
    p = torch.empty((n, 1, h // 2, w // 2, c), dtype=BF16, device="cuda")
    call("mi_relu_maxpool2_fwd", _ptr(a), _ptr(p), n, h, w, c)
    cl = lambda t: t.permute(0, 2, 3, 1).unsqueeze(1)
    assert torch.equal(a.cpu().float(), cl(a_ref.detach()))
    assert torch.equal(p.cpu().float(), cl(p_ref.detach()))
    dp_cl = cl(dp).to(BF16).contiguous().cuda()
    dadd_cl = cl(dadd).to(BF16).contiguous().cuda()
    dz = torch.empty_like(a)
    call("mi_relu_maxpool2_bwd", _ptr(a), _ptr(dp_cl), _ptr(dadd_cl), _ptr(dz), n, h, w, c)
    # reference with the bf16-rounded upstream gradients, routed by torch (first maximum of a window)
    zc.grad = None
    a_ref = F.relu(zc)
    ((F.max_pool2d(a_ref, 2, 2) * dp_cl.cpu().float().squeeze(1).permute(0, 3, 1, 2)).sum() +
     (a_ref * dadd_cl.cpu().float().squeeze(1).permute(0, 3, 1, 2)).sum()).backward()
    assert torch.allclose(dz.cpu().float(), cl(zc.grad), atol=1e-2, rtol=1e-2)
    # ReLU backward alone (dpooled NULL), in place
    g = dadd_cl.clone()
    call("mi_relu_maxpool2_bwd", _ptr(a), None, _ptr(g), _ptr(g), n, h, w, c)
    assert torch.equal(g.cpu().float(), dadd_cl.cpu().float() * (a.cpu().float() > 0))


@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_lpips_head_fwd_bwd(c):
    from medical_image_generation_amd._lib import call
    torch.manual_seed(c)
    s, p = 3, 37
    f0 = F.relu(torch.randn(s, p, c)).to(BF16)
    f1 = F.relu(torch.randn(s, p, c)).to(BF16)
    f0[1, 5].zero_()  # an all-zero feature vector: finite gradient
    w = torch.rand(c) * 0.1
    weight = 0.7
    x = f0.float().clone().requires_grad_(True)
    y = f1.float()
    nx = x / (torch.sqrt((x ** 2).sum(-1, keepdim=True)) + 1e-10)
    ny = y / (torch.sqrt((y ** 2).sum(-1, keepdim=True)) + 1e-10)
    ref = weight * (((nx - ny) ** 2) * w).sum(-1).mean()
    ref.backward()
    loss = torch.full((1,), 0.25, device="cuda")  # accumulates
    df = torch.empty((s, p, c), dtype=BF16, device="cuda")
    f0d, f1d, wd = f0.cuda(), f1.cuda(), w.cuda()
    call("mi_lpips_head", _ptr(f0d), _ptr(f1d), _ptr(wd), s, p, c, weight, 1e-10, _ptr(loss), _ptr(df))
    assert abs(float(loss) - 0.25 - float(ref)) <= 1e-4 * abs(float(ref))
    gref = x.grad.clone()
    gref[1, 5] = df.cpu().float()[1, 5]  # (torch: 0 * inf there)
    assert torch.isfinite(df.float()).all()
    assert torch.allclose(df.cpu().float()[1, 5], (2 * weight / (s * p)) * w * (-y[1, 5] / (y[1, 5].norm() + 1e-10)) / 1e-10, rtol=2e-2)
    cos, rel = _cmp(f"head C={c}", df.cpu().float(), gref)
    assert cos >= 0.9999 and rel <= 1e-2


def test_gather_scatter_adjoint_pair():
    """<G x, y> = <x, G^T y> for the linear part of the gather (the scaling layer's shift removed), all three axes, 1 and 3 channels;
    and the gathered values equal upstream's permute / index_select slicing."""
    from medical_image_generation_amd._lib import call
    from medical_image_generation_amd.perceptual import _SCALE, _SHIFT
    torch.manual_seed(1)
    shift, scale = torch.tensor(_SHIFT).cuda(), torch.tensor(_SCALE).cuda()
    for c in (1, 3):
        n, d, h, w = 2, 5, 6, 7
        x = torch.randn(n, d, h, w, c).to(BF16).cuda()
        zero = torch.zeros_like(x)
        for axis in range(3):
            ext = (d, h, w)[axis]
            idx = torch.randperm(n * ext)[: n * ext - 3].to(torch.int32).cuda()
            ns = idx.numel()
            a, b = [(h, w), (d, w), (d, h)][axis]
            gx, g0 = (torch.empty((ns, 1, a, b, 8), dtype=BF16, device="cuda") for _ in range(2))
            for src, dst in ((x, gx), (zero, g0)):
                call("mi_perc_gather", _ptr(src), c, c, n, d, h, w, axis, _ptr(idx), ns, _ptr(shift), _ptr(scale), _ptr(dst))
            # upstream slicing of the NCDHW volume
            ref = perc_ref.slices(x.float().permute(0, 4, 1, 2, 3), axis + 2).index_select(0, idx.long())
            ref = ((ref.expand(-1, 3, -1, -1) - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1)).permute(0, 2, 3, 1)
            assert torch.allclose(gx.float()[:, 0, :, :, :3], ref, rtol=1e-2, atol=1e-2)
            assert torch.equal(gx.float()[..., 3:], torch.zeros_like(gx.float()[..., 3:]))
            y = torch.randn(ns, 1, a, b, 8).to(BF16).cuda()
            gty = torch.zeros_like(x)
            call("mi_perc_scatter_add", _ptr(y), axis, _ptr(idx), ns, n, d, h, w, c, _ptr(scale), _ptr(gty), c)
            lhs = float(((gx.double() - g0.double())[..., :3] * y.double()[..., :3]).sum())
            rhs = float((x.double() * gty.double()).sum())
            assert abs(lhs - rhs) <= 2e-2 * (abs(lhs) + 1e-3), (c, axis, lhs, rhs)


# ---------------------------------------------------------------------------------------------------------------- loss parity
def test_lpips_2d_loss_and_input_gradient():
    m = _perc(2)
    torch.manual_seed(11)
    x = torch.rand(4, 1, 64, 64, device="cuda").requires_grad_(True)
    y = torch.rand(4, 1, 64, 64, device="cuda")
    loss = m(x, y)
    loss.backward()
    xr = x.detach().clone().requires_grad_(True)
    ref = perc_ref.perceptual(m, xr, y)
    ref.backward()
    rl = abs(float(loss) - float(ref)) / abs(float(ref))
    print(f"\n[LPIPS 2-D] loss {float(loss):.6f} vs {float(ref):.6f} (rel {rl:.2e})")
    cos, rel = _cmp("d input", x.grad, xr.grad)
    # measured on MI355X: loss rel 3.9e-4, cosine 0.9894, rel-L2 0.146 -- the bf16 floor: the same torch network with its activations
    # rounded to bf16 reaches cosine 0.989 against fp32 too (uniform-noise images through 13 ReLU / max-pool layers)
    assert rl <= 6e-4 and cos >= 0.984 and rel <= 0.22


def test_fake3d_loss_and_input_gradient_fixed_indices():
    m = _perc(3)
    x = synth.ellipsoid_volume(S, "x", (2, 1, 32, 32, 32)).cuda()
    y = (x + 0.1 * torch.randn_like(x)).clamp(0, 1)
    idx = m.draw_indices(tuple(x.shape), generator=torch.Generator().manual_seed(5))
    assert [len(i) for i in idx] == [12, 12, 12]
    xh = x.clone().requires_grad_(True)
    loss = m(xh, y, indices=idx)
    loss.backward()
    xr = x.clone().requires_grad_(True)
    ref = perc_ref.perceptual(m, xr, y, idx)
    ref.backward()
    rl = abs(float(loss) - float(ref)) / abs(float(ref))
    print(f"\n[LPIPS fake 3-D] loss {float(loss):.6f} vs {float(ref):.6f} (rel {rl:.2e})")
    cos, rel = _cmp("d input", xh.grad, xr.grad)
    assert rl <= 2e-3 and cos >= 0.995 and rel <= 0.12  # measured: 1.2e-3, 0.9970, 0.078
    # voxels of no selected slice get no gradient; the default call draws on the CPU generator like upstream
    torch.manual_seed(9)
    a = float(m(x, y))
    torch.manual_seed(9)
    assert abs(a - float(perc_ref.perceptual(m, x, y, m.draw_indices(tuple(x.shape))))) <= 3e-2 * abs(a)


# ---------------------------------------------------------------------------------------------------------------- trainers
def _ae():
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    c = cases.AEKL_CASES["aekl_c3a"]
    ref = nets.AutoencoderKL(**c["kwargs"])
    sd0 = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    ref.load_state_dict(sd0)
    with torch.no_grad():
        zshape = tuple(ref.encode(synth.ellipsoid_volume(S, "x", c["shape"]))[0].shape)
    net = AutoencoderKL(**c["kwargs"])
    net.load_state_dict(sd0)
    return net.cuda(), sd0, c["shape"], zshape


def _flat(net, names):
    return torch.cat([net.state_dict()[n].float().cpu().flatten() for n in names])


@pytest.mark.parametrize("graph", [False, True])
def test_ae_step_native_perceptual_matches_extra_loss_restatement(graph):
    from medical_image_generation_amd.trainer import AETrainer
    pw = 2.0
    m = _perc(3)
    x = synth.ellipsoid_volume(S, "x", (1, 1, 32, 32, 32)).cuda()
    idx = m.draw_indices(tuple(x.shape), generator=torch.Generator().manual_seed(2))
    results = {}
    for mode in ("native", "extra"):
        net, sd0, shape, zshape = _ae()
        eps = synth.tensor(S, "eps0", zshape).cuda()
        names = [n for n in sd0 if n in dict(net.named_parameters())]
        if mode == "native":
            tr = AETrainer(net, lr=cases.STEP_LR, kl_weight=1e-3, perceptual=m, perc_weight=pw)
        else:
            tr = AETrainer(net, lr=cases.STEP_LR, kl_weight=1e-3,
                           extra_loss=lambda rec, img: pw * perc_ref.perceptual(m, rec, img, idx))
        if graph and mode == "native":
            tr.capture(x, eps, perc_indices=idx)
            loss = float(tr.step_graph(x, eps, perc_indices=idx))
        else:
            loss = float(tr.step(x, eps, perc_indices=idx) if mode == "native" else tr.step(x, eps))
        results[mode] = (loss, _flat(net, names) - torch.cat([sd0[n].float().flatten() for n in names]),
                         float(tr.perc_loss) if mode == "native" else float(tr.extra_loss_value))
    (ln, un, pn), (le, ue, pe) = results["native"], results["extra"]
    cos = float(torch.dot(un, ue) / (un.norm() * ue.norm()))
    ratio = float(un.norm() / ue.norm())
    print(f"\n[AE + perceptual graph={graph}] loss {ln:.5f} vs {le:.5f}; perc term {pn:.5f} vs {pe:.5f}; update cosine {cos:.4f} ratio {ratio:.3f}")
    assert pn > 0.05 * ln  # the term matters in this set-up
    # measured: loss rel 6e-6, perceptual term rel 9e-5, update cosine 0.9928, norm ratio 1.000
    assert abs(ln - le) <= 2e-2 * abs(le) and abs(pn - pe) <= 3e-4 * abs(pe)
    assert cos >= 0.989 and abs(ratio - 1) <= 0.05


def test_replay_uses_fresh_indices():
    """Indices are a graph INPUT: two replays with different indices give different perceptual terms, each equal to the eager step's
    value for the same indices (lr = 0: the autoencoder does not move between the steps)."""
    from medical_image_generation_amd.trainer import AETrainer
    m = _perc(3)
    net, sd0, shape, zshape = _ae()
    x = synth.ellipsoid_volume(S, "x", shape).cuda()
    eps = synth.tensor(S, "eps0", zshape).cuda()
    tr = AETrainer(net, lr=0.0, kl_weight=1e-3, perceptual=m, perc_weight=1.0)
    gen = torch.Generator().manual_seed(8)
    i1, i2, i3 = (m.draw_indices(tuple(x.shape), generator=gen) for _ in range(3))
    eager = []
    for idx in (i2, i3):
        tr.step(x, eps, perc_indices=idx)
        eager.append(float(tr.perc_loss))
    tr.capture(x, eps, perc_indices=i1)
    replay = []
    for idx in (i2, i3):
        tr.step_graph(perc_indices=idx)
        replay.append(float(tr.perc_loss))
    print(f"\n[replay indices] eager {eager} replay {replay}")
    # measured: the two index sets differ by 8e-4 relative, replay and eager agree to 2e-7 (atomic summation order)
    assert abs(eager[0] - eager[1]) > 1e-4 * abs(eager[0])
    for e, r in zip(eager, replay):
        assert abs(e - r) <= 1e-5 * abs(e)
    # a replay without indices draws fresh ones on the CPU generator
    torch.manual_seed(21)
    tr.step_graph()
    torch.manual_seed(21)
    want = m.draw_indices(tuple(x.shape))
    assert all(torch.equal(b.cpu().long(), w) for b, w in zip(tr._perc_idx, want))


def test_perceptual_net_is_frozen():
    from medical_image_generation_amd import _lib
    from medical_image_generation_amd.trainer import AETrainer
    m = _perc(3)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = synth.ellipsoid_volume(S, "x", (1, 1, 32, 32, 32)).cuda()
    idx = [i.to(torch.int32).cuda() for i in m.draw_indices(tuple(x.shape))]
    from medical_image_generation_amd import hipops as ops
    x_cl = ops.to_channels_last(x)
    loss = torch.zeros(1, device="cuda")
    with _lib.profile_calls() as prof:
        g = m.hip(x_cl, ops.to_channels_last((x * 0.9).contiguous()), idx, loss, 1.0)
    names = set(prof.summary())
    print(f"\n[frozen VGG] entry points {sorted(names)}")
    assert "mi_conv_dgrad" in names and "mi_conv_fwd" in names
    assert not any("wgrad" in n for n in names)
    assert float(loss) > 0 and torch.isfinite(g.float()).all()
    net, sd0, shape, zshape = _ae()
    tr = AETrainer(net, lr=cases.STEP_LR, perceptual=m)
    tr.step(x, synth.tensor(S, "eps0", zshape).cuda())
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_aegan_step_with_perceptual_term():
    from medical_image_generation_amd.discriminator import PatchDiscriminator
    from medical_image_generation_amd.trainer import AEGANTrainer
    m = _perc(3)
    net, sd0, shape, zshape = _ae()
    torch.manual_seed(0)
    D = PatchDiscriminator(spatial_dims=3, num_channels=8, in_channels=1).cuda()
    d0 = {k: v.clone() for k, v in D.state_dict().items()}
    x = synth.ellipsoid_volume(S, "x", shape).cuda()
    eps = synth.tensor(S, "eps0", zshape).cuda()
    tr = AEGANTrainer(net, D, adversarial=True, perceptual=m, perc_weight=0.125)
    names = [n for n in sd0 if n in dict(net.named_parameters())]
    before = _flat(net, names)
    loss = float(tr.step(x, eps))
    print(f"\n[AEGAN + perceptual] loss {loss:.5f} perc {float(tr.perc_loss):.5f} gen {float(tr.gen_loss):.5f} disc {float(tr.disc_loss):.5f}")
    assert all(map(lambda v: torch.isfinite(torch.tensor(v)), (loss, float(tr.perc_loss), float(tr.gen_loss), float(tr.disc_loss))))
    assert float(tr.perc_loss) > 0
    assert float((_flat(net, names) - before).abs().max()) > 0
    assert any(not torch.equal(v, d0[k]) for k, v in D.state_dict().items() if v.is_floating_point())
