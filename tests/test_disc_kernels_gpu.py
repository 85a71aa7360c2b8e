"""Kernel-level parity of the PatchDiscriminator path (csrc/disc.hip and the GroupNorm kernels in their BatchNorm role) against plain
torch references on the CPU, computed in fp32 / fp64 from the same bf16-rounded inputs.

The whole-network checks in test_discriminator_gpu.py run one small shape through four bf16 layers, so their budget is loose.  Here
every op gets its own input and its own tight budget, at the planner's shapes (PatchDiscriminator(num_channels=64, num_layers_d=3) on
2 x 1 x 128^3 patches: the data-movement kernels loop over their grid cap there) and at odd / anisotropic / strided edges.
Data movement is compared bit for bit; the library's standard for a bf16-output op is |err| <= 1e-2 * max|ref|, and no budget here
is looser than that."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

dev = torch.device("cuda")
BF16 = torch.bfloat16
U = 2.0 ** -8  # one bf16 rounding (round to nearest: at most half of this, relative)


@pytest.fixture(scope="module")
def lib():
    from medical_image_generation_amd import _lib
    _lib.load()
    return _lib


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).bfloat16().float()  # bf16-representable fp32


def check(got, ref, tol=1e-2, what=""):
    scale = float(ref.abs().max()) + 1e-12
    err = float((got - ref).abs().max())
    assert math.isfinite(err) and err <= tol * scale, f"{what}: max err {err:.4g} vs scale {scale:.4g}"


def nan_bf16(*shape):
    return torch.full(shape, float("nan"), dtype=BF16, device=dev)


def out_extent(v, k, s, p):
    return (v + 2 * p - k) // s + 1


# ----------------------------------------------------------------------------------------------------------- im2col / col2im
def im2col_ref(x, k, s, p):
    """x [N, D, H, W, C] -> patches [N*Do*Ho*Wo, k^3 * C] (tap-major, channel-minor; zero outside the tensor): a gather from the
    zero-padded tensor."""
    xp = F.pad(x, (0, 0, p, p, p, p, p, p))
    u = xp.unfold(1, k, s).unfold(2, k, s).unfold(3, k, s)  # [N, Do, Ho, Wo, C, k, k, k]
    n, do, ho, wo, c = u.shape[:5]
    return u.permute(0, 1, 2, 3, 5, 6, 7, 4).reshape(n * do * ho * wo, k * k * k * c)


def col2im_ref(pt, shape, k, s, p):
    """The adjoint of im2col_ref in the dtype of `pt`: every patch entry scatter-added onto the input voxel it was read from."""
    n, d, h, w, c = shape
    do, ho, wo = (out_extent(v, k, s, p) for v in (d, h, w))
    pv = pt.view(n, do, ho, wo, k, k, k, c)
    acc = torch.zeros((n, d + 2 * p, h + 2 * p, w + 2 * p, c), dtype=pt.dtype)
    for td in range(k):
        for th in range(k):
            for tw in range(k):
                acc[:, td:td + s * (do - 1) + 1:s, th:th + s * (ho - 1) + 1:s, tw:tw + s * (wo - 1) + 1:s] += pv[:, :, :, :, td, th, tw]
    return acc[:, p:p + d, p:p + h, p:p + w]


IM2COL_CASES = [
    # (N, (D, H, W), C, x channel stride, k, s, p)
    (2, (8, 8, 8), 1, 1, 4, 2, 1),        # the image: one channel, scalar path
    (2, (7, 9, 6), 2, 2, 4, 1, 1),        # two channels, scalar path, odd / anisotropic, stride 1
    (2, (9, 6, 11), 16, 16, 4, 2, 1),     # vector path
    (2, (5, 7, 6), 64, 64, 4, 1, 1),      # vector path, the planner's width
    (2, (9, 8, 7), 16, 24, 3, 2, 0),      # k3 s2 p0, channel stride > C (vector: both multiples of 8)
    (2, (6, 5, 7), 16, 20, 4, 2, 1),      # C % 8 == 0 but x_cs % 8 != 0: must take the scalar path
    (1, (5, 6, 7), 2, 3, 4, 1, 1),        # scalar path with a channel stride > C
    (2, (128, 128, 128), 1, 1, 4, 2, 1),  # the planner's first layer: 33.5 M (voxel, tap) threads, beyond the grid cap
]


def _ids(c):
    return f"n{c[0]}_{'x'.join(map(str, c[1]))}_c{c[2]}cs{c[3]}_k{c[4]}s{c[5]}p{c[6]}"


@pytest.mark.parametrize("case", IM2COL_CASES, ids=_ids)
def test_im2col_matches_gather(lib, case):
    """Pure data movement: bit-exact against the gather (the output is pre-filled with NaN, so an unwritten entry fails too)."""
    n, (d, h, w), c, xcs, k, s, p = case
    xw = rnd(n, d, h, w, xcs, seed=1)
    do, ho, wo = (out_extent(v, k, s, p) for v in (d, h, w))
    pt = nan_bf16(n * do * ho * wo, k ** 3 * c)
    lib.call("mi_im2col3d", lib.ptr(xw.to(dev, BF16)), xcs, lib.ptr(pt), n, d, h, w, c, k, s, p)
    ref = im2col_ref(xw[..., :c], k, s, p).to(BF16)
    assert torch.equal(pt.cpu(), ref)


COL2IM_CASES = [
    # (N, (D, H, W), C, dx channel stride, k, s, p)
    (2, (8, 8, 8), 1, 1, 4, 2, 1),
    (2, (7, 9, 6), 2, 3, 4, 1, 1),        # scalar path, dx_cs > C
    (2, (9, 6, 11), 16, 24, 4, 2, 1),     # vector path, dx_cs > C
    (1, (5, 7, 6), 64, 64, 4, 1, 1),      # 64 taps read every interior voxel
    (2, (8, 10, 6), 16, 16, 3, 2, 0),     # k3 s2 p0 on even extents: the last row / column / plane is read by no window
    (1, (8, 6, 10), 2, 2, 3, 2, 0),       # the same on the scalar path
    (2, (128, 128, 128), 1, 1, 4, 2, 1),  # the data gradient of the planner's first layer: 4.2 M threads, beyond the grid cap
]


@pytest.mark.parametrize("case", COL2IM_CASES, ids=_ids)
def test_col2im_matches_scatter_add(lib, case):
    """mi_col2im3d against the fp64 scatter-add of the same bf16 patches.  Per element: one bf16 rounding of the output (2^-8 of the
    value) plus fp32 accumulation of at most k^3 terms (k^3 * 2^-24 of the sum of their magnitudes, worst case).  Unread voxels must be exactly 0,
    channels >= C of a wider dx untouched (the buffer is pre-filled with NaN).  The adjoint identity <im2col(x), P> = <x, col2im(P)>
    ties the two kernels' tap orders together, in fp64 from the kernels' own outputs: its budget is the same per-element bound summed."""
    n, (d, h, w), c, dcs, k, s, p = case
    do, ho, wo = (out_extent(v, k, s, p) for v in (d, h, w))
    m, kk = n * do * ho * wo, k ** 3 * c
    pt = rnd(m, kk, seed=2)
    dx = nan_bf16(n, d, h, w, dcs)
    lib.call("mi_col2im3d", lib.ptr(pt.to(dev, BF16)), lib.ptr(dx), dcs, n, d, h, w, c, k, s, p)
    dx = dx.cpu()
    assert torch.isnan(dx[..., c:]).all(), "col2im wrote channels beyond C"
    got = dx[..., :c].double()
    ref = col2im_ref(pt.double(), (n, d, h, w, c), k, s, p)
    mag = col2im_ref(pt.abs().double(), (n, d, h, w, c), k, s, p)
    bound = U * ref.abs() + (1 + U) * k ** 3 * 2.0 ** -24 * mag
    assert torch.isfinite(got).all()
    assert bool(((got - ref).abs() <= bound).all()), f"max err {float((got - ref).abs().max()):.4g}"
    for axis, (v, vo) in enumerate(zip((d, h, w), (do, ho, wo))):  # the trailing planes no window reads (k3 s2 p0 on even extents)
        last = (vo - 1) * s + k - 1 - p
        if last + 1 < v:
            assert bool((got.narrow(axis + 1, last + 1, v - last - 1) == 0).all()), f"unread planes of axis {axis} not zero"
    if n * d * h * w <= 4096:  # adjoint identity (the small cases: the fp64 dot products are cheap)
        x = rnd(n, d, h, w, c, seed=3)
        pg = torch.empty((m, kk), dtype=BF16, device=dev)
        lib.call("mi_im2col3d", lib.ptr(x.to(dev, BF16)), c, lib.ptr(pg), n, d, h, w, c, k, s, p)
        lhs = float((pg.cpu().double() * pt.double()).sum())
        rhs = float((x.double() * got).sum())
        budget = float((x.double().abs() * bound).sum())
        assert abs(lhs - rhs) <= budget, f"<im2col(x), P> {lhs:.6g} != <x, col2im(P)> {rhs:.6g}"


# ----------------------------------------------------------------------------------------------------------- weight packing
@pytest.mark.parametrize("co,cop,ci,k", [(64, 64, 1, 4), (128, 128, 64, 4), (1, 8, 512, 4), (3, 8, 5, 3), (20, 24, 7, 4)])
def test_disc_pack_weights_and_wgrad_unpack(lib, co, cop, ci, k):
    """Pure data movement, bit-exact: w2 = the bf16 weight with the taps as the slow K axis, w2t its transpose, padded rows zero; the
    unpack accumulates (one fp32 add per element, the same add torch makes)."""
    taps = k ** 3
    w = torch.randn(co, ci, k, k, k, generator=torch.Generator().manual_seed(co * 1000 + ci))
    w2, w2t = nan_bf16(cop, taps * ci), nan_bf16(taps * ci, cop)
    lib.call("mi_disc_pack_weights", lib.ptr(w.to(dev)), lib.ptr(w2), lib.ptr(w2t), co, cop, ci, taps)
    ref = torch.zeros(cop, taps * ci, dtype=BF16)
    ref[:co] = w.bfloat16().permute(0, 2, 3, 4, 1).reshape(co, taps * ci)
    w2, w2t = w2.cpu(), w2t.cpu()
    assert torch.equal(w2, ref)
    assert torch.equal(w2t, ref.t().contiguous())
    assert bool((w2[co:] == 0).all()) and bool((w2t[:, co:] == 0).all())
    dw2 = torch.randn(cop, taps * ci, generator=torch.Generator().manual_seed(7))
    dw0 = torch.randn(co, ci, k, k, k, generator=torch.Generator().manual_seed(8))
    dw = dw0.to(dev)
    lib.call("mi_disc_wgrad_unpack", lib.ptr(dw2.to(dev)), lib.ptr(dw), co, ci, taps)
    want = dw0 + dw2[:co].view(co, k, k, k, ci).permute(0, 4, 1, 2, 3)
    assert torch.equal(dw.cpu(), want)


# ----------------------------------------------------------------------------------------------------------- LeakyReLU
def _leaky_inputs(n, seed):
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed)).bfloat16()
    special = torch.tensor([0.0, -0.0, 2.0 ** -126, -(2.0 ** -126), 2.0 ** -133, -(2.0 ** -133), 1e-30, -1e-30, 1e-38, -1e-38,
                            3e-39, -3e-39, 1.0, -1.0, 65504.0, -65504.0], dtype=torch.float32).bfloat16()
    x[:special.numel()] = special
    return x


@pytest.mark.parametrize("n", [16, 8 * 1001, 2 * 64 ** 3 * 64])  # the last: the planner's first activation, 16 M threads of 8 (grid cap)
@pytest.mark.parametrize("slope", [0.2, 0.05])
def test_leaky_relu_fwd_bwd_bit_exact(lib, n, slope):
    """F.leaky_relu and its autograd in fp32 on the same bf16 values, rounded once to bf16: the kernel makes the same one product
    and one rounding, so every bit must match (signed zeros and the subnormal products of tiny inputs included)."""
    x = _leaky_inputs(n, 1)
    dy = _leaky_inputs(n, 2).flip(0)
    xd, dyd = x.to(dev), dy.to(dev)
    y, dx = torch.empty_like(xd), torch.empty_like(xd)
    lib.call("mi_leaky_relu_fwd", lib.ptr(xd), lib.ptr(y), n, float(slope))
    lib.call("mi_leaky_relu_bwd", lib.ptr(xd), lib.ptr(dyd), lib.ptr(dx), n, float(slope))
    xr = x.float().requires_grad_(True)
    yr = F.leaky_relu(xr, slope)
    yr.backward(dy.float())
    assert torch.equal(y.cpu().view(torch.int16), yr.detach().bfloat16().view(torch.int16)), "forward"
    assert torch.equal(dx.cpu().view(torch.int16), xr.grad.bfloat16().view(torch.int16)), "backward"


def test_leaky_relu_rejects_ragged_length(lib):
    x = torch.zeros(24, dtype=BF16, device=dev)
    with pytest.raises(lib.HipError):
        lib.call("mi_leaky_relu_fwd", lib.ptr(x), lib.ptr(x), 12, 0.2)
    with pytest.raises(lib.HipError):
        lib.call("mi_leaky_relu_bwd", lib.ptr(x), lib.ptr(x), lib.ptr(x), 20, 0.2)


# ----------------------------------------------------------------------------------------------------------- least-squares loss
@pytest.mark.parametrize("nvox", [1, 5488, 300001])  # one voxel; the planner's logits (2 x 14^3); beyond 1024 blocks x 256 (grid-stride loop)
@pytest.mark.parametrize("target", [0.0, 1.0])
@pytest.mark.parametrize("slope", [0.05, 1.0])  # upstream's LeakyReLU(0.05) in front of the MSE; 1 = no_activation_leastsq
def test_ls_gan_loss(lib, nvox, target, slope):
    """loss += weight * mse(leaky_relu(l, slope), target) and its gradient on channel 0 of a [nvox, 8] logits tensor.  Loss: 1e-5
    relative (fp32 per-thread sums, one atomic per block, 300 k terms at most).  Gradient: one bf16 rounding of each element (2^-8 of
    it).  The padding channels of dlogits are written with exact zeros (pre-filled with NaN); dlogits = None gives the same loss."""
    cs, weight, pre = 8, 0.5, 0.75
    lg = rnd(nvox, cs, seed=4, scale=1.5)
    lgd = lg.to(dev, BF16)
    dl = nan_bf16(nvox, cs)
    loss = torch.full((1,), pre, device=dev)
    lib.call("mi_ls_gan_loss", lib.ptr(lgd), cs, nvox, float(target), float(slope), lib.ptr(dl), lib.ptr(loss), weight)
    loss2 = torch.full((1,), pre, device=dev)
    lib.call("mi_ls_gan_loss", lib.ptr(lgd), cs, nvox, float(target), float(slope), None, lib.ptr(loss2), weight)
    l0 = lg[:, 0].double().requires_grad_(True)
    ref = weight * F.mse_loss(F.leaky_relu(l0, slope), torch.full_like(l0, target))
    ref.backward()
    got = float(loss) - pre
    assert abs(got - float(ref)) <= 1e-5 * abs(float(ref)) + 1e-7, f"loss {got:.8g} vs {float(ref):.8g}"
    assert abs(float(loss2) - float(loss)) <= 1e-5 * abs(float(ref)) + 1e-7, "dlogits = None changes the loss"
    dl = dl.cpu()
    assert bool((dl[:, 1:] == 0).all()), "padding channels of dlogits not zeroed"
    g = dl[:, 0].double()
    assert bool(((g - l0.grad).abs() <= U * l0.grad.abs()).all()), f"gradient: max err {float((g - l0.grad).abs().max()):.4g}"


# ----------------------------------------------------------------------------------------------------------- BatchNorm running buffers
def _ctx(net, grad):
    from medical_image_generation_amd import engine as E
    return E.Ctx(net.arena(dev), {}, grad_enabled=grad)


@pytest.fixture(scope="module")
def planner_net():
    from medical_image_generation_amd.discriminator import PatchDiscriminator
    torch.manual_seed(0)
    return PatchDiscriminator(spatial_dims=3, num_channels=64, in_channels=1, out_channels=1, num_layers_d=3).to(dev)


def test_arena_is_one_for_both_spellings_of_the_device(planner_net):
    """HipModule.arena("cuda") and arena("cuda:<current>") are the same buffer: rebinding the parameters to a fresh copy would leave
    gradients written through the one arena invisible through the other."""
    a = planner_net.arena(torch.device("cuda"))
    assert planner_net.arena(torch.device("cuda", torch.cuda.current_device())) is a and planner_net.arena(torch.device("cuda")) is a


def _set_bn(net, name, c, seed):
    gamma, beta = 1 + 0.2 * rnd(c, seed=seed), 0.1 * rnd(c, seed=seed + 1)
    net.arena(dev).view(name + ".weight").copy_(gamma)
    net.arena(dev).view(name + ".bias").copy_(beta)
    return gamma, beta


BN_BUF_CASES = [
    # (N, D, H, W, C): N*V = 8 and 27 (Bessel's factor 8/7 and 27/26), a mid count, the planner's last BatchNorm layer (2 x 15^3 x 512)
    (2, 1, 2, 2, 128), (1, 3, 3, 3, 256), (2, 5, 6, 7, 128), (2, 15, 15, 15, 512)]


@pytest.mark.parametrize("case", BN_BUF_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bn_running_update_matches_batchnorm3d(lib, planner_net, case):
    """mi_bn_running_update through discriminator.batchnorm_leaky, two training-mode forwards in sequence from random buffers, against
    nn.BatchNorm3d (fp64, momentum 0.1).  The batch statistics recovered from the buffers, (new - (1 - m) old) / m, must equal torch's
    batch mean and UNBIASED variance to 1e-4 relative (fp32 buffers: the recovery costs ~1e-6; the statistics come from fp32 partial
    sums); comparing the buffers alone would hide them behind the momentum.  num_batches_tracked is exact."""
    from medical_image_generation_amd import discriminator as D
    n, d, h, w, c = case
    name = {128: "0.adn.N", 256: "1.adn.N", 512: "2.adn.N"}[c]
    _set_bn(planner_net, name, c, 11)
    g = torch.Generator().manual_seed(c + n * d)
    rm0, rv0 = torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
    bufs = (rm0.to(dev), rv0.to(dev), torch.tensor(5, dtype=torch.long, device=dev))
    bn = torch.nn.BatchNorm3d(c, momentum=0.1).double().train()
    bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0), bn.num_batches_tracked.fill_(5)
    old_m, old_v = rm0.double(), rv0.double()
    for it in range(2):
        x = (rnd(n, d, h, w, c, seed=20 + it) * (0.5 + torch.rand(c, generator=g)) + 2 * torch.rand(c, generator=g) - 1).bfloat16().float()
        D.batchnorm_leaky(_ctx(planner_net, False), x.to(dev, BF16), name, bufs)
        bn(x.permute(0, 4, 1, 2, 3).double())
        xs = x.double().reshape(-1, c)
        mean, var = xs.mean(0), xs.var(0, unbiased=True)
        new_m, new_v = bufs[0].cpu().double(), bufs[1].cpu().double()
        check((new_m - 0.9 * old_m) / 0.1, mean, 1e-4, f"batch mean recovered from running_mean (update {it + 1})")
        check((new_v - 0.9 * old_v) / 0.1, var, 1e-4, f"unbiased batch variance recovered from running_var (update {it + 1})")
        check(new_m, bn.running_mean, 1e-5, "running_mean")
        check(new_v, bn.running_var, 1e-5, "running_var")
        old_m, old_v = new_m, new_v
    assert int(bufs[2]) == int(bn.num_batches_tracked) == 7


# ----------------------------------------------------------------------------------------------------------- the ops, layer by layer
N_PLANNER = 2
PLANNER_LAYERS = [  # (name, N, Cin, Cout, (D, H, W) of the input, stride, bias): PatchDiscriminator(64, num_layers_d=3) on 2 x 1 x 128^3
    ("initial_conv.conv", N_PLANNER, 1, 64, (128, 128, 128), 2, True),
    ("0.conv", N_PLANNER, 64, 128, (64, 64, 64), 2, False),
    ("1.conv", N_PLANNER, 128, 256, (32, 32, 32), 2, False),
    ("2.conv", N_PLANNER, 256, 512, (16, 16, 16), 1, False),   # m = 2 x 15^3 = 6750, not a multiple of 8
    ("final_conv.conv", N_PLANNER, 512, 1, (15, 15, 15), 1, True),  # Cout 1, padded to 8
]
ODD_LAYERS = [  # the same network with in_channels=2 on 1 x 2 x 40 x 56 x 44
    ("initial_conv.conv", 1, 2, 64, (40, 56, 44), 2, True),
    ("0.conv", 1, 64, 128, (20, 28, 22), 2, False),
    ("1.conv", 1, 128, 256, (10, 14, 11), 2, False),
    ("2.conv", 1, 256, 512, (5, 7, 5), 1, False),
    ("final_conv.conv", 1, 512, 1, (4, 6, 4), 1, True),
]


@pytest.fixture(scope="module")
def odd_net():
    from medical_image_generation_amd.discriminator import PatchDiscriminator
    torch.manual_seed(1)
    return PatchDiscriminator(spatial_dims=3, num_channels=64, in_channels=2, out_channels=1, num_layers_d=3).to(dev)


@pytest.mark.parametrize("case", [("planner",) + c for c in PLANNER_LAYERS] + [("odd",) + c for c in ODD_LAYERS],
                         ids=lambda c: f"{c[0]}-{c[1]}-n{c[2]}_{c[3]}to{c[4]}_{'x'.join(map(str, c[5]))}_s{c[6]}")
def test_conv_gemm_layer(request, case):
    """discriminator.conv_gemm (pack + im2col + NT GEMM, and its tape backward: transposes + GEMM + unpack for dW, column sums for the
    bias, GEMM + col2im for dx) against F.conv3d autograd in fp32 on the bf16-rounded input / weight / output gradient.  Budget: the
    library's |err| <= 1e-2 * max|ref| for y, dx, dW and the bias gradient; the forward is bf16 products summed in fp32 and rounded
    once, so every element of y must also be within 2^-7 * max|y|."""
    from medical_image_generation_amd import discriminator as D
    which, name, n, cin, cout, dims, s, bias = case
    net = request.getfixturevalue("planner_net" if which == "planner" else "odd_net")
    torch.set_num_threads(16)
    k, p = 4, 1
    arena = net.arena(dev)
    g = torch.Generator().manual_seed(sum(map(ord, name)) + cin)
    w = (torch.randn(cout, cin, k, k, k, generator=g) / math.sqrt(cin * k ** 3)).bfloat16().float()
    b = torch.randn(cout, generator=g) if bias else None
    arena.view(name + ".weight").copy_(w)
    if bias:
        arena.view(name + ".bias").copy_(b)
    arena.grad.zero_()
    x = torch.randn(n, cin, *dims, generator=g).bfloat16().float()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    yr = F.conv3d(xr, wr, br, stride=s, padding=p)
    gy = torch.randn(yr.shape, generator=g).bfloat16().float()
    yr.backward(gy)
    ctx = _ctx(net, True)
    x_cl = x.permute(0, 2, 3, 4, 1).contiguous().to(dev, BF16)
    y = D.conv_gemm(ctx, x_cl, name, k, s, p, bias)
    cop = y.shape[-1]
    assert cop == (cout + 7) // 8 * 8 and tuple(y.shape[1:4]) == tuple(yr.shape[2:])
    yc = y.cpu()
    assert bool((yc[..., cout:] == 0).all()), "padding channels of y not zero"
    yg = yc[..., :cout].float().permute(0, 4, 1, 2, 3)
    check(yg, yr.detach(), 1e-2, f"{name} forward")
    assert float((yg - yr.detach()).abs().max()) <= 2.0 ** -7 * float(yr.detach().abs().max()), f"{name} forward: beyond bf16 rounding"
    dy = torch.zeros(y.shape, dtype=BF16)
    dy[..., :cout] = gy.permute(0, 2, 3, 4, 1).bfloat16()
    ctx.tape.backward(y, dy.to(dev))
    dx = ctx.tape.take(x_cl)
    check(dx.float().cpu().permute(0, 4, 1, 2, 3), xr.grad, 1e-2, f"{name} dx")
    check(arena.gview(name + ".weight").cpu(), wr.grad, 1e-2, f"{name} dW")
    if bias:
        check(arena.gview(name + ".bias").cpu(), br.grad, 1e-2, f"{name} bias gradient")


BN_CASES = [
    # (N, D, H, W, C, mean offset): the three BatchNorm layers at the planner's shapes, a small count, a mean 30x the standard deviation
    (2, 32, 32, 32, 128, 0.0), (2, 16, 16, 16, 256, 0.0), (2, 15, 15, 15, 512, 0.0),
    (1, 2, 2, 3, 128, 0.0),
    (2, 8, 9, 7, 256, 30.0),
]


@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "x".join(map(str, c[:5])) + (f"_mean{int(c[5])}" if c[5] else ""))
def test_batchnorm_leaky_layer(planner_net, case):
    """discriminator.batchnorm_leaky (GroupNorm kernels, one channel per group, activation code 2) forward / backward against
    F.batch_norm(training=True) + F.leaky_relu(0.2) autograd in fp32.  Budgets of test_groupnorm_fwd_bwd: y 1e-2, dx 1.5e-2 (the
    backward's mean terms cancel), dgamma / dbeta 1e-2, all relative to max|ref|."""
    from medical_image_generation_amd import discriminator as D
    n, d, h, w, c, off = case
    name = {128: "0.adn.N", 256: "1.adn.N", 512: "2.adn.N"}[c]
    torch.set_num_threads(16)
    gamma, beta = _set_bn(planner_net, name, c, 30)
    arena = planner_net.arena(dev)
    arena.grad.zero_()
    x = (rnd(n, d, h, w, c, seed=31) + off).bfloat16().float()
    gy = rnd(n, d, h, w, c, seed=32)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yr = F.leaky_relu(F.batch_norm(xr.permute(0, 4, 1, 2, 3), None, None, gr, br, training=True, eps=1e-5), 0.2)
    yr.backward(gy.permute(0, 4, 1, 2, 3))
    bufs = (torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros((), dtype=torch.long, device=dev))
    ctx = _ctx(planner_net, True)
    x_cl = x.to(dev, BF16)
    y = D.batchnorm_leaky(ctx, x_cl, name, bufs)
    check(y.float().cpu().permute(0, 4, 1, 2, 3), yr.detach(), 1e-2, "batchnorm+leaky forward")
    ctx.tape.backward(y, gy.to(dev, BF16))
    dx = ctx.tape.take(x_cl)
    check(dx.float().cpu(), xr.grad, 1.5e-2, "batchnorm+leaky dx")
    check(arena.gview(name + ".weight").cpu(), gr.grad, 1e-2, "dgamma")
    check(arena.gview(name + ".bias").cpu(), br.grad, 1e-2, "dbeta")
