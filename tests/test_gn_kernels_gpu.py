"""Per-op parity of the GroupNorm kernels (csrc/groupnorm.hip) against fp64 torch references, at the shapes the networks run.

test_kernels_gpu.py checks GroupNorm up to 16^3 voxels against the tensor's max.  At those sizes the streaming apply kernels run one
trip of their grid-stride loop (slot 0 only), and a statistics lane sums one or two voxels.  Here each kernel runs at the network's
sizes, where the apply loops make several trips with a ragged last one and a lane sums 64 to 195 voxels in fp32.  Each output is
compared, element by element or per (image, group) / per channel, with an fp64 restatement of the same operation on the same bf16
inputs.  Inputs have a different mean and spread per (image, channel), so a wrong group, channel or image index changes the
answer.  One case puts every group's mean at 8 times its standard deviation: the cancellation case of E[x^2] - mean^2.

The fp64 references run as torch ops on the GPU (aten, not ours), in voxel slabs, so a 128^3 tensor never has an fp64 copy."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

dev = torch.device("cuda")
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-6  # the networks' GroupNorm eps
SLAB = 1 << 23  # elements per fp64 slab of a reference pass
FUSED_REPLICAS = 16  # MI_GN_FUSED_REPLICAS of include/medimgen_hip.h


@pytest.fixture(scope="module")
def lib():
    from medical_image_generation_amd import _lib
    _lib.load()
    return _lib


# ----------------------------------------------------------------------------------------------------------- launch geometry
def apply_trips(n, c, v, slots):
    """The grid-stride loop of k_gn_apply (slots = 4) and k_gn_bwd_apply (slots = 2, its pieces in flight per stream), restated from
    apply_grid() in csrc/groupnorm.hip: ~16 blocks per CU over the batch (at least 64), ceil(V * C8 / 256) below that, then
    trimmed so that grid * 256 is a multiple of C8.  A trip covers slots * R voxels, R = grid * 256 / C8.
    Returns (R, full trips, voxels in the ragged last trip)."""
    c8 = c // 8
    grid = min(-(-v * c8 // 256), max(256 * 16 // n, 64))
    m = c8 // math.gcd(c8, 256)
    grid = grid - grid % m if grid >= m else m
    r = grid * 256 // c8
    full, rest = divmod(v, slots * r)
    return r, full, rest


def stats_chunk(v):
    """Voxels per chunk of k_gn_partial / k_gn_bwd_partial: pick_vchunk() in csrc/groupnorm.hip."""
    return max(-(-v // 512), 16)


# ----------------------------------------------------------------------------------------------------------- shapes
# (name, N, C, (D, H, W), G, offset): the GroupNorm inputs the configs of oracle/cases.py run at full size.  offset: every group's
# mean is 8x its standard deviation.  Small shapes last: the module-scoped case of the last shape stays alive until the end.
SHAPES = [
    ("c4_128_c32", 1, 32, (128, 128, 128), 32, False),   # C4, level 0 (128^3): the down path
    ("c4_128_c64", 1, 64, (128, 128, 128), 32, False),   # C4, level 0: up-path concatenation 32 + 32
    ("c4_128_c96", 1, 96, (128, 128, 128), 32, True),    # C4, level 0: up-path concatenation 64 + 32; mean = 8 std
    ("c3a_128_c32", 2, 32, (128, 128, 128), 16, False),  # C3a autoencoder, level 0
    ("odd_c32", 1, 32, (100, 101, 103), 32, False),      # odd extents: ragged trips and chunks
    ("c4_64_c64", 1, 64, (64, 64, 64), 32, False),       # C4, level 1
    ("c4_64_c128", 1, 128, (64, 64, 64), 32, False),     # C4, level 1: up-path concatenation 64 + 64
    ("c3a_32_c128", 2, 128, (32, 32, 32), 16, False),    # C3a, level 2
    ("c3b_32_c256", 4, 256, (32, 32, 32), 32, False),    # C3b latent UNet, level 0
    ("c4_16_c256", 1, 256, (16, 16, 16), 32, False),     # C4, level 3
    ("c4_16_c512", 1, 512, (16, 16, 16), 32, False),     # C4, level 3: up-path concatenation 256 + 256
    ("c3b_16_c512", 4, 512, (16, 16, 16), 32, False),    # C3b, level 1
    ("c3b_8_c768", 4, 768, (8, 8, 8), 32, False),        # C3b, level 2: C8 = 96, two voxel rows per block in the fold
]


def test_shapes_cover_every_trip_form():
    """The apply kernels' loop bodies beyond slot 0 and their masked tail run only at the sizes above.  If the grid rules change, this
    fails instead of the coverage vanishing silently."""
    for slots in (4, 2):  # k_gn_apply, k_gn_bwd_apply
        trips = [apply_trips(n, c, d * h * w, slots) + (d * h * w,) for _, n, c, (d, h, w), _, _ in SHAPES]
        assert any(full >= 2 for _, full, _, _ in trips), f"no shape runs >= 2 full trips of the {slots}-slot loop"
        assert any(full >= 1 and rest % r for r, full, rest, _ in trips), \
            f"no shape ends the {slots}-slot loop in a partial trip after full ones"
        assert any(rest > r and rest % r for r, full, rest, _ in trips), \
            f"no shape runs a partial trip with slots beyond slot 0 and some slots masked ({slots}-slot loop)"
    assert apply_trips(1, 96, 128 ** 3, 4) == (87360, 6, 512)  # the worked example: grid 4095
    assert max(stats_chunk(d * h * w) * (c // 8) / 256 for _, _, c, (d, h, w), _, _ in SHAPES) >= 64  # voxels per fp32 lane sum


# ----------------------------------------------------------------------------------------------------------- fp64 references
def slabs(v, c):
    s = max(1, SLAB // c)
    return [(v0, min(v, v0 + s)) for v0 in range(0, v, s)]


def per_channel(t, cpg):  # [N, G] -> [N, C]
    return t.repeat_interleave(cpg, dim=1)


def ref_stats(x3, groups):
    """Two-pass fp64 mean and (biased) variance per (image, group) of x3 [N, V, C]."""
    n, v, c = x3.shape
    cpg = c // groups
    s = torch.zeros(n, c, dtype=F64, device=x3.device)
    for i in range(n):
        for v0, v1 in slabs(v, c):
            s[i] += x3[i, v0:v1].double().sum(0)
    mean = s.view(n, groups, cpg).sum(-1) / (v * cpg)
    mc = per_channel(mean, cpg)
    q = torch.zeros_like(s)
    for i in range(n):
        for v0, v1 in slabs(v, c):
            q[i] += (x3[i, v0:v1].double() - mc[i]).square().sum(0)
    return mean, q.view(n, groups, cpg).sum(-1) / (v * cpg)


def act64(u, act):
    if act == 1:
        return u * torch.sigmoid(u)
    if act == 2:
        return torch.where(u > 0, u, 0.2 * u)
    return u


def dact64(u, act):
    if act == 1:
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    if act == 2:
        return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, 0.2))
    return torch.ones_like(u)


def ulp_bf16(r):
    """One bf16 ulp (8 significant bits) of |r|, at least that of the smallest normal."""
    _, e = torch.frexp(r.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(r), e - 8)


def ref_bwd_coef(x3, g3, sc, sh, mean, rstd, gamma, groups, act):
    """The closed-form backward of y = act(x * sc + sh), xhat = (x - mean) * rstd, in fp64:  dx = a * du + b * x + c  with
    du = g * act'(x * sc + sh), a = rstd * gamma, b = -rstd^2 m2, c = rstd^2 m2 mean - rstd m1, m1 / m2 the group means of
    gamma * du / gamma * du * xhat;  dbeta = sum du, dgamma = sum du * xhat.  sc, sh: [N, C];  mean, rstd: [N, G];  gamma: [C].
    Also the per-channel sums of |du| and |du * xhat| (the scale of the fp32 accumulation error of the parameter gradients)."""
    n, v, c = x3.shape
    cpg = c // groups
    mc, rc = per_channel(mean, cpg), per_channel(rstd, cpg)
    s1, s2, l1, l2 = (torch.zeros(n, c, dtype=F64, device=x3.device) for _ in range(4))
    for i in range(n):
        for v0, v1 in slabs(v, c):
            xs = x3[i, v0:v1].double()
            du = g3[i, v0:v1].double() * dact64(xs * sc[i] + sh[i], act)
            dxh = du * (xs - mc[i]) * rc[i]
            s1[i] += du.sum(0)
            s2[i] += dxh.sum(0)
            l1[i] += du.abs().sum(0)
            l2[i] += dxh.abs().sum(0)
    m = v * cpg
    m1 = (gamma * s1).view(n, groups, cpg).sum(-1) / m
    m2 = (gamma * s2).view(n, groups, cpg).sum(-1) / m
    return dict(a=rc * gamma, b=per_channel(-rstd * rstd * m2, cpg), c=per_channel(rstd * rstd * m2 * mean - rstd * m1, cpg),
                dbeta=s1.sum(0), dgamma=s2.sum(0), l1=l1.sum(0), l2=l2.sum(0))


def ref_dx(x3, g3, sc, sh, coef, act, i, v0, v1, adds=()):
    xs = x3[i, v0:v1].double()
    gs = g3[i, v0:v1].double()
    du = gs * dact64(xs * sc[i] + sh[i], act)
    ref = coef["a"][i] * du + coef["b"][i] * xs + coef["c"][i]
    # fp32 error of the kernel's arithmetic: its coefficients (fp64 finish of fp32 partial sums), du (a SiLU derivative near its
    # zero at u = -1.28 is a difference of O(1) terms, so its error scales with |g|, not |du|) and the sum with the pending branches
    scale = (coef["a"][i] * gs).abs() + (coef["b"][i] * xs).abs() + coef["c"][i].abs()
    for t in adds:
        a = t[i, v0:v1].double()
        ref, scale = ref + a, scale + a.abs()
    return ref, scale


def assert_within(err, bound, what):
    bad = ~(err <= bound)  # NaN (an unwritten output) counts as a violation
    nbad = int(bad.sum())
    if nbad:
        ratio = float(torch.nan_to_num(err / bound, nan=float("inf")).max())
        raise AssertionError(f"{what}: {nbad} of {err.numel()} elements outside the bound (worst err/bound {ratio:.3g})")


# ----------------------------------------------------------------------------------------------------------- inputs
def gen_cl(n, v, c, mu, sd, seed):
    """bf16 [N, V, C]: mu[n, c] + sd[n, c] * N(0, 1), drawn on the GPU slab by slab."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(n, v, c, dtype=BF16, device=dev)
    for i in range(n):
        for v0, v1 in slabs(v, c):
            out[i, v0:v1] = (mu[i] + sd[i] * torch.randn(v1 - v0, c, generator=gen, device=dev)).to(BF16)
    return out


def channel_moments(n, c, groups, seed, offset):
    """A mean and spread per (image, channel).  offset: the channels of a group share one mean, 8x the group's standard deviation
    (sqrt of the mean channel variance), with a random sign per (image, group)."""
    gen = torch.Generator().manual_seed(seed)
    sd = torch.exp(0.5 * torch.randn(n, c, generator=gen))
    if offset:
        cpg = c // groups
        gsd = sd.square().view(n, groups, cpg).mean(-1).sqrt()
        sign = torch.where(torch.rand(n, groups, generator=gen) < 0.5, -1.0, 1.0)
        mu = per_channel(8 * sign * gsd, cpg)
    else:
        mu = 1.5 * torch.randn(n, c, generator=gen)
    return mu.to(dev), sd.to(dev)


def wide(t, c0, extra, fill=0.0):
    """t [N, D, H, W, C] copied into channels [c0, c0 + C) of a buffer with `extra` more channels; returns (buffer, view)."""
    c = t.shape[-1]
    buf = torch.full(t.shape[:-1] + (c + extra,), fill, dtype=t.dtype, device=t.device)
    view = buf[..., c0:c0 + c]
    view.copy_(t)
    return buf, view


class Case:
    pass


@pytest.fixture(scope="module", params=SHAPES, ids=[s[0] for s in SHAPES])
def case(request, lib):
    name, n, c, dims, groups, offset = request.param
    v = dims[0] * dims[1] * dims[2]
    k = Case()
    k.name, k.n, k.c, k.dims, k.v, k.groups, k.offset = name, n, c, dims, v, groups, offset
    seed = sum(map(ord, name))
    mu, sd = channel_moments(n, c, groups, seed, offset)
    k.x3 = gen_cl(n, v, c, mu, sd, seed + 1)
    k.x = k.x3.view(n, *dims, c)
    gen = torch.Generator().manual_seed(seed + 2)
    k.gamma = (1 + 0.3 * torch.randn(c, generator=gen)).to(dev)
    k.beta = (0.5 * torch.randn(c, generator=gen)).to(dev)
    # the incoming gradient: its own mean and spread per (image, channel)
    k.g3 = gen_cl(n, v, c, 0.3 * torch.randn(n, c, generator=gen).to(dev), torch.exp(0.5 * torch.randn(n, c, generator=gen)).to(dev), seed + 3)
    k.mean_ref, k.var_ref = ref_stats(k.x3, groups)
    # the statistics pass under test; its records feed the apply / backward tests (each compared with fp64 of its own inputs)
    k.ss = torch.full((n, c, 2), float("nan"), dtype=F32, device=dev)
    k.mr = torch.full((n, groups, 2), float("nan"), dtype=F32, device=dev)
    nb = lib.call_raw("mi_gn_workspace_bytes", n, v, c)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    lib.call("mi_gn_stats", k.x.data_ptr(), c, n, v, c, groups, EPS, k.gamma.data_ptr(), k.beta.data_ptr(), k.ss.data_ptr(),
             k.mr.data_ptr(), ws.data_ptr(), nb)
    k.sc, k.sh = k.ss[..., 0].double(), k.ss[..., 1].double()
    k.mean_k, k.rstd_k = k.mr[..., 0].double(), k.mr[..., 1].double()
    k.bwd = {}
    yield k
    del k.x, k.x3, k.g3
    torch.cuda.empty_cache()


def check_stats(mean, rstd, sc, sh, mean_ref, var_ref, gamma, beta, what):
    """Bounds on statistics records against fp64 two-pass values: |mean - ref| <= 1e-5 sqrt(E[x^2]), |rstd / ref - 1| <= 1e-4, and
    scale = gamma * rstd, shift = beta - mean * scale to the error those bounds propagate (plus fp32 rounding)."""
    rms = (var_ref + mean_ref.square()).sqrt()
    rstd_ref = 1.0 / (var_ref + EPS).sqrt()
    assert_within((mean - mean_ref).abs(), 1e-5 * rms, f"{what}: mean")
    assert_within((rstd / rstd_ref - 1).abs(), torch.full_like(rstd, 1e-4), f"{what}: rstd")
    cpg = sc.shape[1] // mean.shape[1]
    g64, b64 = gamma.double(), beta.double()
    sc_ref = g64 * per_channel(rstd_ref, cpg)
    sh_ref = b64 - per_channel(mean_ref, cpg) * sc_ref
    assert_within((sc - sc_ref).abs(), 1e-4 * sc_ref.abs() + 1e-30, f"{what}: scale")
    sh_tol = 1e-4 * (per_channel(mean_ref, cpg) * sc_ref).abs() + 1e-5 * per_channel(rms, cpg) * sc_ref.abs() + 1e-6 * b64.abs()
    assert_within((sh - sh_ref).abs(), sh_tol, f"{what}: shift")


def test_stats(case):
    """mi_gn_stats (k_gn_partial + k_gn_finalize) against two-pass fp64 statistics per (image, group)."""
    k = case
    check_stats(k.mean_k, k.rstd_k, k.sc, k.sh, k.mean_ref, k.var_ref, k.gamma, k.beta, k.name)
    if k.offset:  # the inputs are what the case says they are
        ratio = (k.mean_ref.abs() / k.var_ref.sqrt())
        assert float(ratio.min()) > 7.5 and float(ratio.max()) < 8.5


def check_apply(x3, y3, sc, sh, act, what):
    """Every element within one bf16 ulp of the fp64 act(x * sc + sh) (plus the fp32 rounding of x * sc + sh, which only matters
    where it cancels to near zero)."""
    n, v, c = x3.shape
    for i in range(n):
        for v0, v1 in slabs(v, c):
            xs = x3[i, v0:v1].double()
            u = xs * sc[i] + sh[i]
            ref = act64(u, act)
            bound = ulp_bf16(ref) + 2.0 ** -22 * ((xs * sc[i]).abs() + sh[i].abs())
            assert_within((y3[i, v0:v1].double() - ref).abs(), bound, f"{what} (image {i}, voxels {v0}..{v1})")


@pytest.mark.parametrize("act", [0, 1])
def test_apply(case, lib, act):
    """mi_gn_apply against fp64 act(x * sc + sh) with the kernel's own scale / shift; then the same launch on a channel slice of a wider
    x into a channel slice of a wider y: the same bits, and the channels outside the slice untouched.  LeakyReLU (act 2, the
    discriminator's BatchNorm role) runs at one shape."""
    k = case
    n, v, c = k.n, k.v, k.c
    for a in (act, 2) if act == 0 and k.name == "c4_64_c64" else (act,):
        y = torch.full_like(k.x, float("nan"))
        lib.call("mi_gn_apply", k.x.data_ptr(), c, k.ss.data_ptr(), y.data_ptr(), c, n, v, c, a)
        check_apply(k.x3, y.view(n, v, c), k.sc, k.sh, a, f"{k.name} act {a}")
        # pitches: x in channels [8, 8 + C) of a C + 16 buffer, y into channels [16, 16 + C) of a C + 24 buffer
        _, xv = wide(k.x, 8, 16)
        ybuf = torch.full(k.x.shape[:-1] + (c + 24,), -3.0, dtype=BF16, device=dev)
        lib.call("mi_gn_apply", xv.data_ptr(), c + 16, k.ss.data_ptr(), ybuf[..., 16:].data_ptr(), c + 24, n, v, c, a)
        assert torch.equal(ybuf[..., 16:16 + c].view(torch.int16), y.view(torch.int16)), f"act {a}: strided apply differs from the dense one"
        assert bool((ybuf[..., :16] == -3.0).all()) and bool((ybuf[..., 16 + c:] == -3.0).all()), f"act {a}: apply wrote outside its slice"


def bwd_ref(k, act):
    if act not in k.bwd:
        k.bwd[act] = ref_bwd_coef(k.x3, k.g3, k.sc, k.sh, k.mean_k, k.rstd_k, k.gamma.double(), k.groups, act)
    return k.bwd[act]


@pytest.mark.parametrize("fused", [False, True], ids=["mi_gn_bwd", "mi_gn_bwd_fused"])
@pytest.mark.parametrize("act", [0, 1])
def test_bwd(case, lib, act, fused):
    """mi_gn_bwd (the engine's default: partial, finalize, apply) and mi_gn_bwd_fused (fp64 atomic sums in replicas, coefficients
    derived inside the apply pass) against the closed-form fp64 backward, from the forward's records.
    act 0: g is a channel slice of a wider buffer, no pending branches.  act 1 (SiLU): dense g, pending branches add and add2 (add2 a
    channel slice).  dx: one bf16 ulp of the reference plus 1e-5 of the fp32 terms; dgamma / dbeta accumulate onto non-zero values
    and must be within 1e-4 relative per channel, over a floor of 1e-6 of the summed magnitudes."""
    k = case
    n, v, c, groups = k.n, k.v, k.c, k.groups
    coef = bwd_ref(k, act)
    shape = k.x.shape
    adds = ()
    g_cs = c
    if act == 0:
        _, g = wide(k.g3.view(shape), 8, 16)
        g_cs = c + 16
        add_p = add2_p = None
        add_cs = add2_cs = 0
    else:
        g = k.g3.view(shape)
        gen = torch.Generator(device=dev).manual_seed(c + v)
        add = torch.randn(shape, generator=gen, device=dev).to(BF16)
        _, add2 = wide(torch.randn(shape, generator=gen, device=dev).to(BF16), 8, 8)
        add_p, add_cs, add2_p, add2_cs = add.data_ptr(), c, add2.data_ptr(), c + 8
        adds = (add.view(n, v, c), add2.reshape(n, v, c))
    gen = torch.Generator().manual_seed(7 * c + act)
    dg0 = coef["dgamma"].abs().mean() * torch.randn(c, generator=gen, dtype=F64).to(dev)
    db0 = coef["dbeta"].abs().mean() * torch.randn(c, generator=gen, dtype=F64).to(dev)
    dgamma, dbeta = dg0.float(), db0.float()
    dg_before, db_before = dgamma.double(), dbeta.double()
    dx = torch.full(shape, float("nan"), dtype=BF16, device=dev)
    args = (g.data_ptr(), g_cs, k.x.data_ptr(), c, n, v, c, groups, k.gamma.data_ptr(), k.ss.data_ptr(), k.mr.data_ptr(), act,
            add_p, add_cs, add2_p, add2_cs, dx.data_ptr(), c, dgamma.data_ptr(), dbeta.data_ptr())
    if fused:
        sums = torch.zeros(FUSED_REPLICAS * n * c * 2, dtype=F64, device=dev)
        lib.call("mi_gn_bwd_fused", *args, sums.data_ptr())
    else:
        cf = torch.full((n, c, 3), float("nan"), dtype=F32, device=dev)
        nb = lib.call_raw("mi_gn_workspace_bytes", n, v, c)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        lib.call("mi_gn_bwd", *args, cf.data_ptr(), ws.data_ptr(), nb)
    what = f"{k.name} act {act} {'fused' if fused else 'default'}"
    dx3 = dx.view(n, v, c)
    g3 = g.reshape(n, v, c)
    for i in range(n):
        for v0, v1 in slabs(v, c):
            ref, scale = ref_dx(k.x3, g3, k.sc, k.sh, coef, act, i, v0, v1, adds)
            assert_within((dx3[i, v0:v1].double() - ref).abs(), ulp_bf16(ref) + 1e-5 * scale, f"{what}: dx (image {i}, voxels {v0}..{v1})")
    for got, before, ref, l1, nm in ((dgamma, dg_before, coef["dgamma"], coef["l2"], "dgamma"), (dbeta, db_before, coef["dbeta"], coef["l1"], "dbeta")):
        tol = 1e-4 * ref.abs() + 1e-6 * l1 + 2.0 ** -23 * (before + ref).abs()
        assert_within((got.double() - (before + ref)).abs(), tol, f"{what}: {nm}")


def test_reference_matches_autograd():
    """The closed-form references above equal F.group_norm (+ SiLU / LeakyReLU) and autograd in fp64, on the CPU."""
    n, c, dims, groups = 2, 48, (5, 6, 7), 8
    v = dims[0] * dims[1] * dims[2]
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(n, c, *dims, generator=gen, dtype=F64) * torch.exp(0.5 * torch.randn(n, c, 1, 1, 1, generator=gen, dtype=F64))
         + 2 * torch.randn(n, c, 1, 1, 1, generator=gen, dtype=F64))
    g = torch.randn(n, c, *dims, generator=gen, dtype=F64)
    gamma, beta = 1 + 0.3 * torch.randn(c, generator=gen, dtype=F64), 0.5 * torch.randn(c, generator=gen, dtype=F64)
    x3, g3 = x.permute(0, 2, 3, 4, 1).reshape(n, v, c), g.permute(0, 2, 3, 4, 1).reshape(n, v, c)
    mean, var = ref_stats(x3, groups)
    rstd = 1 / (var + EPS).sqrt()
    sc = gamma * per_channel(rstd, c // groups)
    sh = beta - per_channel(mean, c // groups) * sc
    for act in (0, 1, 2):
        xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = F.group_norm(xr, groups, gr, br, EPS)
        y = F.silu(y) if act == 1 else (F.leaky_relu(y, 0.2) if act == 2 else y)
        y.backward(g)
        y3 = y.detach().permute(0, 2, 3, 4, 1).reshape(n, v, c)
        ref_y = torch.stack([act64(x3[i] * sc[i] + sh[i], act) for i in range(n)])
        assert torch.allclose(ref_y, y3, rtol=1e-12, atol=1e-12)
        coef = ref_bwd_coef(x3, g3, sc, sh, mean, rstd, gamma, groups, act)
        dx = torch.stack([ref_dx(x3, g3, sc, sh, coef, act, i, 0, v)[0] for i in range(n)])
        assert torch.allclose(dx, xr.grad.permute(0, 2, 3, 4, 1).reshape(n, v, c), rtol=1e-10, atol=1e-12)
        assert torch.allclose(coef["dgamma"], gr.grad, rtol=1e-10, atol=1e-12)
        assert torch.allclose(coef["dbeta"], br.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(ulp_bf16(torch.tensor([1.0, 1.5, -3.0, 0.75], dtype=F64)), torch.tensor([2 ** -7, 2 ** -7, 2 ** -6, 2 ** -8], dtype=F64))


# ----------------------------------------------------------------------------------------------------------- single-launch form
@pytest.mark.parametrize("name,n,c,groups", [("c4_16_c512", 1, 512, 32), ("c4_16_c256", 1, 256, 32), ("c3b_16_c512", 4, 512, 32)])
@pytest.mark.parametrize("act", [0, 1])
def test_single_launch_at_network_shapes(lib, monkeypatch, name, n, c, groups, act):
    """mi_gn_small_fwd (gn_apply of a pending GNStats, MI_GN_SMALL on) at the 16^3 levels: records and output to the bounds above.
    512 channels at 16^3 (16 per group) is exactly at its support limit V * cpg / 8 = 8192.  act 1 runs the 8x-offset inputs."""
    from medical_image_generation_amd import hipops as ops
    monkeypatch.setattr(ops, "GN_SMALL", True)
    v = 16 ** 3
    vmax = 8192 * 8 // (c // groups)  # the support limit in voxels
    assert lib.call_raw("mi_gn_small_supported", n, v, c, groups) == 1
    assert lib.call_raw("mi_gn_small_supported", n, vmax, c, groups) == 1
    assert lib.call_raw("mi_gn_small_supported", n, vmax + 1, c, groups) == 0
    if c == 512:
        assert vmax == v
    mu, sd = channel_moments(n, c, groups, sum(map(ord, name)) + act, offset=act == 1)
    x3 = gen_cl(n, v, c, mu, sd, 11 + act)
    x = x3.view(n, 16, 16, 16, c)
    gen = torch.Generator().manual_seed(c + act)
    gamma, beta = (1 + 0.3 * torch.randn(c, generator=gen)).to(dev), (0.5 * torch.randn(c, generator=gen)).to(dev)
    st = ops.gn_stats(x, groups, EPS, gamma, beta)
    assert st._pending is not None
    y = ops.gn_apply(x, st, act)
    assert st._pending is None
    mean_ref, var_ref = ref_stats(x3, groups)
    mr, ss = st.mean_rstd, st.scale_shift
    check_stats(mr[..., 0].double(), mr[..., 1].double(), ss[..., 0].double(), ss[..., 1].double(), mean_ref, var_ref, gamma, beta, name)
    check_apply(x3, y.view(n, v, c), ss[..., 0].double(), ss[..., 1].double(), act, f"{name} single launch act {act}")


# ----------------------------------------------------------------------------------------------------------- statistics from conv sums
def fp64_check_from_sums(ops, y, sums, sums_b, groups, what):
    n, d, h, w, c = y.shape
    v = d * h * w
    gen = torch.Generator().manual_seed(c + groups)
    gamma, beta = (1 + 0.3 * torch.randn(c, generator=gen)).to(dev), (0.5 * torch.randn(c, generator=gen)).to(dev)
    st = ops.gn_stats_from_sums(sums, sums_b, n, v, groups, EPS, gamma, beta)
    mean_ref, var_ref = ref_stats(y.view(n, v, c), groups)
    check_stats(st.mean_rstd[..., 0].double(), st.mean_rstd[..., 1].double(), st.scale_shift[..., 0].double(),
                st.scale_shift[..., 1].double(), mean_ref, var_ref, gamma, beta, what)


def test_stats_from_conv_sums_at_size(lib):
    """GroupNorm statistics built by mi_gn_stats_from_partial from the sums the convs emit, at C4's 128^3 level: the rolling-halo k3
    forward (1 x 32 -> 32), the 1 -> 32 input conv (conv_c1.hip), and the 32 + 32 concatenation of the two as on the up path.  Compared
    with fp64 statistics of the stored bf16 outputs, to the bounds of test_stats."""
    from medical_image_generation_amd import hipops as ops
    dims, n, c = (128, 128, 128), 1, 32
    v = dims[0] * dims[1] * dims[2]
    gen = torch.Generator().manual_seed(5)
    # the 1 -> 32 input conv
    plan1 = ops.ConvPlan(n, dims, 1, c, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    assert plan1.stats_chunks > 0
    plan1.pack((torch.randn(c, 1, 3, 3, 3, generator=gen) / math.sqrt(27)).bfloat16().float().to(dev))
    x1 = gen_cl(n, v, 1, torch.full((n, 1), 0.5, device=dev), torch.ones(n, 1, device=dev), 21).view(n, *dims, 1)
    ya, sa = plan1.fwd(x1, addvec=torch.randn(c, generator=gen).to(dev), want_sums=True)
    assert sa is not None
    fp64_check_from_sums(ops, ya, sa, None, 32, "input conv sums")
    # the 32 -> 32 k3 forward on the rolling-halo kernel, input with a mean and spread per channel
    plan = ops.ConvPlan(n, dims, c, c, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    assert plan.stats_chunks > 0
    plan.pack((torch.randn(c, c, 3, 3, 3, generator=gen) / math.sqrt(27 * c)).bfloat16().float().to(dev))
    mu, sd = channel_moments(n, c, 32, 22, False)
    x = gen_cl(n, v, c, mu, sd, 23).view(n, *dims, c)
    yb, sb = plan.fwd(x, addvec=torch.randn(c, generator=gen).to(dev), want_sums=True)
    del x
    assert sb is not None
    fp64_check_from_sums(ops, yb, sb, None, 32, "k3 conv sums")
    # [yb | ya]: two sources with different chunk counts, 32 groups of 2 channels
    cat = ops.concat_channels(yb, ya)
    fp64_check_from_sums(ops, cat, sb, sa, 32, "concatenation of two conv outputs")
