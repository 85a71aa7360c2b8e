"""The instruments of tests/test_perc_kernels_gpu.py (the closed forms in tests/perc_ref.py), checked without a GPU: they agree with
torch's own slicing, pooling and autograd; a model of a correct kernel (fp32 arithmetic in the kernel's order, bf16 outputs) meets every
per-element bound at every shape the GPU tests run; and each planted fault is rejected by the same comparer and bound.

On "inside half of the bound": the outputs of these kernels are bf16, and the first term of each bound, 2^-8 |want|, IS one correct
bf16 rounding (half an ulp is up to 2^-8 of the value at the bottom of a binade), so a correctly rounded output sits at up to 0.996 of
it -- no kernel can stay inside half.  So the model's fp32 value BEFORE the output rounding is held to half of the bound, and, the
sharper statement, to the bound's fp32 term alone (2^-22 ... : three or four fp32 roundings of 2^-24 each reach 0.5 to 0.75 of it);
the rounded output is then held to the whole bound, as the GPU tests hold the kernels."""
import pytest
import torch
import torch.nn.functional as F

from tests import perc_ref as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def _scaling():
    from medical_image_generation_amd.perceptual import _SCALE, _SHIFT
    return torch.tensor(_SHIFT, dtype=F32), torch.tensor(_SCALE, dtype=F32)


GATHER_CASES = [(R.EDGE_VOLUME, c, axis, False) for c in (1, 3) for axis in range(3)] + [(R.LOOP_VOLUME, 1, 0, True)]


def _gather_case(shape, c, axis, loop):
    idx = R.loop_indices() if loop else R.edge_indices(R.extent(shape, axis))
    return R.volume(shape, c, 10 + axis), idx


@pytest.mark.parametrize("shape,c,axis,loop", GATHER_CASES)
def test_gather_closed_form_and_model(shape, c, axis, loop):
    shift, scale = _scaling()
    x, idx = _gather_case(shape, c, axis, loop)
    want, bound = R.gather(x, c, axis, idx, shift, scale)
    assert bool(torch.isfinite(want).all()), "a NaN of the stride's extra channels reached the output"
    # upstream's slicing: permute / index_select of the NCDHW volume, then the scaling layer
    ok = (idx >= 0) & (idx < R.extent(shape, axis))
    ncdhw = x[..., :c].double().permute(0, 4, 1, 2, 3)
    ref = R.slices(ncdhw, axis + 2).index_select(0, idx[ok].long()).expand(-1, 3, -1, -1)
    ref = ((ref - shift.double().view(1, 3, 1, 1)) / scale.double().view(1, 3, 1, 1)).permute(0, 2, 3, 1)
    assert torch.equal(want[ok][..., :3], ref)
    assert not bool(want[~ok].any()) and not bool(want[..., 3:].any())
    # the model: before the rounding inside half of the fp32 term, after it inside the bound
    pre = R.gather_presum(x, c, axis, idx, shift, scale)
    fp32_term = bound[..., :3] - R.U8 * want[..., :3].abs()
    assert R.ratio(pre, want[..., :3], fp32_term) <= 1.0 and R.ratio(pre, want[..., :3], bound[..., :3]) <= 0.5
    got, _ = R.gather(x, c, axis, idx, shift, scale, model=True)
    assert R.ratio(got, want, bound) <= 1.0


def test_gather_transposed_on_axis_1_is_rejected():
    shift, scale = _scaling()
    for c in (1, 3):
        x, idx = _gather_case(R.EDGE_VOLUME, c, 1, False)
        want, bound = R.gather(x, c, 1, idx, shift, scale)
        assert R.ratio(R.gather(x, c, 1, idx, shift, scale, model=True)[0], want, bound) <= 1.0
        assert R.ratio(R.gather(x, c, 1, idx, shift, scale, model=True, fault="transposed")[0], want, bound) > 1.0


SCATTER_CASES = GATHER_CASES


def _scatter_case(shape, c, axis, loop):
    idx = R.loop_indices() if loop else R.edge_indices(R.extent(shape, axis), unique=True)
    a, b = R.pixel_axes(shape, axis)
    return R.volume(shape, c, 20 + axis), R.slice_grads(idx.numel(), a, b, 30 + axis), idx


@pytest.mark.parametrize("shape,c,axis,loop", SCATTER_CASES)
def test_scatter_closed_form_and_model(shape, c, axis, loop):
    _, scale = _scaling()
    dx, ds, idx = _scatter_case(shape, c, axis, loop)
    want, bound, touched = R.scatter_add(dx, ds, c, axis, idx, scale)
    ok = (idx >= 0) & (idx < R.extent(shape, axis))
    assert int(touched.sum()) == int(ok.sum()) * ds.shape[1] * ds.shape[2]
    old = dx[..., :c].double()
    assert torch.equal(want[~touched], old[~touched]) and not bool(bound[~touched].any())
    if not loop:  # the adjoint of the gather's linear part: <G x, y> = <x, G^T y> on random x
        x = R.volume(shape, c, 99)
        gx = R.gather(x, c, axis, idx, torch.zeros(3), scale)[0]
        gty = R.scatter_add(torch.zeros_like(dx), ds, c, axis, idx, scale)[0]
        lhs, rhs = float((gx[..., :3] * ds[..., :3].double()).sum()), float((x[..., :c].double() * gty).sum())
        assert abs(lhs - rhs) <= 1e-10 * abs(lhs)
    got, _, _ = R.scatter_add(dx, ds, c, axis, idx, scale, model=True)
    assert R.ratio(got, want, bound) <= 1.0
    assert torch.equal(got[~touched], old[~touched])
    # before the output rounding: fp32 arithmetic against the fp32 term alone
    sel = touched
    fp32_term = bound - R.U8 * want.abs()
    r = 1.0 / scale.view(3)
    g = ds[..., :3].float()
    osl = R.as_slices(dx[..., :c].float(), axis)
    valid = idx[ok].long()
    pre = osl.clone()
    if c == 3:
        pre[valid] = osl[valid] + g[ok] * r
    else:
        pre[valid] = ((osl[valid] + g[ok][..., :1] * r[0]) + g[ok][..., 1:2] * r[1]) + g[ok][..., 2:3] * r[2]
    pre = R.from_slices(pre, axis, tuple(dx.shape[:4]) + (c,)).double()
    assert R.ratio(pre[sel], want[sel], fp32_term[sel]) <= 1.0 and R.ratio(pre[sel], want[sel], bound[sel]) <= 0.5


def test_scatter_taking_only_g0_is_rejected():
    _, scale = _scaling()
    for axis in range(3):
        dx, ds, idx = _scatter_case(R.EDGE_VOLUME, 1, axis, False)
        want, bound, _ = R.scatter_add(dx, ds, 1, axis, idx, scale)
        assert R.ratio(R.scatter_add(dx, ds, 1, axis, idx, scale, model=True)[0], want, bound) <= 1.0
        assert R.ratio(R.scatter_add(dx, ds, 1, axis, idx, scale, model=True, fault="g0_only")[0], want, bound) > 1.0


POOL_SHAPES = [(3, 7, 10, 16), (3, 7, 9, 16), (2, 1, 9, 16), (2, 7, 1, 16), (2, 8, 6, 8)]


def _pool_inputs(shape, ints=True):
    g = torch.Generator().manual_seed(sum(shape))
    n, h, w, c = shape
    z = torch.randint(-2, 3, shape, generator=g).to(BF16)   # small integers: ties inside most windows, many zeros
    mk = (lambda s: torch.randint(-3, 4, s, generator=g).to(BF16)) if ints else (lambda s: torch.randn(s, generator=g).to(BF16))
    return z, mk((n, h // 2, w // 2, c)), mk(shape)


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_relu_pool_closed_form_equals_torch(shape):
    z, dp, dadd = _pool_inputs(shape, ints=False)
    a, p = R.relu_pool_fwd(z)
    zc = z.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    a_ref = F.relu(zc)
    cl = lambda t: t.permute(0, 2, 3, 1)
    assert torch.equal(a.double(), cl(a_ref.detach()))
    loss = (a_ref * dadd.double().permute(0, 3, 1, 2)).sum()
    if p.numel():
        p_ref = F.max_pool2d(a_ref, 2, 2)
        assert torch.equal(p.double(), cl(p_ref.detach()))
        loss = loss + (p_ref * dp.double().permute(0, 3, 1, 2)).sum()
    else:
        assert p.shape == (shape[0], shape[1] // 2, shape[2] // 2, shape[3])
    loss.backward()
    dx = R.relu_pool_bwd(a, dp, dadd)
    assert torch.equal(dx, cl(zc.grad)), "torch routes a window's gradient to its first maximum in scan order too"
    # ReLU backward alone, and the pooled gradient alone
    assert torch.equal(R.relu_pool_bwd(a, None, dadd), dadd.double() * (a > 0))
    assert torch.equal(R.relu_pool_bwd(a, dp, None) + R.relu_pool_bwd(a, None, dadd), dx)
    # integer gradients: the bf16 result is exact; Gaussian ones: one rounding
    zi, dpi, daddi = _pool_inputs(shape, ints=True)
    ai, _ = R.relu_pool_fwd(zi)
    exact = R.relu_pool_bwd(ai, dpi, daddi)
    assert torch.equal(R.bf16_round(exact).double(), exact)
    assert R.ratio(R.bf16_round(dx), dx, R.U8 * dx.abs()) <= 1.0


def test_pool_faults_are_rejected():
    shape = (3, 7, 9, 16)
    z, dp, dadd = _pool_inputs(shape, ints=True)
    a, p = R.relu_pool_fwd(z)
    bad, _ = R.relu_pool_fwd(z, fault="odd_row_unrectified")
    assert not torch.equal(bad, a) and torch.equal(bad[:, :-1], a[:, :-1])
    want = R.relu_pool_bwd(a, dp, dadd)
    got = R.relu_pool_bwd(a, dp, dadd, fault="last_maximum")
    assert not torch.equal(got, want), "ties inside the windows must tell the first maximum from the last"
    assert R.ratio(got, want, R.U8 * want.abs()) > 1.0


HEAD_CASES = [(c, loop) for c in R.HEAD_CHANNELS for loop in (False, True)]


@pytest.mark.parametrize("c,loop", HEAD_CASES)
def test_head_closed_form_and_model(c, loop):
    npix = R.head_pixels(c, loop)
    if loop:
        assert npix * (c // 8) > R.HEAD_GROUPS
    f0, f1, w = R.head_inputs(npix, c, c)
    loss, df, bound = R.head(f0, f1, w, 0.7)
    assert bool(torch.isfinite(df).all()) and bool(df[5].abs().max() > 0)
    if not loop:  # torch fp64 autograd, away from the zero-norm pixels (0 * inf there)
        x = f0.double().clone().requires_grad_(True)
        y = f1.double()
        eps = float(torch.tensor(1e-10, dtype=F32))
        nx = x / (torch.sqrt((x ** 2).sum(-1, keepdim=True)) + eps)
        ny = y / (torch.sqrt((y ** 2).sum(-1, keepdim=True)) + eps)
        ref = float(torch.tensor(0.7, dtype=F32)) * (((nx - ny) ** 2) * w.double()).sum(-1).mean()
        ref.backward()
        keep = torch.ones(npix, dtype=torch.bool)
        keep[[5, npix - 3]] = False
        assert abs(loss - float(ref.detach())) <= 1e-12 * abs(float(ref.detach()))
        assert float((df[keep] - x.grad[keep]).abs().max()) <= 1e-12 * float(x.grad[keep].abs().max())
    mloss, mdf, _ = R.head(f0, f1, w, 0.7, model=True)
    assert abs(mloss - loss) <= 0.5e-4 * abs(loss)
    assert R.ratio(mdf, df, bound) <= 1.0
    # before the output rounding: the fp32 arithmetic against half of the fp32 term
    u, v, wl = f0.float(), f1.float(), w.float().view(1, -1)
    coef = float(torch.tensor(float(torch.tensor(0.7, dtype=F32)) / npix, dtype=F32))
    eps = float(torch.tensor(1e-10, dtype=F32))
    nu = (u * u).sum(-1, keepdim=True).sqrt()
    i0, i1 = 1.0 / (nu + eps), 1.0 / ((v * v).sum(-1, keepdim=True).sqrt() + eps)
    g = 2.0 * coef * wl * (u * i0 - v * i1)
    t = torch.where(nu > 0, (g * u).sum(-1, keepdim=True) * i0 * i0 / nu.clamp_min(1e-30), torch.zeros_like(nu))
    pre = (g * i0 - u * t).double()
    assert R.ratio(pre, df, bound - R.U8 * df.abs()) <= 1.0 and R.ratio(pre, df, bound) <= 0.5


@pytest.mark.parametrize("c", R.HEAD_CHANNELS)
@pytest.mark.parametrize("fault", ["dot_half_lanes", "no_second_term"])
def test_head_faults_are_rejected(c, fault):
    npix = R.head_pixels(c, False)
    f0, f1, w = R.head_inputs(npix, c, c)
    _, df, bound = R.head(f0, f1, w, 0.7)
    assert R.ratio(R.head(f0, f1, w, 0.7, model=True)[1], df, bound) <= 1.0
    assert R.ratio(R.head(f0, f1, w, 0.7, model=True, fault=fault)[1], df, bound) > 1.0


def test_a_missing_number_fails():
    want = torch.ones(4, dtype=F64)
    for bad in (float("nan"), float("inf")):
        got = want.clone()
        got[2] = bad
        assert R.ratio(got, want, torch.full((4,), 0.1, dtype=F64)) == float("inf")
    assert R.ratio(torch.tensor([1e-30]), torch.zeros(1), torch.zeros(1)) == float("inf")   # a zero bound asks for the exact value
