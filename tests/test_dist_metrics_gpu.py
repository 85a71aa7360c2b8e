"""FID / MMD / KID on the HIP path (metrics.py, csrc/distmetrics.hip) against the fp64 restatements in tests/dist_ref.py.

Tolerance: absolute error <= 1e-10 * scale against the restatement of the same form, with scale = |mu_x - mu_y|^2 + tr S_x + tr S_y for
FID and the sum of the absolute values of the three terms for MMD and KID.  Products of fp32 inputs are exact in fp64; a fixed-order
fp64 sum over K <= 4e4 terms is off by at most K * 2^-53 (about 4e-12 relative); Jacobi adds about c * sweeps * 2^-53 (under 1e-12):
1e-10 leaves about 20x over the worst case.  Every test prints its ratio |error| / scale (and the Jacobi sweeps where there are any).

Shapes: R = n + m ragged against the 16-row MFMA tile and K against its 4 columns, odd c (the Jacobi pad column), both orientations of
the cross block, the smallest legal input, R > 64 (the 2-D tile grid and the mirrored triangle), a rank-5 set (zero singular values),
both sides of the single-workgroup Jacobi threshold (r * c' <= 8192 doubles), several K chunks on both Gram grids."""
import functools

import numpy as np
import pytest
import torch

from medical_image_generation_amd import metrics as M
from medical_image_generation_amd._lib import call_raw
from tests import dist_ref

pytestmark = pytest.mark.gpu
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def _features(seed, n, F, rank=None):
    """Correlated features (the covariances are not diagonal): randn(n, F) @ randn(F, F) * 0.3 + 0.5, fp32 on the host."""
    g = torch.Generator().manual_seed(seed)
    w = F if rank is None else rank
    return torch.randn(n, w, generator=g) @ torch.randn(w, F, generator=g) * 0.3 + 0.5


@functools.lru_cache(maxsize=None)
def _sets(n, m, F, rank=None):
    return _features(11, n, F, rank), _features(12, m, F, rank)


@functools.lru_cache(maxsize=None)
def _fid_ref(n, m, F, rank=None):
    x, y = _sets(n, m, F, rank)
    return dist_ref.fid_gram(x.numpy(), y.numpy())


@functools.lru_cache(maxsize=None)
def _images(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g)


def _check(name, got, want, scale, extra=""):
    assert got.dtype == torch.float64 and got.ndim == 0 and got.is_cuda
    ratio = abs(float(got) - want) / scale
    print(f"  {name}: value {want:.9g}  |err| / scale {ratio:.2e}{extra}")
    assert ratio <= TOL, (name, float(got), want, ratio)
    return ratio


def _single_workgroup(n, m):
    return bool(call_raw("mi_dm_jacobi_single_workgroup", n, m))


FID_CASES = [  # (n, m, F, rank, single-workgroup Jacobi)
    (24, 17, 67, None, True),    # R = 41 ragged against the tile, F % 4 != 0, c = 17 odd, singular (n, m < F)
    (17, 24, 67, None, True),    # the transposed orientation
    (2, 2, 5, None, True),       # the smallest legal input: c = 2, a single round
    (70, 45, 130, None, True),   # R = 115: the 2-D tile grid; r * c' = 70 * 46 = 3220 doubles: below the threshold
    (40, 30, 64, 5, True),       # rank 5: zero singular values, alpha * beta = 0 pairs
    (100, 90, 130, None, False),  # r * c' = 9000 doubles: above the threshold, one launch per round
]


@pytest.mark.parametrize("n,m,F,rank,single", FID_CASES)
def test_fid_against_the_gram_restatement(n, m, F, rank, single):
    x, y = _sets(n, m, F, rank)
    want, scale = _fid_ref(n, m, F, rank)
    assert _single_workgroup(n, m) == single
    fid = M.FIDMetric()
    got = fid(x.cuda(), y.cuda())
    path = "single-workgroup sweeps" if single else "one launch per round"
    _check(f"FID ({n}, {m}, {F}, rank {rank})", got, want, scale, f"  Jacobi: {fid.last_sweeps} sweeps, {path}")
    assert 1 <= fid.last_sweeps <= M.MAX_JACOBI_SWEEPS
    terms = fid.last_terms.cpu()
    assert float(terms[0]) == float((terms[1] + terms[2]) - terms[3])


@pytest.mark.parametrize("n,m,F,centred", [(24, 17, 67, True), (70, 45, 130, True), (70, 45, 130, False), (3, 3, 2574, False)])
def test_gram_matrix_per_element(n, m, F, centred):
    """G against numpy per element, both triangles.  Bound: the centred values carry one rounding each, the K products and adds one each:
    |err| <= (K + 3) * 2^-53 * sqrt(G_ii G_jj) by Cauchy-Schwarz (1.5e-14 at K = 130, 2.9e-13 at K = 2574); asserted at 1e-12 max G_ii."""
    x, y = _sets(n, m, F)
    rows = M._Rows(x.cuda(), y.cuda())
    mean = rows.colmean() if centred else None
    G = rows.gram(mean).cpu().numpy()
    x64, y64 = x.double().numpy(), y.double().numpy()
    if centred:
        assert np.abs(mean.cpu().numpy() - np.stack([x64.mean(0), y64.mean(0)])).max() <= 1e-14 * np.abs(x64).max()
        x64, y64 = x64 - x64.mean(0), y64 - y64.mean(0)
    z = np.concatenate([x64, y64])
    want = z @ z.T
    err = np.abs(G - want).max() / want.diagonal().max()
    print(f"  Gram ({n}+{m}) x {F}, centred {centred}: max |err| / max G_ii {err:.2e}, single pass {bool(call_raw('mi_dm_gram_single_pass', n + m))}")
    assert err <= 1e-12
    assert np.array_equal(G, G.T)


def test_fid_of_a_set_with_its_copy_is_zero():
    x, _ = _sets(24, 17, 67)
    _, scale = dist_ref.fid_gram(x.numpy(), x.numpy())
    got = M.FIDMetric()(x.cuda(), x.clone().cuda())
    _check("FID x vs x.clone()", got, 0.0, scale)


def test_fid_full_rank_against_the_sqrtm_form():
    pytest.importorskip("scipy.linalg")
    n, m, F = 64, 48, 16
    x, y = _sets(n, m, F)
    want, scale = _fid_ref(n, m, F)
    upstream, _ = dist_ref.fid_upstream(x.numpy(), y.numpy())
    fid = M.FIDMetric()
    got = fid(x.cuda(), y.cuda())
    _check(f"FID ({n}, {m}, {F})", got, want, scale, f"  Jacobi: {fid.last_sweeps} sweeps")
    rel = abs(float(got) - upstream) / abs(upstream)
    print(f"  against numpy cov + scipy sqrtm: {upstream:.12g}, relative difference {rel:.2e}")
    assert rel <= 1e-9


def test_reference_scale_fid_and_kid():
    """2048 features (the pooled ResNet-50 width), 128 against 100 samples: both covariances singular, the Gram grid has several K chunks,
    the Jacobi block is 128 x 100 (one launch per round)."""
    n, m, F = 128, 100, 2048
    x, y = _sets(n, m, F)
    want, scale = _fid_ref(n, m, F)
    assert not _single_workgroup(n, m)
    fid = M.FIDMetric()
    got = fid(x.cuda(), y.cuda())
    _check(f"FID ({n}, {m}, {F})", got, want, scale, f"  Jacobi: {fid.last_sweeps} sweeps")
    assert fid.last_sweeps <= M.MAX_JACOBI_SWEEPS  # converged inside the cap (reaching it raises)
    want, scale = dist_ref.kid(x.numpy(), y.numpy())
    _check(f"KID ({n}, {m}, {F})", M.KIDMetric()(x.cuda(), y.cuda()), want, scale)


MMD_SHAPES = [
    (5, 1, 40, 33, 29),  # 38280 elements per row: several K chunks, K % 4 == 0, ragged against the chunk
    (3, 2, 13, 11, 9),   # K = 2574
    (4, 1, 61, 77),      # 2-D images
    (12, 1, 50, 50),     # R = 24: two row tiles (three tile pairs) of the single-pass grid over two K chunks
]


@pytest.mark.parametrize("shape", MMD_SHAPES)
def test_mmd_against_the_three_gram_form(shape):
    y, p = _images(21, shape), _images(22, shape) * 0.8 + 0.1
    want, scale = dist_ref.mmd(y.numpy(), p.numpy())
    mmd = M.MMDMetric()
    got = mmd(y.cuda(), p.cuda())
    _check(f"MMD {shape}", got, want, scale)
    t = mmd.last_terms.cpu()
    assert float(t[0]) == float((t[1] + t[2]) - t[3])


def test_mmd_with_a_transform_and_of_a_batch_with_itself():
    shape = MMD_SHAPES[1]
    y, p = _images(21, shape) * 4 - 2, _images(22, shape)
    # the restatement takes the device's sigmoid: the host's fp32 sigmoid differs from it in the last bit (3e-11 of the scale when it
    # was used here), which is a difference of the inputs, not of the metric
    want, scale = dist_ref.mmd(torch.sigmoid(y.cuda()).cpu().numpy(), p.numpy())
    _check("MMD y_transform=sigmoid", M.MMDMetric(y_transform=torch.sigmoid)(y.cuda(), p.cuda()), want, scale)
    want, scale = dist_ref.mmd(p.numpy(), p.numpy())
    _check("MMD y == y_pred", M.MMDMetric()(p.cuda(), p.cuda()), want, scale)


@pytest.mark.parametrize("n,m,F", [(24, 17, 67), (70, 45, 130)])
@pytest.mark.parametrize("kw", [dict(), dict(degree=2, gamma=0.5, coef0=0.0)], ids=["default", "degree2"])
def test_kid_against_the_restatement(n, m, F, kw):
    x, y = _sets(n, m, F)
    want, scale = dist_ref.kid(x.numpy(), y.numpy(), **kw)
    _check(f"KID ({n}, {m}, {F}) {kw}", M.KIDMetric(**kw)(x.cuda(), y.cuda()), want, scale)


def _bits(t):
    return t.cpu().view(torch.int64).tolist()


@pytest.mark.parametrize("n,m,F", [(24, 17, 67), (70, 45, 130), (100, 90, 130)])
def test_distribution_scores_equal_the_separate_calls_bit_for_bit(n, m, F):
    x, y = (t.cuda() for t in _sets(n, m, F))
    fid, kid = M.FIDMetric(), M.KIDMetric()
    both = M.distribution_scores(x, y)
    assert _bits(both["fid"]) == _bits(fid(x, y)) and _bits(both["kid"]) == _bits(kid(x, y))
    assert both["jacobi_sweeps"] == fid.last_sweeps
    assert "kid" not in M.distribution_scores(x, y, kid=False)
    k2 = M.KIDMetric(degree=2, gamma=0.5, coef0=0.0)
    assert _bits(M.distribution_scores(x, y, kid=k2)["kid"]) == _bits(k2(x, y))


def test_two_runs_are_bit_equal():
    x, y = (t.cuda() for t in _sets(100, 90, 130))
    img, img2 = _images(21, MMD_SHAPES[0]).cuda(), _images(22, MMD_SHAPES[0]).cuda()
    for run in (lambda: M.FIDMetric()(x, y), lambda: M.KIDMetric()(x, y), lambda: M.MMDMetric()(img, img2),
                lambda: M.FIDMetric()(x[:24], y[:17])):
        assert _bits(run()) == _bits(run())


def test_other_dtypes_score_as_their_fp32_cast():
    x, y = _sets(24, 17, 67)
    for dtype in (torch.bfloat16, torch.float64):
        xd, yd = (x.double() * 1.0000001).to(dtype).cuda(), (y.double() * 1.0000001).to(dtype).cuda()  # fp64: not representable in fp32
        x32, y32 = xd.float(), yd.float()
        assert _bits(M.FIDMetric()(xd, yd)) == _bits(M.FIDMetric()(x32, y32))
        assert _bits(M.KIDMetric()(xd, yd)) == _bits(M.KIDMetric()(x32, y32))
        img = xd.reshape(24, 1, 67)
        assert _bits(M.MMDMetric()(img, img * 0.5)) == _bits(M.MMDMetric()(img.float(), (img * 0.5).float()))
