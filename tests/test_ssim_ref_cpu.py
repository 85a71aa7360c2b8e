"""The instruments of tests/test_ssim_kernels_gpu.py (tests/ssim_ref.py), checked without a GPU: the restated tiling, pool and
finalize agree with the whole-volume restatements that already existed; the per-tile bound is the one its derivation gives, and correct
fp32 arithmetic reaches half of it at every shape and input family the GPU test runs; and each planted fault -- what a subtly wrong
k_ssim_pairs would do -- is rejected by the same comparer at the same bound, where the fault-free model passes."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import ssim_ref as R

F32, F64 = torch.float32, torch.float64
BY_NAME = {c[0]: c for c in R.PAIR_CASES}


@pytest.fixture(scope="module")
def runs():
    """(case name, data range, family) -> (fp64 partials, plain fp32 partials, counts), computed once."""
    out = {}
    for name, sd, ch, ext, kw, ranges in R.PAIR_CASES:
        ker = R.kernel(sd, **kw)
        for dr in ranges:
            for fam in R.FAMILIES:
                x, y = R.pair_inputs(*R.make_bases(fam, ch, ext, dr))
                want, counts = R.tile_partials(x, y, ker, dr)
                plain, _ = R.tile_partials(x, y, ker, dr, dtype=F32)
                out[name, dr, fam] = (want, plain, counts)
    return out


def _err(got, want, counts):
    return float(((got - want).abs() / counts.view(1, -1, 1)).max())


def test_the_bound_is_the_one_its_derivation_gives(runs):
    worst = {}
    for (name, dr, fam), (want, plain, counts) in runs.items():
        worst[fam] = max(worst.get(fam, 0.0), _err(plain, want, counts))
    print("worst per-tile-mean error of the plain fp32 restatement, per family:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert R.TILE_BOUND == R.tile_bound(max(worst.values()))
    assert R.TILE_BOUND <= R.TILE_BOUND_CAP == 1e-4
    # the figures the constant's comment quotes
    assert max(worst[f] for f in ("ell", "noise", "anti", "ident")) < 2e-5 and 1e-3 < worst["const"] < 1e-2


def test_fp32_arithmetic_reaches_half_the_bound(runs):
    """The plain restatement everywhere but on constant inputs, where its variance terms cancel against c2; there a formulation that
    does not cancel -- the moments about the tile's first voxel -- is exact in cs and inside half the bound in ssim."""
    for (name, dr, fam), (want, plain, counts) in runs.items():
        if fam != "const":
            r = R.tile_ratios(plain, want, counts)
            assert max(r.values()) <= 0.5, (name, dr, fam, r)
    for name, sd, ch, ext, kw, ranges in R.PAIR_CASES:
        ker = R.kernel(sd, **kw)
        x, y = R.pair_inputs(*R.make_bases("const", ch, ext, ranges[-1]))
        want, _, counts = runs[name, ranges[-1], "const"]
        got, _ = R.tile_partials(x, y, ker, ranges[-1], dtype=F32, shifted=True)
        r = R.tile_ratios(got, want, counts)
        assert max(r.values()) <= 0.5, (name, r)
        assert torch.equal(got[..., 1], counts.view(1, -1).expand(got.shape[0], -1)), "cs of constant inputs, moments about the origin"


@pytest.mark.parametrize("name", ["ragged_c2", "k11_chunks32", "2d_uniform7"])
def test_the_restatement_about_the_tile_origin_is_the_same_function(name):
    """shifted=True takes the moments about each tile's first voxel; in fp64 it equals the plain statement."""
    _, sd, ch, ext, kw, ranges = BY_NAME[name]
    ker = R.kernel(sd, **kw)
    x, y = R.pair_inputs(*R.make_bases("ell", ch, ext))
    a, counts = R.tile_partials(x, y, ker)
    b, _ = R.tile_partials(x, y, ker, shifted=True)
    assert _err(a, b, counts) <= 1e-12


def test_raw_moments_about_the_tile_origin_cancel_on_a_shared_flat_background(runs):
    """What the per-tile test found in k_ssim_pairs: raw moments about the tile's first voxel are exact on constant inputs, but two
    ellipsoid volumes share a zero background, and in a tile that starts inside the object that background is a flat region away from
    the origin -- E[x^2] - E[x]^2 cancels there as it does for the plain statement on constants, and the tile mean misses the bound."""
    _, sd, ch, ext, kw, ranges = BY_NAME["2d_k11"]
    x, y = R.pair_inputs(*R.make_bases("ident", ch, ext))
    want, plain, counts = runs["2d_k11", 1.0, "ident"]
    got, _ = R.tile_partials(x, y, R.kernel(sd, **kw), dtype=F32, shifted=True)
    assert max(R.tile_ratios(plain, want, counts).values()) <= 0.5 < 1.0 < max(R.tile_ratios(got, want, counts).values())


def test_tiling_restated_from_the_launch_code():
    assert R.tiling((19, 19, 35), (4, 4, 4)) == ((16, 16, 32), 16, (1, 1, 1))
    assert R.tiling((21, 22, 37), (4, 4, 4)) == ((18, 19, 34), 16, (2, 2, 2))
    assert R.tiling((20, 19, 36), (4, 4, 4)) == ((17, 16, 33), 16, (2, 1, 2))
    assert R.tiling((44, 27, 43), (11, 11, 11)) == ((34, 17, 33), 32, (2, 2, 2))   # kD > 5: 32-deep chunks; 16 + 11 - 1 = 26 window rows
    assert R.tiling((1, 61, 77), (1, 11, 11))[2] == (1, 4, 3)
    assert R.depth_chunk(5) == 16 and R.depth_chunk(6) == 32
    # every edge the GPU test's docstring names has its case
    ragged = lambda n: [o % t for o, t in zip(R.tiling(R.dhw(BY_NAME[n][3]), R.dhw(tuple(R.kernel(BY_NAME[n][1], **BY_NAME[n][4]).shape)))[0], (16, R.TH, R.TW))]
    assert ragged("one_full_tile") == [0, 0, 0] and ragged("ragged_c2") == [2, 3, 2] and ragged("w_one_column")[2] == 1


@pytest.mark.parametrize("name", [c[0] for c in R.PAIR_CASES])
def test_tile_partials_sum_to_the_whole_volume_ssim(runs, name):
    _, sd, ch, ext, kw, ranges = BY_NAME[name]
    x, y = R.pair_inputs(*R.make_bases("ell", ch, ext, ranges[-1]))
    want, _, counts = runs[name, ranges[-1], "ell"]
    ref = R.ssim(x, y, sd, data_range=ranges[-1], **kw)[:, 0]
    assert float((want[..., 0].sum(1) / counts.sum() - ref).abs().max()) <= 1e-12
    assert want.shape[1] == ch * R.tiles_per_channel(R.dhw(ext), R.dhw(tuple(R.kernel(sd, **kw).shape)))


@pytest.mark.parametrize("sd,ext,weights", [(2, (70, 81), (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)), (3, (21, 22, 37), (0.4, 0.6)),
                                            (3, (19, 19, 35), (1.0,))])
def test_finalize_of_restated_partials_is_ms_ssim(sd, ext, weights):
    kw = dict(kernel_size=4)
    ker = R.kernel(sd, **kw)
    x, y = R.pair_inputs(*R.make_bases("ell", 2, ext))
    parts, tiles, counts = [], [], []
    xs, ys = x.double(), y.double()
    for s in range(len(weights)):
        p, c = R.tile_partials(xs, ys, ker)
        parts.append(p), tiles.append(p.shape[1]), counts.append(float(c.sum()))
        if s + 1 < len(weights):
            flat = lambda t: t.reshape(-1, *R.dhw(tuple(t.shape[2:])))
            xs, ys = (R.pool2(flat(t), sd == 3)[0].reshape(t.shape[0], t.shape[1], *[e // 2 for e in t.shape[2:]]) for t in (xs, ys))
    ms, ss = R.finalize(torch.cat(parts, 1), tiles, counts, weights)
    assert float((ms - R.ms_ssim(x, y, sd, weights=weights, **kw)[:, 0]).abs().max()) <= 1e-12
    assert float((ss - R.ssim(x, y, sd, **kw)[:, 0]).abs().max()) <= 1e-12


def test_finalize_relu_pow_product_and_nan():
    part = torch.tensor([[[2.0, 3.0], [2.0, 1.0], [6.0, -8.0], [1.0, 9.0]]], dtype=F64).repeat(3, 1, 1)   # scales of 2, 1, 1 tiles
    part[1, 2, 1] = 8.0
    part[2, 0, 1] = math.nan
    ms, ss = R.finalize(part, [2, 1, 1], [4.0, 16.0, 2.0], [0.5, 2.0, 1.0])
    assert float(ms[0]) == 0.0                                        # cs mean of scale 1 is -0.5: relu, then pow, then product
    assert float(ms[1]) == pytest.approx(1.0 ** 0.5 * 0.5 ** 2 * 0.5)  # cs, cs, then ssim of the last scale
    assert math.isnan(float(ms[2])) and float(ss[2]) == 1.0 and float(ss[0]) == 1.0
    only_ss = R.finalize(part, [2], [4.0])
    assert only_ss[0] is None and torch.equal(only_ss[1], ss)
    got = torch.tensor([1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -22, math.nan, 0.5], dtype=F32)
    want = torch.tensor([1.0, 1.0, 1.0, math.nan, math.nan], dtype=F64)
    assert R.within_one_ulp_f32(got, want).tolist() == [True, True, False, True, False]


@pytest.mark.parametrize("shape,pool_d", [((3, 5, 7, 9), 1), ((3, 5, 7, 9), 0), ((3, 1, 7, 9), 0), ((2, 3, 2, 3), 1)])
def test_pool2_is_the_floor_average_pool(shape, pool_d):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(3)) * 2 - 0.5
    p64, p32 = R.pool2(x, pool_d)
    ref = F.avg_pool3d(x.double(), 2) if pool_d else F.avg_pool2d(x.double().flatten(0, 1), 2).view(shape[0], shape[1], shape[2] // 2, shape[3] // 2)
    assert p64.shape == ref.shape and float((p64 - ref).abs().max()) <= 1e-15
    assert p32.dtype == F32 and float((p32.double() - p64).abs().max()) <= 0.5 * 4 * 2.0 ** -24 * float(x.abs().max())


FAULTS = [  # fault, case, family: where the fault-free fp32 model passes and the fault must not
    ("ragged_w_column", "ragged_c2", "ell"), ("ragged_w_column", "w_one_column", "noise"), ("ragged_w_column", "2d_k4", "anti"),
    ("ragged_d_plane", "ragged_c2", "ell"), ("ragged_d_plane", "k11_chunks32", "anti"),
    ("chunk2_plane_twice", "ragged_c2", "ell"), ("chunk2_plane_twice", "k11_chunks32", "ell"),
    ("other_channel", "ragged_c2", "ell"), ("other_channel", "ragged_c2", "noise"),
    ("pair_swap", "one_full_tile", "ell"), ("pair_swap", "2d_k11", "noise"),
    ("no_origin_shift", "one_full_tile", "noise"), ("no_origin_shift", "2d_uniform7", "ell"),
    ("voxel", "one_full_tile", "ident"),
]


@pytest.mark.parametrize("fault,name,fam", FAULTS)
def test_planted_fault_misses_the_bound(runs, fault, name, fam):
    _, sd, ch, ext, kw, ranges = BY_NAME[name]
    ker = R.kernel(sd, **kw)
    want, plain, counts = runs[name, ranges[-1], fam]
    assert max(R.tile_ratios(plain, want, counts).values()) <= 1.0, "the fault-free model must pass where the fault is planted"
    xb, yb = R.make_bases(fam, ch, ext, ranges[-1])
    x, y = R.pair_inputs(xb, yb, swapped=(fault == "pair_swap"))
    got, _ = R.tile_partials(x, y, ker, ranges[-1], dtype=F32, fault=None if fault == "pair_swap" else fault)
    r = R.tile_ratios(got, want, counts)
    print(f"{fault} at {name} / {fam}: err / bound {r}")
    assert max(r.values()) > 1.0, (fault, r)


def test_a_fault_needs_a_tile_to_sit_in_and_a_missing_number_fails(runs):
    _, sd, ch, ext, kw, _ = BY_NAME["one_full_tile"]
    x, y = R.pair_inputs(*R.make_bases("ell", ch, ext))
    for fault in ("ragged_w_column", "ragged_d_plane", "chunk2_plane_twice", "other_channel"):
        with pytest.raises(ValueError):
            R.tile_partials(x, y, R.kernel(sd, **kw), fault=fault)
    want, plain, counts = runs["one_full_tile", 1.0, "ell"]
    for bad in (math.nan, math.inf):
        g = plain.clone()
        g[2, 0, 1] = bad
        assert R.tile_ratios(g, want, counts)["cs"] == math.inf
