"""The three kernels of csrc/metrics.hip, called through the C ABI and held per tile / per element to the fp64 restatements of
tests/ssim_ref.py (tests/test_ssim_ref_cpu.py checks those restatements, the bound and the planted faults without a GPU).

k_ssim_pairs (mi_ssim_pairs): one (sum ssim, sum cs) pair per 16 x 32 x DC output tile.  Every case runs two separate bases of three
images, the pair list [(2,0), (0,1), (2,0), (1,1)], part_off = 3 and a part_stride wider than the tiles, into a partial buffer
prefilled with a sentinel: every slot outside [part_off, part_off + tiles) must come back bit for bit.  The restated tile count is
asserted against mi_ssim_tiles, so a tiling change fails here instead of silently moving the edges.  Shapes (ssim_ref.PAIR_CASES), the
smallest at which each edge exists:
  (19,19,35) k4        exactly one full tile (16 x 16 x 32 outputs), nothing ragged -- the one-voxel fault's tile
  (21,22,37) k4, C=2   two tiles per axis, ragged 2 / 3 / 2; the channel index of the tile order; data ranges 1 and 2
  (20,19,36) k4        the second W tile is one column wide
  (44,27,43) k11       32-deep chunks, two per axis; the window is 26 rows = RH, the LDS limit
  (37,30,40) (4,11,7)  mixed taps and sigmas
  (3,23,37)  (1,5,3)   kD = 1 on a 3-D volume
  (61,77)    k4, k11, uniform k7: the 2-D path
Inputs: ellipsoid against ellipsoid + noise, noise against noise, anti-correlated, constant (0.7 against 0.3) and identical.
k_ssim_pool2: odd extents on every axis, pool_d 0 / 1, NC = 3, bit-equal to the fixed-order fp32 statement and within 4 * 2^-24 max|x|
of the fp64 pool; NC = 3 of 1700 x 1000 (the size the pyramid of a large slice has) and 3 x 1701 x 2001 = 2 550 000 outputs, more than
the 8192 x 256 threads of the capped grid, so the grid-stride loop makes a second trip.
k_ssim_finalize: hand-built partials, S = 1, 5, 8 with uneven tile counts, P = 257 (a second workgroup), a negative cs mean at scale 1
(MS-SSIM exactly 0), a NaN partial (NaN out), each output alone, and the refusals; results within one fp32 ulp of the fp64 restatement.
Not covered: the pair chunking at 2^22 workgroups per launch (MAX_BLOCKS) needs 2^22 / tiles pairs -- out of reach at test size;
test_metrics_gpu.py::test_pairwise_at_reference_3d_scale stays the only run with many pairs (780 x 512 tiles, still one launch).

Measured on the MI355X (table in EXPERIMENTS.md): tile counts equal mi_ssim_tiles at every shape.  k_ssim_pairs, worst err / bound
over all cases, families and data ranges: ssim 0.005, cs 0.001 of the 1e-4 bound (5e-7 absolute; cs of constant inputs exactly the
count).  That is after a kernel change this test forced: with raw moments about the tile's first voxel the `ident` family stood at
1.19 (44,27,43) k11, 1.40 (61,77) k11 and 1.32 (61,77) uniform k7 -- the flat zero background two volumes share, in tiles that start
inside the object.  k_ssim_pool2: 0 of up to 2 550 000 outputs differ from the fixed-order statement; 8.9e-8 from the fp64 pool
(bound 3.6e-7).  k_ssim_finalize: every result within one fp32 ulp.  Slowest test: test_pairs_per_tile[k11_chunks32], 4.4 s (the
fp64 dense 11^3 reference of five families on the CPU); every other under 1.4 s.
"""
import ctypes as C
import time

import pytest
import torch

from tests import ssim_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e300


def _lib():
    from medical_image_generation_amd import _lib
    return _lib


def _taps(sd, kw, dr):
    from medical_image_generation_amd.metrics import SSIMMetric
    m = SSIMMetric(sd, data_range=dr, **kw)
    return m, m._tap_table(torch.device("cuda"))


@pytest.mark.parametrize("case", R.PAIR_CASES, ids=lambda c: c[0])
def test_pairs_per_tile(case):
    L = _lib()
    name, sd, ch, ext, kw, ranges = case
    ker = R.kernel(sd, **kw)
    d, h, w = R.dhw(ext)
    kd, kh, kw_ = R.dhw(tuple(ker.shape))
    per_c = R.tiles_per_channel((d, h, w), (kd, kh, kw_))
    assert per_c == L.call_raw("mi_ssim_tiles", d, h, w, kd, kh, kw_), "the restated tiling is not the kernel's"
    tiles, off, P = ch * per_c, 3, len(R.PAIRS)
    stride = off + tiles + 5
    pairs = torch.tensor(R.PAIRS, dtype=torch.int32).cuda()
    t0, worst, missed = time.time(), {}, []
    for dr in ranges:
        m, taps = _taps(sd, kw, dr)
        c1, c2 = m._constants()
        for fam in R.FAMILIES:
            xb, yb = R.make_bases(fam, ch, ext, dr)
            x, y = R.pair_inputs(xb, yb)
            want, counts = R.tile_partials(x, y, ker, dr)
            assert want.shape[1] == tiles and float(counts.sum()) == ch * (d - kd + 1) * (h - kh + 1) * (w - kw_ + 1)
            part = torch.full((P, stride, 2), SENTINEL, dtype=torch.float64, device="cuda")
            xd, yd = xb.cuda(), yb.cuda()
            L.call("mi_ssim_pairs", xd.data_ptr(), yd.data_ptr(), pairs.data_ptr(), P, ch, d, h, w, taps.data_ptr(), kd, kh, kw_, c1, c2,
                   part.data_ptr(), stride, off)
            got = part.cpu()
            fence = torch.cat([got[:, :off], got[:, off + tiles:]], 1)
            assert torch.equal(fence.view(torch.int64), torch.full_like(fence, SENTINEL).view(torch.int64)), (name, fam, "a slot outside the tiles changed")
            got = got[:, off:off + tiles]
            r = R.tile_ratios(got, want, counts)
            print(f"SSIMTILE {name} L={dr} {fam}: err / bound ssim {r['ssim']:.3f} cs {r['cs']:.3f}  (tiles {tiles}, bound {R.TILE_BOUND:.1e})")
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            if not (r["ssim"] <= 1.0 and r["cs"] <= 1.0):
                missed.append((dr, fam, r))
            if fam == "const":  # every moment about the tile's origin is 0: cs = c2 / c2 per voxel, and the sums of ones are exact
                assert torch.equal(got[..., 1], counts.view(1, -1).expand(P, -1)), (name, "cs of constant inputs is not exactly 1 per voxel")
            if fam == "ident":  # PAIRS[3] is an image against itself
                dev = float(((got[3, :, 0] - counts).abs() / counts).max())
                assert dev <= R.TILE_BOUND, (name, "ssim of identical inputs", dev)
            assert torch.equal(got[0], got[2]), (name, fam, "the repeated pair scored differently")
    print(f"SSIMTILE {name} worst ratio ssim {worst['ssim']:.3f} cs {worst['cs']:.3f}; {time.time() - t0:.2f} s")
    assert not missed, (name, missed)


POOL_CASES = [  # NC, D, H, W, pool_d
    (3, 5, 7, 9, 1), (3, 5, 7, 9, 0), (3, 1, 7, 9, 0), (3, 3, 2, 3, 1), (3, 1, 1700, 1000, 0), (3, 1, 1701, 2001, 0),
]


@pytest.mark.parametrize("nc,d,h,w,pool_d", POOL_CASES)
def test_pool2_bit_equal_to_the_fixed_order_statement(nc, d, h, w, pool_d):
    L = _lib()
    g = torch.Generator().manual_seed(d * 1000 + h + w)
    x = (torch.rand((nc, d, h, w), generator=g) * 2 - 0.5).float()
    want64, want32 = R.pool2(x, pool_d)
    n_out = want32.numel()
    if (h, w) == (1701, 2001):
        assert n_out > R.POOL_GRID, "this case exists for the second trip of the grid-stride loop"
    guard = 64
    y = torch.full((n_out + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda")
    xd = x.cuda()
    L.call("mi_ssim_pool2", xd.data_ptr(), y.data_ptr() + 4 * guard, nc, d, h, w, pool_d)
    y = y.cpu()
    assert bool(torch.isnan(y[:guard]).all()) and bool(torch.isnan(y[-guard:]).all()), "a guard element changed"
    got = y[guard:-guard].view(want32.shape)
    assert torch.equal(got, want32), f"{int((got != want32).sum())} of {n_out} outputs differ from the fixed-order fp32 statement"
    err = float((got.double() - want64).abs().max())
    print(f"SSIMPOOL {(nc, d, h, w)} pool_d={pool_d}: outputs {n_out}, max |err| vs fp64 {err:.3e}, bound {4 * 2.0 ** -24 * float(x.abs().max()):.3e}")
    assert err <= 4 * 2.0 ** -24 * float(x.abs().max())


def _hand_partials(P, tiles, counts, stride, seed):
    """Tile sums whose means sit in (0.2, 1): count / tiles per tile, times a random factor."""
    g = torch.Generator().manual_seed(seed)
    part = torch.full((P, stride, 2), SENTINEL, dtype=torch.float64)
    off = 0
    for nt, cnt in zip(tiles, counts):
        part[:, off:off + nt] = (0.2 + 0.8 * torch.rand((P, nt, 2), generator=g, dtype=torch.float64)) * (cnt / nt)
        off += nt
    return part


def _finalize(L, part_d, P, stride, tiles, counts, weights, ms, ss):
    S = len(tiles)
    ht, hc = (C.c_int * S)(*tiles), (C.c_double * S)(*counts)
    hw = (C.c_double * S)(*weights) if weights is not None else None
    L.call("mi_ssim_finalize", part_d.data_ptr(), P, stride, S, ht, hc, hw, None if ms is None else ms.data_ptr(),
           None if ss is None else ss.data_ptr())


FIN_CASES = {1: ([7], [1234.0], [1.0]),
             5: ([16, 5, 2, 1, 3], [40000.0, 5000.0, 601.0, 77.0, 9.0], [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]),
             8: ([9, 1, 4, 2, 7, 1, 1, 3], [9e5, 1e5, 12345.0, 1500.0, 190.0, 23.0, 3.0, 1.0], [0.05, 0.1, 0.15, 0.2, 0.2, 0.1, 0.1, 0.1])}


@pytest.mark.parametrize("S", [1, 5, 8])
def test_finalize_within_one_ulp(S):
    L = _lib()
    assert max(FIN_CASES) == R.MAX_SCALES
    tiles, counts, weights = FIN_CASES[S]
    P, stride = 257, sum(tiles) + 4   # 257 pairs: a second workgroup with one live thread
    part = _hand_partials(P, tiles, counts, stride, S)
    if S > 1:
        part[5, tiles[0]:tiles[0] + tiles[1], 1] *= -1.0          # pair 5: the cs mean of scale 1 is negative
    part[256, 1] = float("nan")                                    # pair 256 (the second workgroup's): a NaN tile at scale 0
    want_ms, want_ss = R.finalize(part, tiles, counts, weights)
    part_d = part.cuda()
    ms = torch.full((P + 2,), -5.0, device="cuda")
    ss = torch.full((P + 2,), -5.0, device="cuda")
    _finalize(L, part_d, P, stride, tiles, counts, weights, ms[1:], ss[1:])
    for name, got, want in (("ms", ms, want_ms), ("ssim", ss, want_ss)):
        got = got.cpu()
        assert float(got[0]) == -5.0 and float(got[-1]) == -5.0, "a guard element changed"
        ok = R.within_one_ulp_f32(got[1:-1], want)
        assert bool(ok.all()), (name, S, int((~ok).sum()), got[1:-1][~ok][:4], want[~ok][:4])
    assert torch.isnan(ms[1:][256]) and torch.isnan(ss[1:][256]), "the NaN partial did not come out"
    if S > 1:
        assert float(ms[1:][5]) == 0.0 and float(want_ms[5]) == 0.0, "relu of a negative cs mean must zero the product"
    assert bool(torch.isfinite(ms[1:-1][:256]).all())
    # each output alone equals the joint call bit for bit (the SSIM-alone call passes no weights, as metrics.py issues it)
    ms1 = torch.full((P,), -5.0, device="cuda")
    ss1 = torch.full((P,), -5.0, device="cuda")
    _finalize(L, part_d, P, stride, tiles, counts, weights, ms1, None)
    _finalize(L, part_d, P, stride, tiles, counts, None, None, ss1)
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(ms1, ms[1:-1]) and same(ss1, ss[1:-1])
    assert torch.equal(part_d.cpu().view(torch.int64), part.view(torch.int64)), "finalize wrote into the partials"


def test_finalize_refusals():
    L = _lib()
    bad = "MI_ERR_BAD_ARG"
    tiles, counts, weights = FIN_CASES[8]
    P, stride = 4, sum(tiles) + 2
    part_d = _hand_partials(P, tiles, counts, stride, 0).cuda()
    out = torch.full((P,), -5.0, device="cuda")
    with pytest.raises(L.HipError, match=bad):   # S = 9 = MAX_SCALES + 1
        _finalize(L, part_d, P, stride + 1, tiles + [1], counts + [1.0], weights + [0.1], out, out)
    with pytest.raises(L.HipError, match=bad):   # a zero tile count
        _finalize(L, part_d, P, stride, tiles[:3] + [0] + tiles[4:], counts, weights, out, out)
    with pytest.raises(L.HipError, match=bad):   # more tiles than the stride holds
        _finalize(L, part_d, P, sum(tiles) - 1, tiles, counts, weights, out, out)
    with pytest.raises(L.HipError, match=bad):   # nothing to write
        _finalize(L, part_d, P, stride, tiles, counts, weights, None, None)
    torch.cuda.synchronize()
    assert bool((out.cpu() == -5.0).all()), "a refused call wrote"
