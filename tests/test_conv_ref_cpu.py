"""The conv reference, inputs and comparer of tests/conv_ref.py, checked without a GPU: fp32 torch passes both input kinds, and every
modelled kernel defect is reported by the comparer -- at the 20x32x32 weight-gradient shape, where a workgroup walks several tiles, and
at 8^3.  The same table shows why the measure of test_conv_fwd_dgrad_wgrad (max |err| <= 1e-2 max |ref| per tensor) cannot stand in for it.

Figures (32 -> 32 channels, k3 s1 p1, one image; printed by test_defects_are_reported, run with -s):
    20x32x32, gauss inputs: max |dw| = 610, so the old tolerance is 6.1; one dropped or doubled (voxel, tap, channel) product moves one
              entry by 0.97 (0.16 of the tolerance), a halo row shifted by one voxel moves the worst entry by 17.7, skipping the last
              tile by 77.7.
    20x32x32, ints inputs:  max |dw| = 722 (tolerance 7.2); a dropped / doubled product moves one entry by 0.031, the shifted halo row
              moves 2993 entries by up to 3.75 -- inside the old tolerance as well -- and the skipped tile 27 545 entries by up to 18.3.
    8^3, ints inputs:       max |dw| = 25.8 (tolerance 0.26): a dropped product moves 0.125, the shifted row 2.3, the skipped tile 17.4.
The old measure therefore passes the first two defects at 20x32x32 with either kind of input (and the third with `ints`); the comparer
reports all seven at both shapes: 1 / 1 / 2993 / 27 545 unequal entries, an unwritten voxel as infinitely wrong, a store past the slot as a
broken fence, and truncation as 25 154 of 655 360 unequal elements.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R

K3, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
SHAPES = [(1, 32, 32, (20, 32, 32)), (1, 32, 32, (8, 8, 8))]
_cache = {}


def _case(kind, shape):
    """inputs and fp64 reference of one shape, computed once and shared (never modified: every test clones what it changes)"""
    key = (kind, shape)
    if key not in _cache:
        n, cin, cout, dims = shape
        if kind == "ints":
            R.check_exact_range(n, cin, cout, dims, K3)
        t = R.make_inputs(kind, n, cin, cout, dims, K3, dims)
        _cache[key] = (t, R.reference(t, S1, P1, with_abs=(kind == "gauss")))
    return _cache[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[3])))
@pytest.mark.parametrize("kind", ["ints", "gauss"])
def test_fp32_torch_passes(kind, shape):
    """fp32 F.conv3d and its autograd gradients on the same operands: equality for `ints`, far inside the bound for `gauss`."""
    n, cin, cout, dims = shape
    t, ref = _case(kind, shape)
    x = t["x"].float().requires_grad_(True)
    w = R.bf(t["w"]).float().requires_grad_(True)
    y = F.conv3d(x, w, t["bias"].float(), padding=1)
    y.backward(t["dy"].float())
    nt = R.terms(n, cin, cout, dims, K3)
    bnd = R.gauss_bounds(ref, nt) if kind == "gauss" else {}
    ys = R.Slot((n,) + dims + (cout,), "last")
    ys.payload()[:] = R.cl(y.detach()).to(R.BF16)
    dxs = R.Slot((n,) + dims + (cin,), "first")
    dxs.payload()[:] = R.cl(x.grad).to(R.BF16)
    dws = R.SlotF32(t["dw0"].reshape(1, -1))
    dws.payload()[:] += w.grad.reshape(1, -1)
    css = R.SlotF32(t["cs0_img"], pitched=True)
    css.payload()[:] += t["dy"].float().sum(dim=(2, 3, 4))
    got = dict(y=R.compare(kind, ys, R.cl(ref["y1"]), R.cl(bnd["y"]) if bnd else None),
               dx=R.compare(kind, dxs, R.cl(ref["dx"]), R.cl(bnd["dx"]) if bnd else None),
               dw=R.compare(kind, dws, (ref["dw"] + t["dw0"]).float().double() if kind == "gauss" else ref["dw"] + t["dw0"], bnd.get("dw")),
               cs=R.compare(kind, css, (ref["cs_img"] + t["cs0_img"]).float().double() if kind == "gauss" else ref["cs_img"] + t["cs0_img"], bnd.get("cs_img")))
    print(kind, shape, got)
    for q, (worst, fences) in got.items():
        assert fences, q
        assert worst == 0 if kind == "ints" else worst <= 1.0, (q, worst)


def _tile_mask(dims, d0, h0, w0):
    m = torch.zeros(dims, dtype=torch.bool)
    m[d0:d0 + 4, h0:h0 + 8, w0:w0 + 8] = True
    return m


def _dw_defects(t, ref, dims):
    """name -> the weight gradient a kernel with that defect would leave (prefill included), from the exact one"""
    x, dy = t["x"], t["dy"]
    full = ref["dw"] + t["dw0"]
    out = {}
    # one (voxel, tap, channel) product: output voxel v, tap (0, 2, 1) reads x[v + tap - 1]
    co, ci, (d, h, w), (kd, kh, kw) = 5, 9, (dims[0] - 2, 3, 4), (0, 2, 1)
    while x[0, ci, d + kd - 1, h + kh - 1, w + kw - 1] == 0 or dy[0, co, d, h, w] == 0:
        w += 1
    prod = x[0, ci, d + kd - 1, h + kh - 1, w + kw - 1] * dy[0, co, d, h, w]
    for name, sign in (("product dropped", -1.0), ("product doubled", 1.0)):
        g = full.clone()
        g[co, ci, kd, kh, kw] += sign * prod
        out[name] = g
    # the halo row (d0 - 1, h0 - 1) of the tile at (4, 8, 0) shifted by one voxel along w: the taps (0, 0, *) of the tile's first output
    # row read x one voxel further
    d0, h0 = 4, 8 if dims[1] > 8 else 0
    g = full.clone()
    row_dy = dy[0, :, d0, h0, 0:8]                                   # [Cout, 8]
    xp = F.pad(x[0, :, d0 - 1, h0 - 1 if h0 else 0, :], (1, 2))      # [Cin, W + 3]: index w + 1 = voxel w
    for kw in range(3):
        good = xp[:, kw:kw + 8] if h0 else torch.zeros_like(xp[:, kw:kw + 8])   # (h0 = 0: the row above is padding, zeros)
        shifted = xp[:, kw + 1:kw + 9]
        g[:, :, 0, 0, kw] += row_dy @ (shifted - good).T
    out["halo row shifted"] = g
    # the last tile of the last split never accumulated
    m = _tile_mask(dims, (dims[0] - 1) // 4 * 4, (dims[1] - 1) // 8 * 8, (dims[2] - 1) // 8 * 8)
    last = torch.nn.grad.conv3d_weight(x, full.shape, dy * m, padding=1)
    out["last tile skipped"] = full - last
    return full, out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[3])))
def test_defects_are_reported(shape):
    n, cin, cout, dims = shape
    t, ref = _case("ints", shape)
    full, defects = _dw_defects(t, ref, dims)
    for name, g in defects.items():
        slot = R.SlotF32(t["dw0"].reshape(1, -1))
        slot.payload()[:] = g.reshape(1, -1).float()
        worst, fences = R.compare("ints", slot, full)
        moved = float((g - full).abs().max())
        print(f"{dims} ints {name}: {int(worst)} unequal entries, worst moved by {moved:.4g}, old tolerance {1e-2 * float(ref['dw'].abs().max()):.4g}")
        assert worst >= 1 and fences, name
        if dims == (20, 32, 32) and name.startswith("product"):
            assert R.old_measure_passes(g - t["dw0"], ref["dw"]), name   # what the old measure cannot see
    # the exact result itself is clean
    slot = R.SlotF32(t["dw0"].reshape(1, -1))
    slot.payload()[:] = full.reshape(1, -1).float()
    assert R.compare("ints", slot, full) == (0.0, True)

    # bf16 output defects, on y in the last channels of a wider buffer
    y2d = R.cl(ref["y1"])
    def fresh():
        s = R.Slot((n,) + dims + (cout,), "last")
        s.payload()[:] = y2d.to(R.BF16)
        return s
    assert R.compare("ints", fresh(), y2d) == (0.0, True)
    s = fresh()
    s.payload()[s.rows - 1] = math.nan                     # one voxel left unwritten: the poison stays
    assert R.compare("ints", s, y2d) == (math.inf, True)
    s = fresh()
    s.buf[s.rows, s.c0:] = s.buf[s.rows - 1, s.c0:]        # one voxel written past the slot
    assert R.compare("ints", s, y2d) == (0.0, False)
    s = fresh()
    s.buf[3, :s.c0] = 1.0                                  # ... or one row's store starting 32 channels early
    assert R.compare("ints", s, y2d)[1] is False
    s = fresh()
    s.payload()[:] = R.bf_trunc(y2d).to(R.BF16)            # truncation instead of round-to-nearest-even
    worst, fences = R.compare("ints", s, y2d)
    print(f"{dims} truncated output: {int(worst)} of {y2d.numel()} elements differ")
    assert worst >= 1 and fences


def test_old_measure_misses_single_products_with_gaussian_inputs():
    """The same two defects with the Gaussian inputs of the existing tests at 20x32x32: inside 1e-2 * max |dw| (module docstring)."""
    shape = SHAPES[0]
    t, ref = _case("gauss", shape)
    full, defects = _dw_defects(t, ref, shape[3])
    tol = 1e-2 * float(ref["dw"].abs().max())
    for name in ("product dropped", "product doubled"):
        moved = float((defects[name] - full).abs().max())
        print(f"gauss {name}: moved {moved:.4g}, old tolerance {tol:.4g}")
        assert moved > 0 and R.old_measure_passes(defects[name] - t["dw0"], ref["dw"])
    for name in ("halo row shifted", "last tile skipped"):
        print(f"gauss {name}: moved {float((defects[name] - full).abs().max()):.4g}, old tolerance {tol:.4g}")


def test_kernel_ids_match_the_header():
    """The names the GPU tests use are read from include/medimgen_hip.h (conv_ref.kernel_ids), so they cannot drift from the library."""
    ids = R.kernel_ids()
    assert ids["MI_CK_NONE"] == 0 and ids["MI_CK_COUNT"] == len(ids) - 1 and sorted(ids.values()) == list(range(len(ids)))
