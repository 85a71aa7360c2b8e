"""The five kernels of csrc/perceptual.hip, called through the C ABI and held per element to the fp64 closed forms of
tests/perc_ref.py (tests/test_perc_ref_cpu.py checks those forms, the bounds and the planted faults without a GPU).  Buffers are
poisoned and fenced where a kernel must not read or write: NaN in the channels of a stride beyond C, sentinel guard slices / volumes /
rows around every output.  No element is left out of a comparison.

Shapes -- the smallest at which each path exists:
  mi_perc_gather        (2,5,6,7), C = 1 and 3, the three axes, channel stride C + 2 with NaN extra channels (they must not reach the
                        output); indices -1, N * L, a repeat, an unsorted tail: bad indices give exactly zero slices, channels 3..7
                        are exactly zero.  Loop: axis 0 of (1,83,160,160), every slice in shuffled order = 2 124 800 pixels, more than
                        the 2 097 152 threads of the capped grid (grid_for), so the grid-stride loop makes a second trip.
  mi_perc_scatter_add   the same two cases with unique valid indices (a plain read-modify-write), a non-zero starting dx, stride C + 2,
                        the bad indices: every voxel of a slice not selected, every extra channel and the guard volumes bit-unchanged.
  mi_relu_maxpool2_*    odd W and odd H together (3,7,9,16); H = 1 and W = 1 (no pooling window: `pooled` empty, rectify only, through
                        both kernels); the in-place backward with a pooled gradient (dx == dadd, dpooled != NULL), the form
                        PerceptualLoss._axis issues on every level; loop: (8,130,130,512) = 2 163 200 threads.  Forward and pooled
                        output bit-equal; backward bit-equal on integer gradients, one bf16 rounding (2^-8 |want|) on Gaussian ones.
                        (The tie test stays in test_perceptual_gpu.py.)
  mi_lpips_head         C = 64, 128, 256, 512 at the existing small shape (3 x 37) and at 4096 * 256 / (C / 8) + 37 pixels, one pixel
                        group past a full pass of the head's capped grid (about 16 MB per tensor); a zero f0 pixel (in both trips), a
                        zero f1 pixel, a loss that already holds a value; loss alone and df0 alone; C = 96 refused, nothing written.
Bounds (perc_ref): gather 2^-8 |want| + 2^-22 (|v| + |shift|) / scale; scatter 2^-8 |want| + 2^-22 (|dx_old| + sum_c |g_c| / scale_c);
head df0 2^-8 |want| + 2^-18 (|g_c| / r0 + |u_c| |t|); loss 1e-4 relative.

Measured on the MI355X (table in EXPERIMENTS.md), worst err / bound per kernel: gather 0.987, scatter-add 0.996, head df0 0.995 (bf16
outputs: the bound's first term is the output rounding itself, so a correct kernel sits just under 1), head loss 3.9e-6 relative
against 1e-4; pool forward, pooled output and integer-gradient backward bit-equal at every shape, Gaussian-gradient backward 0.996 of
one rounding; no guard, extra channel or unselected voxel changed.  No kernel fault found.  Slowest test:
test_relu_maxpool_fwd_bwd_bit_equal[8x130x130x512], 1.1 s; the other loop cases 0.2 to 0.6 s.
"""
import time

import pytest
import torch

from tests import perc_ref as R

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
GUARD = -77.0   # a value a rectifier would change and an accumulation would move


def _lib():
    from medical_image_generation_amd import _lib
    return _lib


def _scaling():
    from medical_image_generation_amd.perceptual import _SCALE, _SHIFT
    return torch.tensor(_SHIFT, dtype=F32), torch.tensor(_SCALE, dtype=F32)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _fenced(payload_shape, dtype=BF16, fill=GUARD):
    """A device buffer with one guard entry of the leading axis on either side: (whole, payload view)."""
    whole = torch.full((payload_shape[0] + 2,) + tuple(payload_shape[1:]), fill, dtype=dtype, device="cuda")
    return whole, whole[1:-1]


def _guards_intact(whole, fill=GUARD):
    w = whole.cpu()
    return bool((w[0] == fill).all()) and bool((w[-1] == fill).all())


GATHER_CASES = [(R.EDGE_VOLUME, c, axis, False) for c in (1, 3) for axis in range(3)] + [(R.LOOP_VOLUME, 1, 0, True)]

def _id(case):
    shape, c, axis, loop = case
    return f"{'loop' if loop else 'edge'}-C{c}-axis{axis}"


@pytest.mark.parametrize("case", GATHER_CASES, ids=_id)
def test_gather_per_element(case):
    L = _lib()
    shape, c, axis, loop = case
    n, d, h, w = shape
    shift, scale = _scaling()
    idx = R.loop_indices() if loop else R.edge_indices(R.extent(shape, axis))
    a, b = R.pixel_axes(shape, axis)
    S = idx.numel()
    if loop:
        assert S * a * b > R.GRID_THREADS, "this case exists for the second trip of the grid-stride loop"
    x = R.volume(shape, c, 10 + axis)
    want, bound = R.gather(x, c, axis, idx, shift, scale)
    whole, out = _fenced((S, a, b, 8))
    xd, idxd, shd, scd = x.cuda(), idx.cuda(), shift.cuda(), scale.cuda()
    t0 = time.time()
    L.call("mi_perc_gather", xd.data_ptr(), c + 2, c, n, d, h, w, axis, idxd.data_ptr(), S, shd.data_ptr(), scd.data_ptr(), out.data_ptr())
    got = out.cpu().double()
    assert _guards_intact(whole), "a guard slice changed"
    ok = (idx >= 0) & (idx < R.extent(shape, axis))
    assert not bool(got[..., 3:].any()), "channels 3..7 must be exactly zero"
    assert not bool(got[~ok].any()), "an index outside the axis must give an exactly zero slice"
    r = R.ratio(got, want, bound)
    print(f"PERC gather {_id(case)}: {S * a * b} pixels, err / bound {r:.3f}, {time.time() - t0:.2f} s")
    assert r <= 1.0


@pytest.mark.parametrize("case", GATHER_CASES, ids=_id)
def test_scatter_add_per_element(case):
    L = _lib()
    shape, c, axis, loop = case
    n, d, h, w = shape
    _, scale = _scaling()
    idx = R.loop_indices() if loop else R.edge_indices(R.extent(shape, axis), unique=True)
    a, b = R.pixel_axes(shape, axis)
    S = idx.numel()
    dx0 = R.volume(shape, c, 20 + axis)
    ds = R.slice_grads(S, a, b, 30 + axis)
    want, bound, touched = R.scatter_add(dx0, ds, c, axis, idx, scale)
    whole, dx = _fenced((1,) + tuple(dx0.shape))   # a guard volume on either side
    dx[0].copy_(dx0)
    dsd, idxd, scd = ds.cuda(), idx.cuda(), scale.cuda()
    L.call("mi_perc_scatter_add", dsd.data_ptr(), axis, idxd.data_ptr(), S, n, d, h, w, c, scd.data_ptr(), dx.data_ptr(), c + 2)
    got = dx[0].cpu()
    assert _guards_intact(whole), "a guard volume changed"
    assert torch.equal(_bits(got[..., c:]), _bits(dx0[..., c:])), "a channel of the stride beyond C changed"
    assert torch.equal(_bits(got[..., :c][~touched]), _bits(dx0[..., :c][~touched])), "a voxel of a slice that was not selected changed"
    r = R.ratio(got[..., :c][touched].double(), want[touched], bound[touched])
    print(f"PERC scatter {_id(case)}: {int(touched.sum())} voxels touched, err / bound {r:.3f}")
    assert r <= 1.0


POOL_SHAPES = [(3, 7, 9, 16), (2, 1, 9, 16), (2, 7, 1, 16), (8, 130, 130, 512)]


def _pool_inputs(shape, ints):
    g = torch.Generator().manual_seed(sum(shape))
    n, h, w, c = shape
    z = torch.randint(-2, 3, shape, generator=g, dtype=torch.int8).to(BF16)   # small integers: ties inside most windows, many zeros
    mk = (lambda s: torch.randint(-3, 4, s, generator=g, dtype=torch.int8).to(BF16)) if ints else (lambda s: torch.randn(s, generator=g).to(BF16))
    return z, mk((n, h // 2, w // 2, c)), mk(shape)


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_relu_maxpool_fwd_bwd_bit_equal(shape):
    L = _lib()
    n, h, w, c = shape
    big = n * h * w * c > 1 << 24
    if big:
        assert n * ((h + 1) // 2) * ((w + 1) // 2) * (c // 8) > R.GRID_THREADS, "this case exists for the second trip of the grid-stride loop"
    t0 = time.time()
    z, dp, dadd = _pool_inputs(shape, ints=True)
    a_want, p_want = R.relu_pool_fwd(z)
    # ---- forward: rectify in place, pool into a fenced buffer (an empty `pooled` still takes the pooling kernel: a non-NULL pointer)
    xw, x = _fenced(shape)
    x.copy_(z)
    pw, p = _fenced((n, max(h // 2, 1), max(w // 2, 1), c))
    L.call("mi_relu_maxpool2_fwd", x.data_ptr(), p.data_ptr(), n, h, w, c)
    assert _guards_intact(xw) and _guards_intact(pw), "a guard row changed"
    assert torch.equal(_bits(x.cpu()), _bits(a_want)), "the rectified activation is not bit-equal"
    if p_want.numel():
        assert torch.equal(_bits(p.cpu()), _bits(p_want)), "the pooled output is not bit-equal"
    else:
        assert bool((p.cpu() == GUARD).all()), "there is no pooling window at this shape: nothing may be written"
        x2w, x2 = _fenced(shape)   # and the rectifier alone (pooled NULL)
        x2.copy_(z)
        L.call("mi_relu_maxpool2_fwd", x2.data_ptr(), None, n, h, w, c)
        assert _guards_intact(x2w) and torch.equal(_bits(x2.cpu()), _bits(a_want))
    # ---- backward in place (dx == dadd) with a pooled gradient, as PerceptualLoss._axis issues it; integer gradients: exact
    want = R.relu_pool_bwd(a_want, dp, dadd, dtype=F32)
    gw, g = _fenced(shape)
    g.copy_(dadd)
    dpw, dpd = _fenced((n, max(h // 2, 1), max(w // 2, 1), c))
    if dp.numel():
        dpd.copy_(dp)
    L.call("mi_relu_maxpool2_bwd", x.data_ptr(), dpd.data_ptr(), g.data_ptr(), g.data_ptr(), n, h, w, c)
    assert _guards_intact(gw) and _guards_intact(dpw) and _guards_intact(xw)
    got = g.cpu()
    assert torch.equal(_bits(got), _bits(want.to(BF16))) and torch.equal(got.float(), want), "the in-place backward is not bit-equal"
    del want, got
    if not big:
        # out of place, pooled gradient alone (dadd NULL) and both, Gaussian gradients: one bf16 rounding of the exact sum
        _, dpg, daddg = _pool_inputs(shape, ints=False)
        for use_dadd in (True, False):
            want64 = R.relu_pool_bwd(a_want, dpg, daddg if use_dadd else None)
            ow, o = _fenced(shape)
            dd = daddg.cuda() if use_dadd else None
            if dpg.numel():
                dpd.copy_(dpg)
            elif not use_dadd:
                continue   # (neither gradient: the entry point refuses)
            L.call("mi_relu_maxpool2_bwd", x.data_ptr(), dpd.data_ptr(), None if dd is None else dd.data_ptr(), o.data_ptr(), n, h, w, c)
            assert _guards_intact(ow)
            r = R.ratio(o.cpu().double(), want64, R.U8 * want64.abs())
            print(f"PERC pool bwd {shape} dadd={use_dadd}: err / bound {r:.3f}")
            assert r <= 1.0
    print(f"PERC pool {shape}: {time.time() - t0:.2f} s")


HEAD_CASES = [(c, loop) for c in R.HEAD_CHANNELS for loop in (False, True)]


@pytest.mark.parametrize("c,loop", HEAD_CASES, ids=lambda v: None)
def test_lpips_head_per_element(c, loop):
    L = _lib()
    npix = R.head_pixels(c, loop)
    s, p = (1, npix) if loop else R.HEAD_SMALL
    if loop:
        assert npix * (c // 8) > R.HEAD_GROUPS, "this case exists for the second trip of the head's loop"
    weight, start = 0.7, 0.03125
    t0 = time.time()
    f0, f1, w = R.head_inputs(npix, c, c)
    loss_want, df_want, bound = R.head(f0, f1, w, weight)
    f0d, f1d, wd = f0.cuda(), f1.cuda(), w.cuda()
    loss = torch.tensor([start, GUARD], device="cuda")
    dfw, df = _fenced((npix, c))
    L.call("mi_lpips_head", f0d.data_ptr(), f1d.data_ptr(), wd.data_ptr(), s, p, c, weight, 1e-10, loss.data_ptr(), df.data_ptr())
    got = df.cpu()
    assert _guards_intact(dfw) and float(loss[1]) == GUARD
    rel = abs(float(loss[0]) - start - loss_want) / abs(loss_want)
    r = R.ratio(got.double(), df_want, bound)
    print(f"PERC head C={c} npix={npix}: df0 err / bound {r:.3f}, loss rel {rel:.2e}, {time.time() - t0:.2f} s")
    assert r <= 1.0
    assert rel <= 1e-4
    # loss alone and df0 alone: the same values
    loss1 = torch.tensor([start, GUARD], device="cuda")
    L.call("mi_lpips_head", f0d.data_ptr(), f1d.data_ptr(), wd.data_ptr(), s, p, c, weight, 1e-10, loss1.data_ptr(), None)
    assert abs(float(loss1[0]) - start - loss_want) <= 1e-4 * abs(loss_want) and float(loss1[1]) == GUARD
    df1w, df1 = _fenced((npix, c))
    L.call("mi_lpips_head", f0d.data_ptr(), f1d.data_ptr(), wd.data_ptr(), s, p, c, weight, 1e-10, None, df1.data_ptr())
    assert _guards_intact(df1w) and torch.equal(_bits(df1.cpu()), _bits(got)), "df0 alone differs from df0 with the loss"


def test_lpips_head_refuses_other_channel_counts():
    L = _lib()
    npix, c = 37, 96
    f0, f1, w = R.head_inputs(npix, c, c)
    f0d, f1d, wd = f0.cuda(), f1.cuda(), w.cuda()
    loss = torch.tensor([0.25], device="cuda")
    dfw, df = _fenced((npix, c))
    with pytest.raises(L.HipError, match="MI_ERR_UNSUPPORTED"):
        L.call("mi_lpips_head", f0d.data_ptr(), f1d.data_ptr(), wd.data_ptr(), 1, npix, c, 0.7, 1e-10, loss.data_ptr(), df.data_ptr())
    torch.cuda.synchronize()
    assert float(loss) == 0.25 and bool((dfw.cpu() == GUARD).all()), "a refused call wrote"
