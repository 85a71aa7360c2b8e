"""Sliding-window inference on the GPU (csrc/sliding.hip, medical_image_generation_amd/sliding.py) against the fp64 restatement
tests/sliding_ref.py: the three kernels per element, the inferer around a synthetic network whose windows disagree on shared voxels,
the real AutoencoderKL, graph replay, the tiled decode of the latent inferer, bad arguments.

The per-element bound of every blended value is (2 K + 4) * 2^-24 * (sum_k w_k |p_k|) / (sum_k w_k), K = windows over the voxel: one
rounding per product and per add in the numerator, one per add in the denominator, and the division."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases, synth
from tests import sliding_ref as R

pytestmark = pytest.mark.gpu
S = cases.SEED
I32 = torch.int32

# rows 1-3 of the planning table: image, roi, overlap
BLEND_CASES = {"plain": ((13, 18, 23), (8, 8, 16), 0.25), "padded": ((5, 18, 23), (8, 8, 16), 0.5), "aligned": ((16, 24, 32), (8, 16, 16), 0.5)}


def _table(head, rows):
    t = torch.tensor([list(head)] + [list(r) for r in rows], dtype=I32)
    return t.cuda(), t


def _gather(image, rows, roi, mode, cval=0.0, host=True):
    from medical_image_generation_amd._lib import call, ptr
    dev, hostt = _table((image.shape[0],) + tuple(image.shape[2:]), rows)
    tiles = torch.full((len(rows), image.shape[1]) + tuple(roi), float("nan"), device="cuda")
    call("mi_sw_gather", ptr(image), image.numel(), image.shape[1], ptr(dev), hostt.data_ptr() if host else None, len(rows), *roi,
         {"constant": 0, "reflect": 1, "replicate": 2}[mode], cval, ptr(tiles))
    return tiles


# ------------------------------------------------------------------------------------------------------------------ 1. gather
@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate"])
@pytest.mark.parametrize("channels,shape,roi", [(1, (6, 9, 16), (4, 5, 8)), (3, (6, 9, 23), (4, 5, 7)), (1, (6, 9, 23), (4, 5, 8)),
                                                (3, (5, 7, 16), (4, 4, 16)), (1, (1, 9, 16), (1, 4, 8)), (3, (1, 10, 23), (1, 6, 23))])
def test_gather_is_bit_equal_to_the_restatement(mode, channels, shape, roi):
    """Windows touching every face, negative origins, origins that are and are not multiples of four voxels (both access paths; W
    16 and 23), a filler row, C = 1 and 3, 2-D as D = 1."""
    image = synth.tensor(S, f"sw_gather_{channels}_{shape}", (2, channels) + shape)
    d, h, w = shape
    rd, rh, rw = roi
    rows = [(0, 0, 0, 0), (1, d - rd, h - rh, w - rw),                          # the two corners, inside
            (0, -min(2, d - 1), -3, -4), (1, d - rd + min(2, d - 1), h - rh + 3, w - rw + 4),  # over every face, x origin a multiple of 4
            (-1, 0, 0, 0),                                                      # filler
            (1, 0, 1, -3), (0, d - rd, -2, w - rw + 1), (1, 0, 2, (w - rw) // 2)]    # odd x origins
    got = _gather(image.cuda(), rows, roi, mode, cval=-1.5)
    want = R.gather_ref(image, rows, roi, mode, -1.5)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got[4].cpu(), torch.zeros_like(want[4]))
    assert torch.equal(_gather(image.cuda(), rows, roi, mode, cval=-1.5, host=False).cpu(), want)  # without the host copy of the table


# ------------------------------------------------------------------------------------------------- 2. accumulate + finish
@functools.lru_cache(maxsize=None)
def _blend_case(name):
    """fp32 pred / imp shared by every batch size of one case, and the fp64 blend of them."""
    from medical_image_generation_amd.sliding import WindowPlan, importance_map
    image, roi, overlap = BLEND_CASES[name]
    n, co = 2, 2
    plan = WindowPlan(image, roi, overlap)
    pads, _, windows = R.window_starts(image, roi, overlap)
    assert plan.windows == windows
    preds = synth.tensor(S, "sw_pred_" + name, (n * len(windows), co) + roi)
    imp = torch.from_numpy(importance_map(roi, "gaussian", 0.125).astype(np.float32))
    assert torch.equal(imp, R.importance(roi, "gaussian", 0.125).float())
    padded = tuple(s + b + a for s, (b, a) in zip(image, pads))
    want, bound = R.blend(list(preds), imp, windows, n, co, padded, [p[0] for p in pads], image)
    return plan, preds, imp, padded, want, bound


def _blend_on_gpu(name, batch):
    from medical_image_generation_amd._lib import call, ptr
    plan, preds, imp, padded, _, _ = _blend_case(name)
    n, co = 2, 2
    rows = plan.rows(n, batch)
    nw = plan.num_windows
    acc = torch.zeros((n, co) + padded, device="cuda")
    wsum = torch.zeros(padded, device="cuda")
    imp_d = imp.cuda()
    for call_rows in rows:
        pred = torch.full((batch, co) + plan.roi, float("nan"), device="cuda")  # fillers carry NaN: they must not be read into acc
        for b, r in enumerate(call_rows):
            if r[0] >= 0:
                pred[b] = preds[int(r[0]) * nw + plan.windows.index(tuple(int(v) for v in r[1:]))].cuda()
        dev, host = _table((n,) + padded, call_rows.tolist())
        call("mi_sw_accumulate", ptr(pred), ptr(imp_d), ptr(dev), host.data_ptr(), batch, co, *plan.roi, ptr(acc), ptr(wsum), acc.numel())
    out = torch.empty((n, co) + plan.image, device="cuda")
    call("mi_sw_finish", ptr(acc), ptr(wsum), ptr(out), n, co, *padded, *plan.pad_before, *plan.image)
    return out.cpu()


@pytest.mark.parametrize("name", list(BLEND_CASES))
def test_accumulate_and_finish_per_element(name):
    plan, _, _, _, want, bound = _blend_case(name)
    outs = {b: _blend_on_gpu(name, b) for b in (1, 3, 5)}
    assert (plan.num_windows * 2) % 5 != 0  # batch 5 ends in filler rows for 24, 16 and 36 windows
    err = (outs[1].double() - want).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"\n[{name}] max |err| {float(err.max()):.3e}, max err / bound {worst:.3f}, windows {plan.num_windows}")
    assert bool((err <= bound).all())
    for b in (3, 5):
        assert torch.equal(outs[b], outs[1]), b  # the sum is in enumeration order whatever the batch size
    assert torch.equal(_blend_on_gpu(name, 3), outs[3])  # and from run to run


# ------------------------------------------------------------------------------------------------- 3. synthetic network
class _Synthetic:
    """p = tile * R + S with dyadic tiles and small-integer-over-power-of-two R, S: every product and sum is exact in fp32, on both
    sides; R and S vary over the window, so two windows disagree on the voxels they share and the seams matter.  pooled=True also
    returns avg_pool3d(p, 4): a second member of another extent."""

    def __init__(self, roi, pooled=False):
        g = torch.Generator().manual_seed(S)
        self.r = torch.randint(-8, 9, roi, generator=g).float() / 8
        self.s = torch.randint(-8, 9, roi, generator=g).float() / 4
        self.pooled = pooled

    def __call__(self, t):
        p = t * self.r.to(t.device) + self.s.to(t.device)
        return (p, F.avg_pool3d(p, 4)) if self.pooled else p


def _dyadic(name, shape):
    return torch.randint(-32, 33, shape, generator=torch.Generator().manual_seed(S + len(name))).float() / 16


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
@pytest.mark.parametrize("name", ["plain", "padded"])
def test_inferer_with_a_synthetic_network(name, mode):
    from medical_image_generation_amd.sliding import SlidingWindowInferer, sliding_window_inference
    image, roi, overlap = BLEND_CASES[name]
    x = _dyadic(name, (2, 3) + image)
    net = _Synthetic(roi)
    (want, bound), = R.infer(x, net, roi, overlap, mode, padding_mode="reflect")
    outs = {b: SlidingWindowInferer(roi, b, overlap, mode, padding_mode="reflect")(x.cuda(), net).cpu() for b in (1, 5)}
    assert outs[1].shape == x.shape
    err = (outs[1].double() - want).abs()
    print(f"\n[{name} {mode}] max |err| {float(err.max()):.3e}, max err / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(outs[5], outs[1])
    assert torch.equal(sliding_window_inference(x.cuda(), roi, 5, net, overlap, mode, padding_mode="reflect").cpu(), outs[1])


def test_inferer_blends_a_tuple_output_per_member():
    from medical_image_generation_amd.sliding import SlidingWindowInferer
    image, roi, overlap = BLEND_CASES["aligned"]  # starts and extents are multiples of 4: the pooled member maps to whole voxels
    x = _dyadic("tuple", (2, 1) + image)
    net = _Synthetic(roi, pooled=True)
    ref = R.infer(x, net, roi, overlap, "gaussian")
    got = SlidingWindowInferer(roi, 5, overlap, "gaussian")(x.cuda(), net)
    assert isinstance(got, tuple) and len(got) == 2
    assert got[0].shape == x.shape and got[1].shape == (2, 1) + tuple(s // 4 for s in image)
    for g, (want, bound) in zip(got, ref):
        err = (g.cpu().double() - want).abs()
        assert bool((err <= bound).all())
    with pytest.raises(ValueError, match="whole output voxel"):  # row 1: start 5, extent 13 have no quarter
        SlidingWindowInferer((8, 8, 16), 2, 0.25)(_dyadic("odd", (1, 1, 13, 18, 23)).cuda(), _Synthetic((8, 8, 16), pooled=True))


def test_inferer_runs_2d():
    from medical_image_generation_amd.sliding import SlidingWindowInferer
    x = _dyadic("2d", (2, 2, 18, 23))
    g = torch.Generator().manual_seed(S)
    r, s = torch.randint(-8, 9, (8, 16), generator=g).float() / 8, torch.randint(-8, 9, (8, 16), generator=g).float() / 4
    net = lambda t: t * r.to(t.device) + s.to(t.device)  # noqa: E731
    (want, bound), = R.infer(x, net, (8, 16), 0.25, "gaussian")
    got = SlidingWindowInferer((8, 16), 3, 0.25, "gaussian")(x.cuda(), net).cpu()
    assert got.shape == x.shape and bool(((got.double() - want).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------- 4./5. the real autoencoder
AE_IMAGE = (1, 1, 24, 16, 32)


@functools.lru_cache(maxsize=None)
def _ae():
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    ae = AutoencoderKL(**cases.AEKL_CASES["aekl_c3a"]["kwargs"])
    ae.load_state_dict(synth.state_dict({k: tuple(v.shape) for k, v in ae.state_dict().items()}, S))
    return ae.cuda().eval()


@functools.lru_cache(maxsize=None)
def _ae_reference():
    """The restatement fed by the same model, called per window on torch-sliced windows: shared by the eager and the graph test."""
    ae = _ae()
    x = synth.ellipsoid_volume(S, "sw_case", AE_IMAGE)

    def on_gpu(fn):
        def run(t):
            with torch.no_grad():
                out = fn(t.cuda().contiguous())
            return tuple(o.cpu() for o in out) if isinstance(out, tuple) else out.cpu()
        return run

    with torch.no_grad():
        z = ae.encode(x.cuda())[0].cpu()
    return {"x": x, "z": z,
            "reconstruct": R.infer(x, on_gpu(ae.reconstruct), (16, 16, 16), 0.5),
            "encode": R.infer(x, on_gpu(ae.encode), (16, 16, 16), 0.5),
            "decode": R.infer(z, on_gpu(ae.decode), (4, 4, 4), 0.5)}


def _check_members(got, ref, what):
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(ref)
    for g, (want, bound) in zip(got, ref):
        err = (g.cpu().double() - want).abs()
        print(f"\n[{what}] max |err| {float(err.max()):.3e}, max err / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
        assert g.shape == want.shape and bool((err <= bound).all()), what


def test_tiled_reconstruct_with_one_window_is_the_plain_reconstruct():
    from medical_image_generation_amd.sliding import SlidingWindowInferer, tiled_reconstruct
    ae, x = _ae(), synth.ellipsoid_volume(S, "sw_case", AE_IMAGE).cuda()
    with torch.no_grad():
        want = ae.reconstruct(x)
    got = tiled_reconstruct(ae, x, SlidingWindowInferer(AE_IMAGE[2:], 1, 0.25, "constant"))
    assert torch.equal(got, want)


@pytest.mark.parametrize("use_graph", [False, True])
def test_tiled_autoencoder_matches_the_restatement(use_graph):
    """roi 16^3, overlap 0.5 on (24, 16, 32): 6 windows.  Against the restatement one window per call, as the restatement calls the
    model, so both sides blend the same predictions and the tolerance is the blend's alone.  The captured mode is bit-equal to eager
    (also at batch 4, which ends in filler rows), and a second case of another extent goes through the same graph."""
    from medical_image_generation_amd.sliding import SlidingWindowInferer, WindowPlan, tiled_decode, tiled_encode, tiled_reconstruct
    assert WindowPlan(AE_IMAGE[2:], 16, 0.5).num_windows == 6
    ae, ref = _ae(), _ae_reference()
    x, z = ref["x"].cuda(), ref["z"].cuda()
    img = SlidingWindowInferer(16, 1, 0.5, use_graph=use_graph)
    lat = SlidingWindowInferer(4, 1, 0.5, use_graph=use_graph)
    got = {"reconstruct": tiled_reconstruct(ae, x, img), "encode": tiled_encode(ae, x, img), "decode": tiled_decode(ae, z, lat)}
    for what in got:
        _check_members(got[what], ref[what], f"{what} graph={use_graph}")
    if not use_graph:
        return
    eager_img, eager_lat = SlidingWindowInferer(16, 1, 0.5), SlidingWindowInferer(4, 1, 0.5)
    assert torch.equal(got["reconstruct"], tiled_reconstruct(ae, x, eager_img))
    for g, e in zip(got["encode"], tiled_encode(ae, x, eager_img)):
        assert torch.equal(g, e)
    assert torch.equal(got["decode"], tiled_decode(ae, z, eager_lat))
    # one graph per (network, channels): reconstruct and encode on `img`; each captured once
    assert len(img._graphs) == 2 and [c.captures for c in img._graphs.values()] == [1, 1]
    x2 = synth.ellipsoid_volume(S, "sw_case2", (1, 1, 16, 24, 24)).cuda()  # another extent, 4 windows
    out2 = tiled_reconstruct(ae, x2, img)
    assert len(img._graphs) == 2 and [c.captures for c in img._graphs.values()] == [1, 1]  # no new capture
    assert torch.equal(out2, tiled_reconstruct(ae, x2, eager_img))
    assert torch.equal(tiled_reconstruct(ae, x, img), got["reconstruct"])  # and back to the first extent
    x3 = synth.ellipsoid_volume(S, "sw_case3", (1, 1, 32, 16, 32)).cuda()  # more voxels than any case before: larger buffers, one more capture
    assert torch.equal(tiled_reconstruct(ae, x3, img), tiled_reconstruct(ae, x3, eager_img))
    assert [c.captures for c in img._graphs.values()] == [2, 1]
    assert torch.equal(tiled_reconstruct(ae, x, img), got["reconstruct"]) and [c.captures for c in img._graphs.values()] == [2, 1]
    img4 = SlidingWindowInferer(16, 4, 0.5, "gaussian", use_graph=True)
    assert torch.equal(tiled_reconstruct(ae, x, img4), tiled_reconstruct(ae, x, SlidingWindowInferer(16, 4, 0.5, "gaussian")))


# ------------------------------------------------------------------------------------------------- 6. latent inferer
def test_latent_inferer_decodes_tiled():
    from medical_image_generation_amd.inferer import DDPMScheduler, DiffusionInferer, LatentDiffusionInferer
    from medical_image_generation_amd.sliding import SlidingWindowInferer, tiled_decode
    from medical_image_generation_amd.unet import DiffusionModelUNet
    ae = _ae()
    kw = dict(spatial_dims=3, in_channels=8, out_channels=8, num_res_blocks=1, num_channels=(32, 64), attention_levels=(False, True),
              num_head_channels=(0, 32), norm_num_groups=16, strides=[[1] * 3, [2] * 3], kernel_sizes=[[3] * 3] * 2, paddings=[[1] * 3] * 2)
    net = DiffusionModelUNet(**kw)
    net.load_state_dict(synth.state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, S))
    net = net.cuda().eval()
    sch = DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205)
    sch.set_timesteps(3)
    shape = (1, 8, 8, 8, 8)
    z = synth.tensor(S, "sw_latent_noise", shape).cuda()
    zs = [synth.tensor(S, f"sw_latent_z{i}", shape).cuda() for i in range(3)]
    scale = 0.7
    lat = DiffusionInferer(sch).sample(z, net, sch, verbose=False, noises=zs)
    ldi = LatentDiffusionInferer(sch, scale_factor=scale)
    plain = ldi.sample(z, ae, net, sch, verbose=False, noises=zs)
    with torch.no_grad():
        assert torch.equal(plain, ae.decode_stage_2_outputs(lat / scale))  # the path without the keyword
    assert torch.equal(ldi.sample(z, ae, net, sch, verbose=False, noises=zs, decode_inferer=None), plain)
    tiler = SlidingWindowInferer(4, 2, 0.5, "gaussian")
    tiled = ldi.sample(z, ae, net, sch, verbose=False, noises=zs, decode_inferer=tiler)
    assert tiled.shape == plain.shape == (1, 1, 32, 32, 32)
    assert torch.equal(tiled, tiled_decode(ae, lat / scale, SlidingWindowInferer(4, 2, 0.5, "gaussian")))
    assert not torch.equal(tiled, plain)  # 4^3 windows see less context than the whole latent


# ------------------------------------------------------------------------------------------------- 7. bad arguments
def test_bad_arguments_are_refused_and_the_good_call_still_runs():
    from medical_image_generation_amd._lib import HipError, call, ptr
    image = synth.tensor(S, "sw_bad", (2, 1, 6, 9, 16)).cuda()
    roi = (4, 5, 8)
    dev, host = _table((2, 6, 9, 16), [(0, 0, 0, 0), (1, 1, 2, 3)])
    tiles = torch.empty((2, 1) + roi, device="cuda")

    def gather(image_p=ptr(image), elems=image.numel(), c=1, dev_p=ptr(dev), host_t=host, b=2, roi=roi, mode=0, tiles_p=ptr(tiles)):
        call("mi_sw_gather", image_p, elems, c, dev_p, host_t.data_ptr(), b, *roi, mode, 0.0, tiles_p)

    def table(head, rows):
        return _table(head, rows)[1]

    bad_gather = [dict(image_p=None), dict(dev_p=None), dict(tiles_p=None), dict(elems=0), dict(c=0), dict(b=0), dict(roi=(0, 5, 8)),
                  dict(roi=(4, -1, 8)), dict(roi=(4, 5, 0)), dict(mode=3), dict(mode=-1),
                  dict(elems=image.numel() - 1),                                   # the table's tensor is larger than the buffer
                  dict(host_t=table((0, 6, 9, 16), [(0, 0, 0, 0), (0, 0, 0, 0)])),  # non-positive extents in the table
                  dict(host_t=table((2, 6, 0, 16), [(0, 0, 0, 0), (0, 0, 0, 0)])),
                  dict(host_t=table((2, 6, 9, 16), [(2, 0, 0, 0), (0, 0, 0, 0)])),  # a row names image 2 of 2
                  dict(mode=1, host_t=table((2, 6, 9, 16), [(0, -6, 0, 0), (0, 0, 0, 0)])),  # reflect pad = the axis extent
                  dict(mode=1, host_t=table((2, 6, 9, 16), [(0, 0, 0, 0), (0, 0, 0, 24)]))]
    for kw in bad_gather:
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            gather(**kw)
    gather(mode=1, host_t=table((2, 6, 9, 16), [(0, -5, 0, 0), (1, 1, 2, 3)]))  # pad 5 < 6 is fine
    gather()
    assert torch.equal(tiles.cpu(), R.gather_ref(image.cpu(), [(0, 0, 0, 0), (1, 1, 2, 3)], roi, "constant", 0.0))

    t = (4, 5, 8)
    pred, imp = torch.ones((2, 2) + t, device="cuda"), torch.ones(t, device="cuda")
    acc, wsum = torch.zeros((2, 2, 6, 9, 16), device="cuda"), torch.zeros((6, 9, 16), device="cuda")
    good = [(0, 2, 4, 8), (1, 0, 0, 0)]
    adev, ahost = _table((2, 6, 9, 16), good)

    def accumulate(pred_p=ptr(pred), imp_p=ptr(imp), dev_p=ptr(adev), host_t=ahost, b=2, co=2, t=t, acc_p=ptr(acc), wsum_p=ptr(wsum),
                   elems=acc.numel()):
        call("mi_sw_accumulate", pred_p, imp_p, dev_p, host_t.data_ptr(), b, co, *t, acc_p, wsum_p, elems)

    bad_acc = [dict(pred_p=None), dict(imp_p=None), dict(dev_p=None), dict(acc_p=None), dict(wsum_p=None), dict(b=0), dict(co=0),
               dict(t=(0, 5, 8)), dict(t=(4, 0, 8)), dict(t=(4, 5, -8)), dict(elems=0), dict(elems=acc.numel() - 1),
               dict(host_t=table((2, 6, 9, 0), good)), dict(host_t=table((2, 6, 9, 16), [(2, 0, 0, 0), (0, 0, 0, 0)])),
               dict(host_t=table((2, 6, 9, 16), [(0, 3, 4, 8), (1, 0, 0, 0)])),   # windows that leave the accumulator: z, y, x, negative
               dict(host_t=table((2, 6, 9, 16), [(0, 2, 5, 8), (1, 0, 0, 0)])),
               dict(host_t=table((2, 6, 9, 16), [(0, 2, 4, 9), (1, 0, 0, 0)])),
               dict(host_t=table((2, 6, 9, 16), [(0, 2, 4, 8), (1, 0, -1, 0)]))]
    for kw in bad_acc:
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            accumulate(**kw)
    assert float(acc.abs().max()) == 0 and float(wsum.abs().max()) == 0  # nothing was launched
    accumulate()
    want = torch.zeros(2, 2, 6, 9, 16)
    want[0, :, 2:6, 4:9, 8:16] = 1
    want[1, :, 0:4, 0:5, 0:8] = 1
    assert torch.equal(acc.cpu(), want) and torch.equal(wsum.cpu(), want[0, 0])

    out = torch.full((2, 2, 4, 5, 8), float("nan"), device="cuda")
    wsum.fill_(2.0)

    def finish(acc_p=ptr(acc), wsum_p=ptr(wsum), out_p=ptr(out), n=2, co=2, size=(6, 9, 16), pad=(2, 4, 8), final=(4, 5, 8)):
        call("mi_sw_finish", acc_p, wsum_p, out_p, n, co, *size, *pad, *final)

    bad_fin = [dict(acc_p=None), dict(wsum_p=None), dict(out_p=None), dict(n=0), dict(co=0), dict(size=(0, 9, 16)), dict(final=(4, 0, 8)),
               dict(pad=(-1, 4, 8)), dict(pad=(3, 4, 8)), dict(pad=(2, 5, 8)), dict(pad=(2, 4, 9)), dict(final=(4, 5, 9), pad=(2, 4, 8))]
    for kw in bad_fin:
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            finish(**kw)
    finish()
    assert torch.equal(out.cpu(), want[:, :, 2:6, 4:9, 8:16] / 2)
