"""Tiled (sliding-window) diffusion sampling on the GPU (`window_inferer=` of the inferers, csrc/sliding.hip: mi_sw_gather_cl,
mi_sw_accumulate_cl, mi_sw_diffusion_step) against the fp64 restatement tests/tiled_sampling_ref.py: the three kernels per element,
one window against the plain sampler bit for bit, several windows against the same loop on the oracle's U-Net, conditioning, captured
mode, the latent inferer, refusals.

Bounds.  Blend: sliding_ref.blend's (2 K + 4) 2^-24 sum_k w_k |p_k| / sum_k w_k.  Guided blend: every guided p_k = p_u + w (p_c - p_u)
carries at most three fp32 roundings relative to |p_u| + |w| (|p_c| + |p_u|), so twice the blend's bound on those magnitudes
((4 K + 8) >= (2 K + 4) + 3).  Update on general values: 1e-5 max(1, max |want|), the figure of tests/test_inferer_gpu.py.  Loops on
the bf16 U-Net against the fp32 oracle: rel-L2 3e-2, the budget tests/test_inferer_gpu.py gives a 5-step loop."""
import functools

import pytest
import torch

from oracle import cases, nets, step, synth
from tests import ddim_ref
from tests import guidance_ref as G
from tests import sliding_ref as R
from tests import tiled_sampling_ref as T

pytestmark = pytest.mark.gpu
S = cases.SEED
I32 = torch.int32
BF16 = torch.bfloat16
VOLUMES = {"aligned": ((6, 9, 16), (4, 5, 8)), "odd": ((6, 9, 23), (4, 5, 7))}  # W and roi multiples of four / neither: both access paths
BOUND = 3e-2
DDPM_KW = dict(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205)
STEPS = 4


def _table(head, rows):
    t = torch.tensor([list(head)] + [list(r) for r in rows], dtype=I32)
    return t.cuda(), t


def _cl(p):
    """[B, C, d, h, w] -> NDHWC bf16 on the device."""
    return p.permute(0, 2, 3, 4, 1).contiguous().to(BF16).cuda()


# ------------------------------------------------------------------------------------------------------------- 1. gather_cl
@pytest.mark.parametrize("name", list(VOLUMES))
@pytest.mark.parametrize("c,cc", [(1, 0), (3, 0), (1, 2), (3, 2)])
def test_gather_cl_is_bit_equal_to_slice_cat_cast(name, c, cc):
    """Origins that are odd and that are multiples of four voxels, the far corner, a filler row (zeros), with and without the host
    table, plain and guided (rows [B, 2B): the sample again, zero condition channels)."""
    from medical_image_generation_amd._lib import call, ptr
    (d, h, w), roi = VOLUMES[name]
    rd, rh, rw = roi
    x = synth.tensor(S, f"ts_x_{name}_{c}", (2, c, d, h, w))
    cond = synth.tensor(S, f"ts_cond_{name}_{cc}", (2, cc, d, h, w)) if cc else None
    rows = [(0, 0, 0, 0), (1, d - rd, h - rh, w - rw), (-1, 0, 0, 0), (1, 1, 3, 1), (0, 2, 4, 4), (0, 1, 2, 5), (1, 0, 1, 8)]
    b = len(rows)
    want = torch.zeros((2 * b, rd, rh, rw, c + cc), dtype=BF16)
    for i, (n, z0, y0, x0) in enumerate(rows):
        if n < 0:
            continue
        sl = (n, slice(None), slice(z0, z0 + rd), slice(y0, y0 + rh), slice(x0, x0 + rw))
        tile = x[sl] if cond is None else torch.cat([x[sl], cond[sl]])
        want[i] = tile.to(BF16).permute(1, 2, 3, 0)
        want[b + i, ..., :c] = want[i, ..., :c]
    xd, cd = x.cuda(), None if cond is None else cond.cuda()
    dev, host = _table((2, d, h, w), rows)
    for guided in (0, 1):
        for use_host in (True, False):
            out = torch.full(((2 if guided else 1) * b, rd, rh, rw, c + cc), float("nan"), dtype=BF16, device="cuda")
            call("mi_sw_gather_cl", ptr(xd), xd.numel(), c, ptr(cd), cd.numel() if cc else 0, cc, ptr(dev), host.data_ptr() if use_host else None,
                 b, guided, rd, rh, rw, ptr(out))
            assert torch.equal(out.cpu().view(torch.int16), want[:out.shape[0]].view(torch.int16)), (guided, use_host)


# --------------------------------------------------------------------------------------------------------- 2. accumulate_cl
@functools.lru_cache(maxsize=None)
def _blend_case(name, co):
    """The bf16 predictions (condition and null branch) of every window of two images, the gaussian map, and the fp64 blends: plain
    and guided at w = 2.5 with their bounds."""
    from medical_image_generation_amd.sliding import WindowPlan, importance_map
    volume, roi = VOLUMES[name]
    plan = WindowPlan(volume, roi, 0.5)
    assert plan.padded == volume and (2 * plan.num_windows) % 5 != 0  # batch 5 ends in filler rows
    nflat = 2 * plan.num_windows
    pc = synth.tensor(S, f"ts_pc_{name}_{co}", (nflat, co) + roi).to(BF16)
    pu = synth.tensor(S, f"ts_pu_{name}_{co}", (nflat, co) + roi).to(BF16)
    imp = torch.from_numpy(importance_map(roi, "gaussian", 0.125)).float()
    assert torch.equal(imp, R.importance(roi, "gaussian", 0.125).float())
    zero = (0,) * 3
    plain = R.blend(list(pc.float()), imp, plan.windows, 2, co, volume, zero, volume)
    w = 2.5
    guided, _ = R.blend(list(G.combine(pc.float(), pu.float(), w)), imp, plan.windows, 2, co, volume, zero, volume)
    mag = pu.float().abs().double() + w * (pc.float().abs().double() + pu.float().abs().double())
    _, gbound = R.blend(list(mag), imp, plan.windows, 2, co, volume, zero, volume)
    return plan, pc, pu, imp, plain, (guided, 2 * gbound), w


def _accumulate(name, co, batch, guided=False, use_host=True, want_wsum=True):
    """acc and wsum after every window batch of the case went through mi_sw_accumulate_cl; fillers carry NaN predictions."""
    from medical_image_generation_amd._lib import call, ptr
    plan, pc, pu, imp, _, _, w = _blend_case(name, co)
    volume, roi = VOLUMES[name]
    acc = torch.zeros((2, co) + volume, device="cuda")
    wsum = torch.zeros(volume, device="cuda")
    imp_d, wd = imp.cuda(), torch.tensor([w], device="cuda")
    nw = plan.num_windows
    for call_rows in plan.rows(2, batch):
        pred = torch.full(((2 if guided else 1) * batch,) + roi + (co,), float("nan"), dtype=BF16, device="cuda")
        for b, r in enumerate(call_rows):
            if r[0] >= 0:
                f = int(r[0]) * nw + plan.windows.index(tuple(int(v) for v in r[1:]))
                pred[b] = _cl(pc[f:f + 1])[0]
                if guided:
                    pred[batch + b] = _cl(pu[f:f + 1])[0]
        dev, host = _table((2,) + volume, call_rows.tolist())
        call("mi_sw_accumulate_cl", ptr(pred), ptr(wd) if guided else None, ptr(imp_d), ptr(dev), host.data_ptr() if use_host else None, batch, co,
             *roi, ptr(acc), ptr(wsum) if want_wsum else None, acc.numel())
    return acc.cpu(), wsum.cpu()


@pytest.mark.parametrize("name", list(VOLUMES))
@pytest.mark.parametrize("co", [1, 3])
def test_accumulate_cl_per_element(name, co):
    plan, _, _, imp, (want, bound), (gwant, gbound), _ = _blend_case(name, co)
    outs = {b: _accumulate(name, co, b) for b in (1, 3, 5)}
    acc, wsum = outs[1]
    assert torch.isfinite(acc).all()  # the NaN of a filler row reached nothing
    err = (acc.double() / wsum.double() - want).abs()
    # acc / wsum formed in fp64 here: the bound's division rounding is not spent
    print(f"\n[{name} Co={co}] max |err| {float(err.max()):.3e}, max err / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}, "
          f"windows {plan.num_windows}")
    assert bool((err <= bound).all())
    for b in (3, 5):
        assert torch.equal(outs[b][0], acc) and torch.equal(outs[b][1], wsum), b  # enumeration order whatever the batch size
    again = _accumulate(name, co, 3)
    assert torch.equal(again[0], acc) and torch.equal(again[1], wsum)               # and from run to run
    no_host = _accumulate(name, co, 3, use_host=False)
    assert torch.equal(no_host[0], acc) and torch.equal(no_host[1], wsum)
    acc_only = _accumulate(name, co, 3, want_wsum=False)                            # a NULL wsum is left alone
    assert torch.equal(acc_only[0], acc) and float(acc_only[1].abs().max()) == 0
    # the guided form: the combination of guidance_ref per window, before the blend
    gacc, gwsum = _accumulate(name, co, 3, guided=True)
    assert torch.equal(gwsum, wsum)
    gerr = (gacc.double() / gwsum.double() - gwant).abs()
    print(f"[{name} Co={co} guided] max |err| {float(gerr.max()):.3e}, max err / bound {float((gerr / gbound.clamp(min=1e-300)).max()):.3f}")
    assert bool((gerr <= gbound).all())
    assert torch.equal(_accumulate(name, co, 5, guided=True)[0], gacc)


def test_accumulate_cl_weights_alone():
    """pred NULL: the weight sum alone, in the same order -- how a run computes wsum once."""
    from medical_image_generation_amd._lib import call, ptr
    plan, _, _, imp, _, _, _ = _blend_case("odd", 1)
    volume, roi = VOLUMES["odd"]
    acc, wsum, imp_d = torch.zeros((2, 1) + volume, device="cuda"), torch.zeros(volume, device="cuda"), imp.cuda()
    for call_rows in plan.rows(2, 5):
        dev, host = _table((2,) + volume, call_rows.tolist())
        call("mi_sw_accumulate_cl", None, None, ptr(imp_d), ptr(dev), host.data_ptr(), 5, 1, *roi, ptr(acc), ptr(wsum), acc.numel())
    assert torch.equal(wsum.cpu(), _accumulate("odd", 1, 1)[1]) and float(acc.abs().max()) == 0


# -------------------------------------------------------------------------------------------------------- 3. diffusion_step
def _step_tables():
    from medical_image_generation_amd.inferer import DDIMScheduler, DDPMScheduler
    ddpm = DDPMScheduler(**DDPM_KW)
    ddim = DDIMScheduler(1000, **G.GENTLE)
    ddim.set_timesteps(STEPS)
    # (ddim, table fp32 [rows, 5], row index, whether its sigma is non-zero)
    return [(0, ddpm._coef, 500, True), (0, ddpm._coef, 0, False), (1, ddim.rows(0.0), 1, False), (1, ddim.rows(0.5), 1, True)]


def _tiled_step(x, acc, wsum, z, table, index, flags, ddim):
    from medical_image_generation_amd._lib import call, ptr
    xd, ad, wd, zd, td = x.cuda(), acc.cuda(), wsum.cuda(), z.cuda(), table.cuda()  # every buffer outlives the launch
    idx = torch.tensor([index], device="cuda")
    n, c, v = x.shape[0], x.shape[1], x[0, 0].numel()
    call("mi_sw_diffusion_step", ptr(xd), ptr(ad), ptr(wd), ptr(zd), ptr(td), ptr(idx), n, c, v, flags, ddim)
    return xd.cpu(), ad.cpu()


@pytest.mark.parametrize("name", list(VOLUMES))
@pytest.mark.parametrize("c", [1, 3])
def test_diffusion_step_is_bit_equal_to_the_plain_step(name, c):
    """acc = 2 m and wsum = 2 with m bf16-representable: the division is exact, so the tiled update must carry the bits of
    mi_diffusion_step on the bf16 model output m -- both schedulers, both prediction types, clip on and off, sigma zero and non-zero."""
    from medical_image_generation_amd._lib import call, ptr
    volume, _ = VOLUMES[name]
    shape = (2, c) + volume
    x, z = synth.tensor(S, f"ts_sx_{name}_{c}", shape) * 1.5, synth.tensor(S, f"ts_sz_{name}_{c}", shape)
    m = synth.tensor(S, f"ts_sm_{name}_{c}", shape).to(BF16)
    m_cl = _cl(m)
    for ddim, table, index, noisy in _step_tables():
        assert (float(table[index, 4]) != 0) == noisy
        for flags in (0, 1, 2, 3):
            xd, zd, td, idx = x.cuda(), z.cuda(), table.cuda(), torch.tensor([index], device="cuda")
            call("mi_diffusion_step", ptr(xd), ptr(m_cl), ptr(zd), ptr(td), ptr(idx), None, None, None, None, None, None, 0,
                 2, c, volume[0] * volume[1] * volume[2], flags, ddim)
            got, acc = _tiled_step(x, 2 * m.float(), torch.full(volume, 2.0), z, table, index, flags, ddim)
            assert torch.equal(got, xd.cpu()), (ddim, index, flags)
            assert float(acc.abs().max()) == 0 and not torch.equal(got, x)


@pytest.mark.parametrize("name", list(VOLUMES))
def test_diffusion_step_on_general_values(name):
    volume, _ = VOLUMES[name]
    shape = (2, 3) + volume
    x, z = synth.tensor(S, f"ts_gx_{name}", shape) * 1.5, synth.tensor(S, f"ts_gz_{name}", shape)
    acc = synth.tensor(S, f"ts_ga_{name}", shape) * 2
    wsum = torch.rand(volume, generator=torch.Generator().manual_seed(S)) * 1.5 + 0.5
    m = acc.double() / wsum.double()
    for ddim, table, index, _ in _step_tables():
        for flags in (0, 1, 2, 3):
            ptype, clip = ("v_prediction" if flags & 2 else "epsilon"), bool(flags & 1)
            if ddim:
                want = ddim_ref.update(table[index].double(), x, m, z, ptype, clip)[0]
            else:
                want = step.DDPMSchedule(prediction_type=ptype).step(m, index, x.double(), z.double(), clip_sample=clip)[0]
            got, left = _tiled_step(x, acc, wsum, z, table, index, flags, ddim)
            err = float((got.double() - want).abs().max())
            assert err <= 1e-5 * max(1.0, float(want.abs().max())), (ddim, index, flags, err)
            assert float(left.abs().max()) == 0


def test_kernels_refuse_bad_arguments():
    from medical_image_generation_amd._lib import HipError, call, ptr
    (d, h, w), roi = VOLUMES["aligned"]
    x = torch.zeros((2, 1, d, h, w), device="cuda")
    out = torch.zeros((2,) + roi + (1,), dtype=BF16, device="cuda")
    good = [(0, 0, 0, 0), (1, 2, 4, 8)]
    dev, host = _table((2, d, h, w), good)
    bad_rows = [[(0, 3, 0, 0), (1, 0, 0, 0)], [(0, 0, 0, 9), (1, 0, 0, 0)], [(0, 0, -1, 0), (1, 0, 0, 0)], [(2, 0, 0, 0), (1, 0, 0, 0)]]
    for rows in bad_rows:  # a window that leaves the case: there is no padding
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            call("mi_sw_gather_cl", ptr(x), x.numel(), 1, None, 0, 0, ptr(dev), _table((2, d, h, w), rows)[1].data_ptr(), 2, 0, *roi, ptr(out))
    with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):  # condition channels without a condition
        call("mi_sw_gather_cl", ptr(x), x.numel(), 1, None, 0, 2, ptr(dev), host.data_ptr(), 2, 0, *roi, ptr(out))
    with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):  # the table's tensor is larger than the buffer
        call("mi_sw_gather_cl", ptr(x), x.numel() - 1, 1, None, 0, 0, ptr(dev), host.data_ptr(), 2, 0, *roi, ptr(out))
    call("mi_sw_gather_cl", ptr(x), x.numel(), 1, None, 0, 0, ptr(dev), host.data_ptr(), 2, 0, *roi, ptr(out))
    acc, wsum, imp = torch.zeros_like(x), torch.zeros((d, h, w), device="cuda"), torch.ones(roi, device="cuda")
    for rows in bad_rows:
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            call("mi_sw_accumulate_cl", ptr(out), None, ptr(imp), ptr(dev), _table((2, d, h, w), rows)[1].data_ptr(), 2, 1, *roi, ptr(acc), ptr(wsum),
                 acc.numel())
    with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):  # neither predictions nor a weight sum
        call("mi_sw_accumulate_cl", None, None, ptr(imp), ptr(dev), host.data_ptr(), 2, 1, *roi, ptr(acc), None, acc.numel())
    idx, tab, z = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.ones((1, 5), device="cuda"), torch.zeros_like(x)
    for kw in (dict(x=None), dict(acc=None), dict(wsum=None), dict(z=None), dict(n=0), dict(v=0)):
        a = dict(x=ptr(x), acc=ptr(acc), wsum=ptr(wsum), z=ptr(z), n=2, v=d * h * w)
        a.update(kw)
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            call("mi_sw_diffusion_step", a["x"], a["acc"], a["wsum"], a["z"], ptr(tab), ptr(idx), a["n"], 1, a["v"], 0, 0)
    assert float(acc.abs().max()) == 0 and float(wsum.abs().max()) == 0  # nothing was launched


# --------------------------------------------------------------------------------------------------------------- the loops
@functools.lru_cache(maxsize=None)
def _nets(case, **override):
    """(the oracle's CPU U-Net in eval mode, the product's on the GPU) with the same synthetic weights."""
    from medical_image_generation_amd.unet import DiffusionModelUNet
    kw = dict(cases.UNET_CASES[case]["kwargs"], **override)
    ref = nets.DiffusionModelUNet(**kw)
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    ref.load_state_dict(sd)
    net = DiffusionModelUNet(**kw)
    net.load_state_dict(sd)
    return ref.eval(), net.cuda().eval()


def _scheduler(kind, prediction_type="epsilon"):
    from medical_image_generation_amd.inferer import DDIMScheduler, DDPMScheduler
    sch = DDPMScheduler(prediction_type=prediction_type, **DDPM_KW) if kind == "ddpm" else DDIMScheduler(1000, prediction_type=prediction_type,
                                                                                                        **G.GENTLE)
    sch.set_timesteps(STEPS)
    return sch


def _reference_loop(kind, eta=0.0):
    """(timesteps, update) of tiled_sampling_ref.sample for the scheduler `_scheduler(kind)` builds."""
    ts = ddim_ref.timesteps(1000, STEPS)
    if kind == "ddpm":
        sch = step.DDPMSchedule()
        return ts, lambda i, t, x, m, z: sch.step(m, t, x, None if z is None else z.double(), clip_sample=True)[0]
    acp, _ = ddim_ref.alphas_cumprod(1000, **G.GENTLE)
    rows = ddim_ref.rows(acp, STEPS, eta)
    return ts, lambda i, t, x, m, z: ddim_ref.update(rows[i], x, m, z, "epsilon", True)[0]


def _oracle_model(ref, labels=None, context=None):
    def f(inp, t, n, null):
        kw = {}
        if labels is not None:
            kw["class_labels"] = torch.tensor([G.NULL_CLASS if null else int(labels[n])])
        if context is not None:
            kw["context"] = torch.zeros_like(context[n:n + 1]) if null else context[n:n + 1]
        with torch.no_grad():
            return ref(inp, torch.full((1,), t, dtype=torch.int64), **kw)
    return f


def _noises(name, shape):
    return [synth.tensor(S, f"ts_{name}_z{i}", shape) for i in range(STEPS)]


# ------------------------------------------------------------------------------------- 4. one window is the plain sampler
@pytest.mark.parametrize("kind,ptype,eta", [("ddpm", "epsilon", 0.0), ("ddim", "epsilon", 0.0), ("ddim", "epsilon", 0.5), ("ddpm", "v_prediction", 0.0),
                                            ("ddim", "v_prediction", 0.5)])
def test_one_window_is_the_plain_sampler(kind, ptype, eta):
    """A window that covers the case, mode="constant": acc = 1 * p, wsum = 1, and the update is the plain step's own arithmetic.
    (Gaussian mode is excluded: (imp p) / imp is not p bit for bit.)"""
    from medical_image_generation_amd.inferer import DiffusionInferer
    from medical_image_generation_amd.sliding import SlidingWindowInferer
    _, net = _nets("unet3d")
    shape = (2, 1, 16, 16, 16)
    sch = _scheduler(kind, ptype)
    x0 = synth.tensor(S, "ts_one_noise", shape).cuda()
    zs = [z.cuda() for z in _noises("one", shape)]
    inf = DiffusionInferer(sch)
    win = SlidingWindowInferer(16, 2, 0.25, "constant")
    want, want_inter = inf.sample(x0, net, sch, verbose=False, noises=zs, eta=eta, save_intermediates=True, intermediate_steps=250)
    got, inter = inf.sample(x0, net, sch, verbose=False, noises=zs, eta=eta, save_intermediates=True, intermediate_steps=250, window_inferer=win)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert len(inter) == len(want_inter) == STEPS and all(torch.equal(a, b) for a, b in zip(inter, want_inter))
    if kind == "ddim" and ptype == "epsilon" and eta == 0.0:  # the other entries of the surface, on the same loop
        image = synth.tensor(S, "ts_one_image", shape).clamp(-1, 1).cuda()
        assert torch.equal(inf.invert(image, net, sch, window_inferer=win), inf.invert(image, net, sch))
        assert torch.equal(inf.img2img(image, net, 0.5, x0, sch, verbose=False, window_inferer=win), inf.img2img(image, net, 0.5, x0, sch, verbose=False))


def test_one_window_is_the_plain_guided_sampler():
    from medical_image_generation_amd.inferer import DiffusionInferer
    from medical_image_generation_amd.sliding import SlidingWindowInferer
    _, net = _nets("unet2d_class")
    c = cases.UNET_CASES["unet2d_class"]
    shape, labels = tuple(c["shape"]), torch.tensor(c["class_labels"]).cuda()
    assert shape == (2, 1, 16, 16)
    sch = _scheduler("ddim")
    x0 = synth.tensor(S, "ts_oneg_noise", shape).cuda()
    inf = DiffusionInferer(sch)
    kw = dict(verbose=False, class_labels=labels, guidance_scale=G.W["class"], null_class=G.NULL_CLASS)
    want = inf.sample(x0, net, sch, **kw)
    got = inf.sample(x0, net, sch, window_inferer=SlidingWindowInferer(16, 2, 0.25, "constant"), **kw)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(got, inf.sample(x0, net, sch, verbose=False, class_labels=labels))  # the guidance matters


# --------------------------------------------------------------------------------- 5. several windows against the oracle
MULTI = (2, 1, 16, 24, 24)


@functools.lru_cache(maxsize=None)
def _multi_reference(kind, mode):
    ref, _ = _nets("unet3d")
    ts, update = _reference_loop(kind)
    x0 = synth.tensor(S, "ts_multi_noise", MULTI)
    return T.sample(x0, _oracle_model(ref), ts, update, 16, 0.5, mode, noises=_noises("multi", MULTI))


@functools.lru_cache(maxsize=None)
def _multi_on_gpu(kind, mode, batch, use_graph=True):
    from medical_image_generation_amd.inferer import DiffusionInferer
    from medical_image_generation_amd.sliding import SlidingWindowInferer
    _, net = _nets("unet3d")
    sch = _scheduler(kind)
    inf = DiffusionInferer(sch)
    x0 = synth.tensor(S, "ts_multi_noise", MULTI).cuda()
    zs = [z.cuda() for z in _noises("multi", MULTI)]
    win = SlidingWindowInferer(16, batch, 0.5, mode)
    got = inf.sample(x0, net, sch, verbose=False, noises=zs, use_graph=use_graph, window_inferer=win)
    return got.cpu(), inf, (x0, net, sch, zs, win)


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_several_windows_match_the_oracle(kind, mode):
    """(16, 24, 24) under 16^3 windows at overlap 0.5: 4 windows per image; batch 3 -> 3 calls, the second mixes both images, the last
    ends in one filler row (tests/test_tiled_sampling_cpu.py asserts the plan)."""
    from medical_image_generation_amd.sliding import WindowPlan
    plan = WindowPlan(MULTI[2:], 16, 0.5)
    assert plan.starts == [[0], [0, 8], [0, 8]] and plan.rows(2, 3)[:, :, 0].tolist() == [[0, 0, 0], [0, 1, 1], [1, 1, -1]]
    want = _multi_reference(kind, mode)
    got = _multi_on_gpu(kind, mode, 3)[0]
    err = G.rel(got, want)
    print(f"\n[tiled {kind} {mode}] rel-L2 after {STEPS} steps: {err:.3e}")
    assert torch.isfinite(got).all() and err <= BOUND
    assert torch.equal(_multi_on_gpu(kind, mode, 1)[0], got)  # the blend does not depend on the batch size


# ----------------------------------------------------------------------------------------------------------- 6. conditioning
def test_concat_conditioning_follows_the_window():
    """unet_ldm with 9 input channels on (8, 8, 12) under 8^3 windows: 2 windows along W; the condition is a ramp along W, so a window
    that read the condition at another offset does not fit."""
    from medical_image_generation_amd.inferer import DiffusionInferer
    from medical_image_generation_amd.sliding import SlidingWindowInferer, WindowPlan
    ref, net = _nets("unet_ldm", in_channels=9, out_channels=8)
    shape = (1, 8, 8, 8, 12)
    assert WindowPlan(shape[2:], 8, 0.5).windows == [(0, 0, 0), (0, 0, 4)]
    x0 = synth.tensor(S, "ts_concat_noise", shape)
    cond = torch.linspace(-1, 1, 12).expand(1, 1, 8, 8, 12).contiguous()
    ts, update = _reference_loop("ddim")
    want = T.sample(x0, _oracle_model(ref), ts, update, 8, 0.5, "gaussian", cond=cond)
    shifted = T.sample(x0, _oracle_model(ref), ts, update, 8, 0.5, "gaussian", cond=cond.flip(-1))
    sch = _scheduler("ddim")
    got = DiffusionInferer(sch).sample(x0.cuda(), net, sch, conditioning=cond.cuda(), mode="concat", verbose=False,
                                       window_inferer=SlidingWindowInferer(8, 2, 0.5, "gaussian")).cpu()
    err = G.rel(got, want)
    print(f"\n[tiled concat] rel-L2: {err:.3e}; a mirrored condition lies {G.rel(shifted, want):.3e} away")
    assert torch.isfinite(got).all() and err <= BOUND
    assert G.rel(shifted, want) > 2 * BOUND  # the condition matters at this size


@pytest.mark.parametrize("guided", [False, True])
def test_labels_follow_the_window(guided):
    """unet2d_class on (16, 24) under 16^2 windows, two images with different labels, batch 3: the first call holds both windows of
    image 0 and the first of image 1."""
    from medical_image_generation_amd.inferer import DiffusionInferer
    from medical_image_generation_amd.sliding import SlidingWindowInferer, WindowPlan
    ref, net = _nets("unet2d_class")
    shape, labels = (2, 1, 16, 24), torch.tensor(cases.UNET_CASES["unet2d_class"]["class_labels"])
    assert WindowPlan(shape[2:], 16, 0.5).rows(2, 3)[:, :, 0].tolist() == [[0, 0, 1], [1, -1, -1]] and labels[0] != labels[1]
    x0 = synth.tensor(S, "ts_label_noise", shape)
    ts, update = _reference_loop("ddim")
    w = G.W["class"] if guided else None
    want = T.sample(x0, _oracle_model(ref, labels), ts, update, 16, 0.5, "gaussian", w=w)
    sch = _scheduler("ddim")
    kw = dict(guidance_scale=w, null_class=G.NULL_CLASS) if guided else {}
    got = DiffusionInferer(sch).sample(x0.cuda(), net, sch, verbose=False, class_labels=labels.cuda(),
                                       window_inferer=SlidingWindowInferer(16, 3, 0.5, "gaussian"), **kw).cpu()
    err = G.rel(got, want)
    print(f"\n[tiled labels guided={guided}] rel-L2: {err:.3e}")
    assert torch.isfinite(got).all() and err <= BOUND


def test_context_follows_the_window():
    """unet2d_xattn on (16, 24) under 16^2 windows, a context per image, batch 3 (the first call mixes the images), guided at w = 2:
    the null half of the model's batch reads zero tokens."""
    from medical_image_generation_amd.inferer import DiffusionInferer
    from medical_image_generation_amd.sliding import SlidingWindowInferer
    ref, net = _nets("unet2d_xattn")
    shape = (2, 1, 16, 24)
    context = synth.tensor(S, "context", cases.UNET_CASES["unet2d_xattn"]["context"])
    x0 = synth.tensor(S, "ts_ctx_noise", shape)
    ts, update = _reference_loop("ddim")
    sch = _scheduler("ddim")
    inf = DiffusionInferer(sch)
    for w in (None, G.W["xattn"]):
        want = T.sample(x0, _oracle_model(ref, context=context), ts, update, 16, 0.5, "gaussian", w=w)
        got = inf.sample(x0.cuda(), net, sch, verbose=False, conditioning=context.cuda(), guidance_scale=w,
                         window_inferer=SlidingWindowInferer(16, 3, 0.5, "gaussian")).cpu()
        err = G.rel(got, want)
        print(f"\n[tiled context w={w}] rel-L2: {err:.3e}")
        assert torch.isfinite(got).all() and err <= BOUND
    swapped = T.sample(x0, _oracle_model(ref, context=context.flip(0)), ts, update, 16, 0.5, "gaussian")
    assert G.rel(swapped, T.sample(x0, _oracle_model(ref, context=context), ts, update, 16, 0.5, "gaussian")) > BOUND  # whose context matters


# ---------------------------------------------------------------------------------------------------------- 7. captured mode
def test_captured_mode_is_bit_equal_to_eager_and_captures_once():
    got, inf, (x0, net, sch, zs, win) = _multi_on_gpu("ddim", "gaussian", 3)
    loops = list(inf._loops.values())
    assert len(loops) == 1 and loops[0].graph is not None and loops[0].captures == 1
    eager = _multi_on_gpu("ddim", "gaussian", 3, use_graph=False)
    assert eager[1]._loops and next(iter(eager[1]._loops.values())).graph is None
    assert torch.equal(eager[0], got)
    again = inf.sample(x0, net, sch, verbose=False, noises=zs, window_inferer=win)
    assert torch.equal(again.cpu(), got)
    assert list(inf._loops.values()) == loops and loops[0].captures == 1  # the same loop, no new capture


# --------------------------------------------------------------------------------------------------------- 8. latent inferer
def test_latent_inferer_samples_and_decodes_tiled():
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    from medical_image_generation_amd.inferer import DiffusionInferer, LatentDiffusionInferer
    from medical_image_generation_amd.sliding import SlidingWindowInferer, tiled_decode
    ae = AutoencoderKL(**cases.AEKL_CASES["aekl_c3a"]["kwargs"])
    ae.load_state_dict(synth.state_dict({k: tuple(v.shape) for k, v in ae.state_dict().items()}, S))
    ae = ae.cuda().eval()
    _, net = _nets("unet_ldm")
    sch = _scheduler("ddpm")
    shape = (1, 8, 8, 8, 12)
    z = synth.tensor(S, "ts_latent_noise", shape).cuda()
    zs = [n.cuda() for n in _noises("latent", shape)]
    scale = 0.7
    lat = DiffusionInferer(sch).sample(z, net, sch, verbose=False, noises=zs, window_inferer=SlidingWindowInferer(8, 2, 0.5, "gaussian"))
    assert not torch.equal(lat, DiffusionInferer(sch).sample(z, net, sch, verbose=False, noises=zs))  # 8^3 windows see less than the whole latent
    img = LatentDiffusionInferer(sch, scale_factor=scale).sample(z, ae, net, sch, verbose=False, noises=zs,
                                                                 window_inferer=SlidingWindowInferer(8, 2, 0.5, "gaussian"),
                                                                 decode_inferer=SlidingWindowInferer(4, 2, 0.5, "gaussian"))
    assert img.shape == (1, 1, 32, 32, 48) and torch.isfinite(img).all()
    assert torch.equal(img, tiled_decode(ae, lat / scale, SlidingWindowInferer(4, 2, 0.5, "gaussian")))


# -------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_and_the_plain_call_still_runs():
    from medical_image_generation_amd.inferer import DiffusionInferer
    from medical_image_generation_amd.sliding import SlidingWindowInferer
    _, net = _nets("unet3d")
    sch = _scheduler("ddim")
    inf = DiffusionInferer(sch)
    shape = (2, 1, 16, 16, 16)
    x0 = synth.tensor(S, "ts_one_noise", shape).cuda()
    with pytest.raises(ValueError, match="smaller than the window"):
        inf.sample(x0, net, sch, verbose=False, window_inferer=SlidingWindowInferer((16, 16, 24), 1, 0.5))
    mask = torch.ones((1, 1, 16, 16, 16), device="cuda")
    with pytest.raises(NotImplementedError, match="window_inferer"):
        inf.inpaint(x0.clamp(-1, 1), mask, net, scheduler=sch, verbose=False, window_inferer=SlidingWindowInferer(16, 1, 0.5))
    got = inf.sample(x0, net, sch, verbose=False)
    assert got.shape == shape and torch.isfinite(got).all()
