"""Classifier-free guidance on the HIP path (Ho & Salimans 2022; not part of the reference: PARITY UNPINNED): the guided update kernels
against the fp64 restatements (tests/guidance_ref.py on tests/ddim_ref.py / oracle/step.py), the condition-dropout kernels against the
torch expression, the train step with a drop mask against the step on the effective inputs, and the guided sample loop against the
two-pass loop on the oracle's fp32 U-Net.  Null means zeros (context, condition channels) or `null_class` (labels)."""
import functools

import pytest
import torch

from oracle import cases, step, synth
from tests import ddim_ref
from tests import guidance_ref as G

pytestmark = pytest.mark.gpu
S = cases.SEED
TRAIN = dict(schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205)
SHAPE = (2, 3, 4, 6, 5)  # V = 120: no multiple of the wave or the block
SCALES = (0.0, 1.0, 2.5)


# ---------------------------------------------------------------------------------------------------------------- guided update kernels
@functools.lru_cache(maxsize=None)
def _kernel_inputs():
    from medical_image_generation_amd import hipops as ops
    N, C = SHAPE[0], SHAPE[1]
    x, z = synth.tensor(S, "cfg_x", SHAPE) * 1.5, synth.tensor(S, "cfg_z", SHAPE)
    mc = synth.tensor(S, "cfg_mc", SHAPE).bfloat16().float()  # the model output is bf16; the two halves are distinct tensors
    mu = synth.tensor(S, "cfg_mu", SHAPE).bfloat16().float()
    mo_cl = ops.to_channels_last(torch.cat([mc, mu]).cuda())  # batch 2N: [conditional, unconditional]
    sentinel = synth.tensor(S, "cfg_cond", (2 * N, 4, 6, 5, 2)).bfloat16().cuda()
    return x, z, mc, mu, mo_cl, z.cuda(), sentinel


def _launch_and_check(ddim, table, idx, wd, flags, want, cs, worst, what):
    """One guided launch of `mi_diffusion_step` (no known region) at x_cl pitch cs (0: no x_cl) and every check of its outputs."""
    from medical_image_generation_amd import hipops as ops
    from medical_image_generation_amd._lib import call, ptr
    x, _, _, _, mo_cl, zd, sentinel = _kernel_inputs()
    N, C, V = SHAPE[0], SHAPE[1], 4 * 6 * 5
    xd = x.cuda()
    x_cl = None
    if cs:
        x_cl = torch.zeros((2 * N, 4, 6, 5, cs), dtype=torch.bfloat16, device="cuda")
        x_cl[..., C:] = sentinel[..., :cs - C]
    call("mi_diffusion_step", ptr(xd), ptr(mo_cl), ptr(zd), ptr(table), ptr(idx), ptr(wd), None, None, None, None, ptr(x_cl), cs, N, C, V, flags,
         ddim)
    tol = 1e-5 * max(1.0, float(want.abs().max()))
    err = float((xd.cpu().double() - want).abs().max())
    worst[0] = max(worst[0], err / tol)
    assert err <= tol, (what, cs, err, tol)
    if cs:
        halves = x_cl[:N, ..., :C].contiguous(), x_cl[N:, ..., :C].contiguous()
        assert torch.equal(halves[0].view(torch.int16), halves[1].view(torch.int16)), (what, cs)  # both halves, bit for bit
        err_cl = float((ops.to_channels_first(halves[0]).cpu().double() - want).abs().max())
        worst[1] = max(worst[1], err_cl / (1e-2 * float(want.abs().max())))
        assert err_cl <= 1e-2 * float(want.abs().max()), (what, cs, err_cl)
        assert torch.equal(x_cl[..., C:].view(torch.int16), sentinel[..., :cs - C].view(torch.int16)), (what, cs)  # the condition stays


def test_ddim_step_guided_kernel_matches_closed_form():
    """The cases of test_ddim_step_kernel_matches_closed_form (both prediction types, clip on / off, first / middle / last row, eta 0 and
    0.5, reverse; x_cl pitch C, C + 2, none) at w in {0, 1, 2.5} on a batch-4 model output with distinct halves; expected values:
    ddim_ref.update in fp64 on the fp64 combination.  Bounds of the unguided kernel test: fp32 1e-5 max(1, max|want|), bf16 1e-2 max|want|."""
    from medical_image_generation_amd.inferer import DDIMScheduler
    x, z, mc, mu, _, _, _ = _kernel_inputs()
    C, n = SHAPE[1], 10
    acp, _ = ddim_ref.alphas_cumprod(1000, **TRAIN)
    idx = torch.zeros(1, dtype=torch.int64, device="cuda")
    wd = torch.zeros(1, device="cuda")
    worst = [0.0, 0.0]
    for pred in ("epsilon", "v_prediction"):
        for clip in (True, False):
            sch = DDIMScheduler(prediction_type=pred, clip_sample=clip, **TRAIN)
            sch.set_timesteps(n)
            flags = int(clip) | (2 if pred == "v_prediction" else 0)
            for eta, reverse in ((0.0, False), (0.5, False), (0.0, True)):
                table = sch.rows(eta, reverse).cuda()
                want_rows = ddim_ref.rows(acp, n, eta, reverse=reverse)
                for i in (0, 5, n - 1):
                    idx.fill_(i)
                    for w in SCALES:
                        wd.fill_(w)
                        want, _ = ddim_ref.update(want_rows[i], x, G.combine(mc, mu, w), z, prediction_type=pred, clip_sample=clip)
                        for cs in (C, C + 2, 0):
                            _launch_and_check(1, table, idx, wd, flags, want, cs, worst, (pred, clip, eta, reverse, i, w))
    print(f"\n[mi_diffusion_step ddim guided] worst error / bound: fp32 {worst[0]:.3f}, bf16 copy {worst[1]:.3f}")
    assert float((G.combine(mc, mu, 2.5) - mc.double()).abs().max()) > 1.0  # the halves differ: a swapped or dropped branch shows


def test_ddpm_step_guided_kernel_matches_closed_form():
    """t in {0, 500, 999} (no noise at 0), both prediction types, clip on / off, w in {0, 1, 2.5}, the three x_cl pitches; expected values:
    oracle/step.py's DDPMSchedule.step evaluated in fp64 on the fp64 combination."""
    from medical_image_generation_amd.inferer import DDPMScheduler
    x, z, mc, mu, _, _, _ = _kernel_inputs()
    C = SHAPE[1]
    td = torch.zeros(1, dtype=torch.int64, device="cuda")
    wd = torch.zeros(1, device="cuda")
    worst = [0.0, 0.0]
    for pred in ("epsilon", "v_prediction"):
        sch = DDPMScheduler(num_train_timesteps=1000, prediction_type=pred, **TRAIN)
        ref = step.DDPMSchedule(prediction_type=pred)
        table = sch.coefficients("cuda")
        for clip in (True, False):
            flags = int(clip) | (2 if pred == "v_prediction" else 0)
            for t in (0, 500, 999):
                td.fill_(t)
                for w in SCALES:
                    wd.fill_(w)
                    want, _ = ref.step(G.combine(mc, mu, w), t, x.double(), z.double(), clip_sample=clip)
                    assert want.dtype == torch.float64
                    for cs in (C, C + 2, 0):
                        _launch_and_check(0, table, td, wd, flags, want, cs, worst, (pred, clip, t, w))
    print(f"\n[mi_diffusion_step ddpm guided] worst error / bound: fp32 {worst[0]:.3f}, bf16 copy {worst[1]:.3f}")


@pytest.mark.parametrize("ddim", [1, 0], ids=["ddim", "ddpm"])
def test_guided_step_kernels_refuse_bad_arguments(ddim):
    """What the guided entries refused, on the one entry that replaced them -- but a NULL guidance is the unguided step now."""
    from medical_image_generation_amd._lib import HipError, call, ptr
    x = torch.zeros(2, 3, 120, device="cuda")
    mo = torch.zeros(4, 120, 3, dtype=torch.bfloat16, device="cuda")
    x_cl = torch.zeros(4, 120, 3, dtype=torch.bfloat16, device="cuda")
    rows = torch.ones(4, 5, device="cuda")
    idx = torch.zeros(1, dtype=torch.int64, device="cuda")
    w = torch.ones(1, device="cuda")
    good = [ptr(x), ptr(mo), ptr(x), ptr(rows), ptr(idx), ptr(w), None, None, None, None, ptr(x_cl), 3, 2, 3, 120, 1, ddim]
    for k in range(5):  # x, model_out, noise, table, index
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            call("mi_diffusion_step", *(good[:k] + [None] + good[k + 1:]))
    for k, v in ((11, 2), (12, 0), (13, 0), (14, 0), (12, -1), (14, -5)):  # x_cl pitch below C; non-positive N, C, V
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            call("mi_diffusion_step", *(good[:k] + [v] + good[k + 1:]))
    call("mi_diffusion_step", *good)  # (the unchanged arguments are accepted)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- dropout kernels
def test_select_labels_and_dropped_cast_match_torch():
    from medical_image_generation_amd._lib import HipError, call, ptr
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    labels = torch.tensor([1, 3, 2], device="cuda")
    out = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    call("mi_select_labels", ptr(labels), ptr(mask), 5, ptr(out), 3)
    assert torch.equal(out, torch.where(mask.bool(), torch.full_like(labels, 5), labels))
    as_bool = mask.bool()
    call("mi_select_labels", ptr(labels), ptr(as_bool.view(torch.uint8)), 0, ptr(out), 3)  # a bool mask's bytes
    assert out.tolist() == [0, 3, 0]
    src = synth.tensor(S, "cfg_ctx", (3, 5 * 16)).cuda()
    dst = torch.full((3, 5 * 16), 9.0, dtype=torch.bfloat16, device="cuda")
    call("mi_cast_bf16_drop", ptr(src), ptr(dst), ptr(mask), 3, 5 * 16)
    want = torch.where(mask.bool()[:, None], torch.zeros_like(src), src).bfloat16()
    assert torch.equal(dst.view(torch.int16), want.view(torch.int16))
    for bad in ([None, ptr(mask), 0, ptr(out), 3], [ptr(labels), None, 0, ptr(out), 3], [ptr(labels), ptr(mask), 0, None, 3],
                [ptr(labels), ptr(mask), -1, ptr(out), 3], [ptr(labels), ptr(mask), 0, ptr(out), 0]):
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            call("mi_select_labels", *bad)
    for bad in ([None, ptr(dst), ptr(mask), 3, 80], [ptr(src), None, ptr(mask), 3, 80], [ptr(src), ptr(dst), None, 3, 80],
                [ptr(src), ptr(dst), ptr(mask), 0, 80], [ptr(src), ptr(dst), ptr(mask), 3, 0]):
        with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
            call("mi_cast_bf16_drop", *bad)


def test_qsample_drop_matches_qsample_on_a_zeroed_condition():
    """(3, 2 + 2, 4, 6, 5), mask [1, 0, 1]: bit-equal to mi_qsample on a condition whose dropped samples were zeroed on the host (model
    input and velocity); with an all-zero mask bit-equal to mi_qsample on the condition as it is."""
    from medical_image_generation_amd._lib import HipError, call, ptr
    from medical_image_generation_amd.trainer import DDPMSchedule
    n, c, cc, v = 3, 2, 2, 4 * 6 * 5
    sch = DDPMSchedule(device="cuda")
    x0, noise = synth.tensor(S, "cfg_q_x0", (n, c, 4, 6, 5)).cuda(), synth.tensor(S, "cfg_q_n", (n, c, 4, 6, 5)).cuda()
    cond = synth.tensor(S, "cfg_q_c", (n, cc, 4, 6, 5)).cuda()
    t = torch.tensor([0, 417, 999], device="cuda")
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")

    def run(entry, cond_, *tail):
        out = torch.full((n, 4, 6, 5, c + cc), 3.0, dtype=torch.bfloat16, device="cuda")
        vel = torch.full((n, c, 4, 6, 5), 3.0, device="cuda")
        call(entry, ptr(x0), ptr(noise), ptr(sch.sqrt_acp), ptr(sch.sqrt_1macp), ptr(t), ptr(cond_), cc, ptr(out), ptr(vel), n, c, v, 1000, *tail)
        return out.view(torch.int16), vel

    zeroed = cond.clone()
    zeroed[mask.bool()] = 0.0
    got, want, plain = run("mi_qsample_drop", cond, ptr(mask)), run("mi_qsample", zeroed), run("mi_qsample", cond)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], plain[0]) and torch.equal(got[0][1], plain[0][1])  # the kept sample is the plain one
    keep_all = torch.zeros_like(mask)  # (held: a temporary's memory would be handed to `out` before the kernel reads it)
    none = run("mi_qsample_drop", cond, ptr(keep_all))
    assert torch.equal(none[0], plain[0]) and torch.equal(none[1], plain[1])
    with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
        run("mi_qsample_drop", cond, None)


# ---------------------------------------------------------------------------------------------------------------- train step
def _product_net(route):
    from medical_image_generation_amd.unet import DiffusionModelUNet
    kw, sd, _, _, _ = G.case(route)
    net = DiffusionModelUNet(**kw)
    net.load_state_dict(sd)
    return net.cuda()


@functools.lru_cache(maxsize=None)
def _step_inputs(route):
    """-> (x0, noise, timesteps, labels, context, condition) on the device, at the shapes of the sampling tests."""
    _, _, _, shape, cond = G.case(route)
    t ={"class": cases.UNET_CASES["unet2d_class"]["timesteps"], "xattn": cases.UNET_CASES["unet2d_xattn"]["timesteps"], "concat": (250, 750)}[route]
    x0, noise = synth.tensor(S, "cfg_x0", shape) * 0.5, synth.tensor(S, "noise0", shape)
    return tuple(None if a is None else a.cuda().contiguous() for a in (x0, noise, torch.tensor(t), cond.get("labels"), cond.get("context"), cond.get("cond")))


def _effective(inputs, mask):
    """What a step with `mask` must compute, built on the host: label -> null_class, context rows -> 0, condition channels -> 0."""
    x0, noise, t, labels, context, condition = inputs
    m = torch.tensor(mask, dtype=torch.bool, device="cuda")
    if labels is not None:
        labels = torch.where(m, torch.full_like(labels, G.NULL_CLASS), labels)
    if context is not None:
        context = context.clone()
        context[m] = 0.0
    if condition is not None:
        condition = condition.clone()
        condition[m] = 0.0
    return x0, noise, t, labels, context, condition


def _trainer(route):
    from medical_image_generation_amd.trainer import DDPMTrainer
    return DDPMTrainer(_product_net(route), lr=cases.STEP_LR, optimizer="AdamW", max_grad_norm=1.0, null_class=G.NULL_CLASS if route == "class" else None)


def _state(tr, loss):
    """-> (loss, gradients, parameters, what the model read: bf16 input, context tokens, labels)."""
    n = tr.arena.n_trainable
    x_t, _, ctx_tokens, _, labels, _ = tr._keep
    read = tuple(None if t is None else t.clone() for t in (x_t, ctx_tokens, labels))
    return loss.clone(), tr.arena.grad[:n].clone(), tr.arena.data[:n].clone(), read


@functools.lru_cache(maxsize=None)
def _eager(route, variant):
    """(loss, gradients, parameters) after ONE eager step from the route's initial state."""
    inputs, tr = _step_inputs(route), _trainer(route)
    if variant == "plain":
        return _state(tr, tr.step(*inputs))
    if variant == "zero_mask":
        return _state(tr, tr.step(*inputs, torch.zeros(2, dtype=torch.bool, device="cuda")))
    if variant == "drop":
        return _state(tr, tr.step(*inputs, torch.tensor([1, 0], dtype=torch.uint8, device="cuda")))
    if variant == "effective":
        return _state(tr, tr.step(*_effective(inputs, [1, 0])))
    raise ValueError(variant)


@pytest.mark.parametrize("route", G.ROUTES)
def test_step_with_a_mask_is_the_step_on_the_effective_inputs(route):
    """Batch 2, mask [1, 0]: equal loss; gradients (and the parameters after the optimizer) to rtol 1e-5 -- slack only because the
    embedding backward uses atomics.  The mask matters: the plain step's loss differs."""
    got, want, plain = _eager(route, "drop"), _eager(route, "effective"), _eager(route, "plain")
    print(f"\n[{route} drop [1, 0]] loss {float(got[0]):.6f} (effective inputs {float(want[0]):.6f}, plain {float(plain[0]):.6f}); "
          f"max gradient difference {float((got[1] - want[1]).abs().max()):.3e}")
    assert torch.equal(got[0], want[0])
    assert torch.allclose(got[1], want[1], rtol=1e-5) and torch.allclose(got[2], want[2], rtol=1e-5)
    assert not torch.equal(got[0], plain[0]) and not torch.allclose(got[1], plain[1], rtol=1e-3)


@pytest.mark.parametrize("route", G.ROUTES)
def test_step_with_an_all_zero_mask_is_the_step_without_one(route):
    """Bit-identical where a step is bit-reproducible at all: everything the model reads (bf16 input with the condition channels,
    context tokens, labels) and the loss.  The gradients of two runs of the SAME step already differ in the last bits (measured on
    the step without a mask: bias and norm gradients are summed with fp32 atomics in arrival order), so they and the parameters are
    held to the rtol 1e-5 of the test above."""
    got, want = _eager(route, "zero_mask"), _eager(route, "plain")
    for a, b in zip(got[3], want[3]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else a.dtype), b.view(torch.int16 if b.dtype == torch.bfloat16 else b.dtype))), route
    assert torch.equal(got[0], want[0]), route
    assert torch.allclose(got[1], want[1], rtol=1e-5) and torch.allclose(got[2], want[2], rtol=1e-5), route


@pytest.mark.parametrize("route", G.ROUTES)
def test_captured_step_takes_a_new_mask_per_replay(route):
    """capture() with mask [0, 1], step_graph() with [1, 0] (given as bool, captured as uint8): the eager step with [1, 0]."""
    inputs, tr = _step_inputs(route), _trainer(route)
    tr.capture(*inputs, torch.tensor([0, 1], dtype=torch.uint8, device="cuda"))
    loss = tr.step_graph(*inputs, torch.tensor([True, False], device="cuda"))
    got, want = _state(tr, loss), _eager(route, "drop")
    assert torch.equal(got[0], want[0])
    assert torch.allclose(got[1], want[1], rtol=1e-5) and torch.allclose(got[2], want[2], rtol=1e-5)


def test_validate_takes_the_mask():
    """validate(..., drop) is the validation batch on the effective inputs, eager and captured with another mask."""
    inputs, tr = _step_inputs("class"), _trainer("class")
    want = float(tr.validate(*_effective(inputs, [1, 0])))
    plain = float(tr.validate(*inputs))
    got = float(tr.validate(*inputs, torch.tensor([1, 0], dtype=torch.uint8, device="cuda")))
    tr.capture_validate(*inputs, torch.tensor([0, 1], dtype=torch.uint8, device="cuda"))
    got_g = float(tr.validate_graph(*inputs, torch.tensor([1, 0], dtype=torch.uint8, device="cuda")))
    assert got == want and got_g == want and got != plain


def test_ldm_trainer_takes_the_mask():
    """LDMTrainer(images, eps, noise, t, None, None, condition, drop): the mask reaches the diffusion step behind the frozen encoder --
    equal loss and gradients at rtol 1e-5 against the step on a condition whose dropped sample was zeroed on the host."""
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    from medical_image_generation_amd.trainer import LDMTrainer
    ae = AutoencoderKL(**cases.AEKL_CASES["aekl_c3a"]["kwargs"])
    ae.load_state_dict(synth.state_dict({k: tuple(v.shape) for k, v in ae.state_dict().items()}, S))
    tr = LDMTrainer(_product_net("concat"), ae.cuda(), scale_factor=0.7, lr=cases.STEP_LR)
    images = synth.ellipsoid_volume(S, "x", (2, 1, 32, 32, 32)).cuda()
    eps, noise = synth.tensor(S, "eps", (2, 8, 8, 8, 8)).cuda(), synth.tensor(S, "lnoise", (2, 8, 8, 8, 8)).cuda()
    t, label = torch.tensor([250, 750], device="cuda"), G.case("concat")[4]["cond"].cuda()
    mask = torch.tensor([True, False], device="cuda")
    n = tr.arena.n_trainable
    tr.forward_backward(images, eps, noise, t, None, None, label, mask)
    got = tr.loss.clone(), tr.arena.grad[:n].clone()
    zeroed = label.clone()
    zeroed[0] = 0.0
    tr.forward_backward(images, eps, noise, t, None, None, zeroed)
    assert torch.equal(got[0], tr.loss) and torch.allclose(got[1], tr.arena.grad[:n], rtol=1e-5)
    tr.forward_backward(images, eps, noise, t, None, None, label)
    assert not torch.equal(got[0], tr.loss)  # the mask matters
    with pytest.raises(ValueError, match="drop"):
        tr.forward_backward(images, eps, noise, t, None, None, label, torch.zeros(3, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="drop"):
        tr.validate(images, eps, noise, t, None, None, label, mask.float())


def test_trainer_refuses_bad_masks():
    from medical_image_generation_amd.trainer import DDPMTrainer, draw_drop
    from medical_image_generation_amd.unet import DiffusionModelUNet
    inputs, tr = _step_inputs("class"), _trainer("class")
    before = tr.arena.data.clone()
    for bad in (torch.zeros(2, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"),  # dtype
                torch.zeros(3, dtype=torch.bool, device="cuda"), torch.zeros(2, 1, dtype=torch.bool, device="cuda"),  # shape
                torch.zeros(2, dtype=torch.bool), [True, False]):  # device, not a tensor
        with pytest.raises(ValueError, match="drop"):
            tr.step(*inputs, bad)
        with pytest.raises(ValueError, match="drop"):
            tr.validate(*inputs, bad)
    assert torch.equal(tr.arena.data, before)
    mask = draw_drop(2, 0.5, generator=torch.Generator("cuda").manual_seed(1))
    assert mask.is_cuda and mask.dtype == torch.bool and mask.shape == (2,)
    no_null = DDPMTrainer(_product_net("class"), lr=cases.STEP_LR)
    with pytest.raises(ValueError, match="null_class"):
        no_null.step(*inputs, mask)
    for bad in (-1, 4):
        with pytest.raises(ValueError, match="null_class"):
            DDPMTrainer(_product_net("class"), null_class=bad)
    with pytest.raises(ValueError, match="null_class"):
        DDPMTrainer(_product_net("xattn"), null_class=0)
    c = cases.UNET_CASES["unet2d_updown"]
    plain = DDPMTrainer(DiffusionModelUNet(**c["kwargs"]).cuda(), lr=cases.STEP_LR)
    x0 = synth.tensor(S, "cfg_x0", c["shape"]).cuda()
    with pytest.raises(ValueError, match="no conditioning"):
        plain.step(x0, x0.clone(), torch.tensor(c["timesteps"], device="cuda"), None, None, None, mask)


# ---------------------------------------------------------------------------------------------------------------- sampling
@functools.lru_cache(maxsize=None)
def _sampler(route):
    """-> (net, scheduler, inferer, the route's sample() keywords without the guidance scale)."""
    from medical_image_generation_amd.inferer import DDIMScheduler, DiffusionInferer
    cond = G.case(route)[4]
    sch = DDIMScheduler(1000, **G.GENTLE)
    sch.set_timesteps(G.STEPS)
    if route == "class":
        kw = dict(class_labels=cond["labels"].cuda())
    elif route == "xattn":
        kw = dict(conditioning=cond["context"].cuda())
    else:
        kw = dict(conditioning=cond["cond"].cuda(), mode="concat")
    return _product_net(route).eval(), sch, DiffusionInferer(sch), kw


def _null_kw(route):
    return dict(null_class=G.NULL_CLASS) if route == "class" else {}


def test_class_labels_reach_the_model():
    """(a) unet2d_class with class_labels only: the conditional-only oracle loop, graph off and on, within the unguided BOUND."""
    net, sch, inf, kw = _sampler("class")
    x0, want = G.start("class"), G.wants("class")["cond"]
    for graph in (False, True):
        got = inf.sample(x0.cuda(), net, sch, verbose=False, use_graph=graph, **kw)
        assert torch.isfinite(got).all()
        err = G.rel(got.cpu(), want)
        print(f"\n[class labels only, graph={graph}] rel-L2: {err:.3e}")
        assert err <= G.BOUND
    assert G.rel(G.wants("class")["uncond"], want) > G.BOUND  # the labels matter
    with pytest.raises(ValueError, match="class_labels"):
        inf.sample(x0.cuda(), net, sch, verbose=False)  # a class-conditional net needs its labels
    with pytest.raises(ValueError, match="class_labels"):
        inf.sample(x0.cuda(), net, sch, verbose=False, class_labels=torch.tensor([1, 4]))  # out of the table
    with pytest.raises(ValueError, match="class_labels"):
        inf.sample(x0.cuda(), net, sch, verbose=False, class_labels=torch.tensor([1]))


@pytest.mark.parametrize("route", G.ROUTES)
def test_guided_sample_loop_matches_the_two_pass_oracle_loop(route):
    """(b) 4 eta-0 DDIM steps at w = W[route], graph off and on, against two fp32 oracle forwards per step with the fp64 update; then
    (c) on the same inferer w = 0: the same loop object and captured graph, and the oracle's unconditional loop (null labels / zeros).

    Bound: max(BOUND, 2 x drift), drift = the guided oracle loop in fp32 against itself with both model outputs rounded to bf16,
    measured on the CPU (tests/guidance_ref.py, printed by tests/test_guidance_cpu.py): class (w = 4) 4.6e-3, xattn (w = 2) 1.5e-3,
    concat (w = 2) 1.8e-3 -- twice that is below BOUND on every route, so the bound is BOUND = 3e-2.  The guided trajectory ends
    0.167 / 0.256 / 0.162 from the conditional-only one and 0.215 / 0.474 / 0.313 from the unconditional one, so neither a wrong branch
    order nor a missing branch fits."""
    net, sch, inf, kw = _sampler(route)
    x0, want, bound = G.start(route), G.wants(route), G.bound(route)
    for graph in (False, True):
        got = inf.sample(x0.cuda(), net, sch, verbose=False, use_graph=graph, guidance_scale=G.W[route], **kw, **_null_kw(route))
        assert got.shape == x0.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
        err = G.rel(got.cpu(), want["guided"])
        print(f"\n[{route} guided w={G.W[route]} graph={graph}] rel-L2: {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    guided = [l for l in inf._loops.values() if l.guided]
    assert len(guided) == 1 and guided[0].graph is not None
    loop, captured = guided[0], guided[0].graph
    got = inf.sample(x0.cuda(), net, sch, verbose=False, guidance_scale=0.0, **kw, **_null_kw(route))
    assert [l for l in inf._loops.values() if l.guided] == [loop] and loop.graph is captured  # the scale is not part of the graph
    err = G.rel(got.cpu(), want["uncond"])
    print(f"\n[{route} w=0 on the graph of w={G.W[route]}] rel-L2 against the unconditional loop: {err:.3e}")
    assert err <= bound


def test_invert_with_class_labels_matches_oracle():
    """(d) image -> noise with the labels at every step."""
    net, sch, inf, kw = _sampler("class")
    _, _, ref, shape, cond = G.case("class")
    image = synth.tensor(S, "invert_image", shape).clamp(-1, 1)
    want = G.loop(ref, image, cond, reverse=True)
    got = inf.invert(image.cuda(), net, **kw)
    err = G.rel(got.cpu(), want)
    print(f"\n[ddim invert with class labels] rel-L2: {err:.3e}")
    assert got.shape == image.shape and err <= G.BOUND
    assert G.rel(G.loop(ref, image, G.null_of(cond), reverse=True), want) > G.BOUND / 10  # the labels move the inversion


def test_guidance_refusals():
    from medical_image_generation_amd.unet import DiffusionModelUNet
    net, sch, inf, kw = _sampler("class")
    x0 = G.start("class").cuda()
    with pytest.raises(ValueError, match="null_class"):
        inf.sample(x0, net, sch, verbose=False, guidance_scale=2.0, **kw)
    for bad in (-1, 4):
        with pytest.raises(ValueError, match="null_class"):
            inf.sample(x0, net, sch, verbose=False, guidance_scale=2.0, null_class=bad, **kw)
    c = cases.UNET_CASES["unet2d_updown"]
    plain = DiffusionModelUNet(**c["kwargs"]).cuda().eval()
    with pytest.raises(ValueError, match="guidance_scale"):
        inf.sample(torch.zeros(c["shape"], device="cuda"), plain, sch, verbose=False, guidance_scale=2.0)
    with pytest.raises(ValueError, match="class_labels"):
        inf.sample(torch.zeros(c["shape"], device="cuda"), plain, sch, verbose=False, class_labels=torch.tensor([0, 1]))


def test_latent_inferer_decodes_the_guided_sample():
    """(e) LatentDiffusionInferer.sample(guidance_scale=) = decode(latents / scale) of DiffusionInferer's guided sample, bit for bit."""
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    from medical_image_generation_amd.inferer import DiffusionInferer, LatentDiffusionInferer
    ae = AutoencoderKL(**cases.AEKL_CASES["aekl_c3a"]["kwargs"])
    ae.load_state_dict(synth.state_dict({k: tuple(v.shape) for k, v in ae.state_dict().items()}, S))
    ae = ae.cuda().eval()
    net, sch, _, _ = _sampler("concat")
    z = synth.tensor(S, "latent_noise", (1, 8, 8, 8, 8)).cuda()
    label = G.case("concat")[4]["cond"][:1].cuda()
    scale = 0.7
    kw = dict(conditioning=label, mode="concat", verbose=False, guidance_scale=2.0)
    lat = DiffusionInferer(sch).sample(z, net, sch, **kw)
    img = LatentDiffusionInferer(sch, scale_factor=scale).sample(z, ae, net, sch, **kw)
    with torch.no_grad():
        want = ae.decode_stage_2_outputs(lat / scale)
    assert img.shape == (1, 1, 32, 32, 32) and torch.isfinite(img).all() and torch.equal(img, want)
    plain = DiffusionInferer(sch).sample(z, net, sch, conditioning=label, mode="concat", verbose=False)
    assert not torch.equal(plain, lat)
