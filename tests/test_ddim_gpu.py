"""DDIM few-step sampling and inversion on the HIP path (inferer.DDIMScheduler, `mi_diffusion_step` with ddim = 1) against the fp64 restatement in
tests/ddim_ref.py (third-party closed form, PARITY UNPINNED -- see its docstring): the fused update kernel per row, and the whole loop
(UNet forward + update, hipGraph-replayed) against the same loop on the oracle's fp32 UNet.

The loop tests use DDIMScheduler(1000, "linear_beta", beta_start=1e-4, beta_end=2e-3), not the training schedule: under
scaled_linear 0.0015..0.0205 five eta-0 steps turn a 1e-2 relative error of the bf16 forward into 6.6e-2 (x0 = (x - r1 m) / r0 with
r0 down to 0.02), so a trajectory comparison there shows nothing; under the gentle schedule the same error ends at about 0.5e-2
(sampling) and 1.2e-2 (inversion), while a wrong previous-level index moves r2 by about 10 %."""
import functools

import pytest
import torch

from oracle import cases, nets, synth
from tests import ddim_ref

pytestmark = pytest.mark.gpu
S = cases.SEED
TRAIN = dict(schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205)
GENTLE = dict(schedule="linear_beta", beta_start=1e-4, beta_end=2e-3)
BOUND = 3e-2  # rel-L2 budget of this net's bf16 forward over a few steps (tests/test_inferer_gpu.py::test_sample_loop_matches_oracle)
N_INVERT = 5


def test_ddim_step_kernel_matches_closed_form():
    """Shape (2, 3, 4, 6, 5): V = 120 is no multiple of the wave or the block.  The kernel reads the product's fp32 rows; the expected
    values come from the restatement's fp64 rows.  Bounds as for the DDPM form: fp32 x 1e-5 max(1, max|want|), bf16 copy 1e-2 max|want|."""
    from medical_image_generation_amd import hipops as ops
    from medical_image_generation_amd._lib import call, ptr
    from medical_image_generation_amd.inferer import DDIMScheduler
    shape, n = (2, 3, 4, 6, 5), 10
    N, C, V = shape[0], shape[1], 4 * 6 * 5
    acp, _ = ddim_ref.alphas_cumprod(1000, **TRAIN)
    x, z = synth.tensor(S, "ddim_x", shape) * 1.5, synth.tensor(S, "ddim_z", shape)
    mo = synth.tensor(S, "ddim_m", shape).bfloat16().float()  # the model output is bf16
    mo_cl, zd = ops.to_channels_last(mo.cuda()), z.cuda()
    sentinel = synth.tensor(S, "ddim_cond", (N, 4, 6, 5, 2)).bfloat16().cuda()
    idx = torch.zeros(1, dtype=torch.int64, device="cuda")
    worst = [0.0, 0.0]
    for pred in ("epsilon", "v_prediction"):
        for clip in (True, False):
            sch = DDIMScheduler(prediction_type=pred, clip_sample=clip, **TRAIN)
            sch.set_timesteps(n)
            flags = int(clip) | (2 if pred == "v_prediction" else 0)
            for eta, reverse in ((0.0, False), (0.5, False), (0.0, True)):
                table = sch.rows(eta, reverse).cuda()
                want_rows = ddim_ref.rows(acp, n, eta, reverse=reverse)
                for i in (0, 5, n - 1):  # first, middle, last: p < 0 (denoising: ap = 1), p >= T (inversion: ap = 0)
                    want, _ = ddim_ref.update(want_rows[i], x, mo, z, prediction_type=pred, clip_sample=clip)
                    idx.fill_(i)
                    tol = 1e-5 * max(1.0, float(want.abs().max()))
                    for cs in (C, C + 2, 0):
                        xd = x.cuda()
                        x_cl = None
                        if cs:
                            x_cl = torch.zeros((N, 4, 6, 5, cs), dtype=torch.bfloat16, device="cuda")
                            x_cl[..., C:] = sentinel[..., :cs - C]
                        call("mi_diffusion_step", ptr(xd), ptr(mo_cl), ptr(zd), ptr(table), ptr(idx), None, None, None, None, None, ptr(x_cl), cs, N, C, V,
                             flags, 1)
                        err = float((xd.cpu().double() - want).abs().max())
                        worst[0] = max(worst[0], err / tol)
                        assert err <= tol, (pred, clip, eta, reverse, i, cs, err, tol)
                        if cs:
                            got_cl = ops.to_channels_first(x_cl[..., :C].contiguous()).cpu().double()
                            err_cl = float((got_cl - want).abs().max())
                            worst[1] = max(worst[1], err_cl / (1e-2 * float(want.abs().max())))
                            assert err_cl <= 1e-2 * float(want.abs().max()), (pred, clip, eta, reverse, i, cs, err_cl)
                            assert torch.equal(x_cl[..., C:].view(torch.int16), sentinel[..., :cs - C].view(torch.int16))  # the condition stays
    print(f"\n[mi_diffusion_step ddim] worst error / bound: fp32 {worst[0]:.3f}, bf16 copy {worst[1]:.3f}")
    assert ddim_ref.rows(acp, n, 0.5)[5, 4] > 0 and ddim_ref.rows(acp, n, reverse=True)[n - 1, 2] == 0  # the rows are the ones meant


def test_ddim_step_kernel_refuses_bad_arguments():
    from medical_image_generation_amd._lib import HipError, call, ptr
    x = torch.zeros(2, 3, 120, device="cuda")
    mo = torch.zeros(2, 120, 3, dtype=torch.bfloat16, device="cuda")
    x_cl = torch.zeros(2, 120, 3, dtype=torch.bfloat16, device="cuda")
    rows = torch.ones(4, 5, device="cuda")
    idx = torch.zeros(1, dtype=torch.int64, device="cuda")
    for ddim in (1, 0):  # the plain step of either form: no guidance, no known region
        good = [ptr(x), ptr(mo), ptr(x), ptr(rows), ptr(idx), None, None, None, None, None, ptr(x_cl), 3, 2, 3, 120, 1, ddim]
        for k in range(5):  # x, model_out, noise, rows, row_index
            with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
                call("mi_diffusion_step", *(good[:k] + [None] + good[k + 1:]))
        for k, v in ((11, 2), (12, 0), (13, 0), (14, 0), (12, -1), (14, -5)):  # x_cl pitch below C; non-positive N, C, V
            with pytest.raises(HipError, match="MI_ERR_BAD_ARG"):
                call("mi_diffusion_step", *(good[:k] + [v] + good[k + 1:]))
        call("mi_diffusion_step", *good)  # (the unchanged arguments are accepted)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _nets(name, in_channels=None, out_channels=None):
    from medical_image_generation_amd.unet import DiffusionModelUNet
    kw = dict(cases.UNET_CASES[name]["kwargs"])
    if in_channels:
        kw.update(in_channels=in_channels, out_channels=out_channels)
    ref = nets.DiffusionModelUNet(**kw)
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    ref.load_state_dict(sd)
    net = DiffusionModelUNet(**kw)
    net.load_state_dict(sd)
    return ref.eval(), net.cuda().eval()


def _oracle_loop(ref, x, n, eta=0.0, steps_offset=0, reverse=False, zs=None, cond=None):
    """The loop of the inferer on the oracle's fp32 UNet, the update in fp64 (tests/ddim_ref.py)."""
    acp, _ = ddim_ref.alphas_cumprod(1000, **GENTLE)
    ts = ddim_ref.timesteps(1000, n, steps_offset)
    rows = ddim_ref.rows(acp, n, eta, steps_offset, reverse=reverse)
    with torch.no_grad():
        for i, t in enumerate(ts[::-1] if reverse else ts):
            inp = x if cond is None else torch.cat([x, cond], dim=1)
            mo = ref(inp, torch.full((x.shape[0],), t, dtype=torch.int64))
            x = ddim_ref.update(rows[i], x, mo, None if zs is None else zs[i], clip_sample=True)[0].float()
    return x


def _rel(got, want):
    assert torch.isfinite(got).all()
    return float((got.cpu() - want).norm() / want.norm())


def test_sample_loop_matches_oracle_and_reuses_its_graph():
    """(a) n = 5, eta = 0, graph off and on; then (b) on the same inferer and scheduler n = 4, eta = 0.5, steps_offset = 1 with pinned
    noises: the graph captured in (a) is replayed over a refilled row table (a stale table would give (a)'s rows)."""
    from medical_image_generation_amd.inferer import DDIMScheduler, DiffusionInferer
    ref, net = _nets("unet3d")
    shape = cases.UNET_CASES["unet3d"]["shape"]
    x0 = synth.tensor(S, "sample_noise", shape)
    sch = DDIMScheduler(1000, **GENTLE)
    sch.set_timesteps(5)
    inf = DiffusionInferer(sch)
    want = _oracle_loop(ref, x0, 5)
    errs = {}
    for graph in (False, True):
        errs[graph] = _rel(inf.sample(x0.cuda(), net, sch, verbose=False, use_graph=graph), want)
        print(f"\n[ddim sample n=5 eta=0 graph={graph}] rel-L2: {errs[graph]:.3e}")
    (loop,) = inf._loops.values()
    captured = loop.graph
    assert captured is not None
    sch.steps_offset = 1
    sch.set_timesteps(4)
    assert sch.timesteps.tolist() == [751, 501, 251, 1]
    zs = [synth.tensor(S, f"sample_z{i}", shape) for i in range(4)]
    want_b = _oracle_loop(ref, x0, 4, eta=0.5, steps_offset=1, zs=zs)
    err_b = _rel(inf.sample(x0.cuda(), net, sch, verbose=False, noises=[z.cuda() for z in zs], eta=0.5), want_b)
    print(f"\n[ddim sample n=4 eta=0.5 offset=1, graph of the n=5 run] rel-L2: {err_b:.3e}")
    assert len(inf._loops) == 1 and loop.graph is captured
    # the two runs end far apart (0.32 on the oracle; (b)'s steps over (a)'s rows end 0.32 from (b) as well): stale rows cannot pass
    assert float((want_b - want).norm() / want.norm()) > 5 * BOUND
    assert errs[False] <= BOUND and errs[True] <= BOUND and err_b <= BOUND


def _invert_errors(n):
    from medical_image_generation_amd.inferer import DDIMScheduler, DiffusionInferer
    ref, net = _nets("unet3d")
    image = synth.tensor(S, "invert_image", cases.UNET_CASES["unet3d"]["shape"]).clamp(-1, 1)
    sch = DDIMScheduler(1000, **GENTLE)
    sch.set_timesteps(n)
    inf = DiffusionInferer(sch)
    want = _oracle_loop(ref, image, n, reverse=True)
    errs = []
    for graph in (False, True):
        got = inf.invert(image.cuda(), net, use_graph=graph)
        assert got.dtype == torch.float32 and got.shape == image.shape
        errs.append(_rel(got, want))
        print(f"\n[ddim invert n={n} graph={graph}] rel-L2: {errs[-1]:.3e}")
    assert float((want - image).norm() / image.norm()) > 0.5  # the inversion went somewhere: the last row lands on the model's noise
    return errs


def test_invert_loop_matches_oracle():
    """(c) image -> noise over ascending timesteps with the reverse rows (first, middle and last row replayed), graph off and on."""
    errs = _invert_errors(N_INVERT)
    assert max(errs) <= BOUND


def test_sample_loop_with_concat_conditioning_matches_oracle():
    """(d) mode="concat" on the net of tests/test_inferer_gpu.py's concat test: the kernel rewrites the 8 sample channels of the
    9-channel model input and leaves the label channel."""
    from medical_image_generation_amd.inferer import DDIMScheduler, DiffusionInferer
    ref, net = _nets("unet_ldm", 9, 8)
    shape = (2, 8, 8, 8, 8)
    x0 = synth.tensor(S, "sample_noise", shape)
    label = (synth.ellipsoid_volume(S, "label", (2, 1, 8, 8, 8)) > 0).float()
    sch = DDIMScheduler(1000, **GENTLE)
    sch.set_timesteps(4)
    want = _oracle_loop(ref, x0, 4, cond=label)
    got = DiffusionInferer(sch).sample(x0.cuda(), net, sch, conditioning=label.cuda(), mode="concat", verbose=False)
    err = _rel(got, want)
    print(f"\n[ddim concat-conditioned sample n=4 eta=0 graph=True] rel-L2: {err:.3e}")
    assert got.shape == shape and err <= BOUND


def test_latent_inferer_samples_and_inverts_through_the_autoencoder():
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    from medical_image_generation_amd.inferer import DDIMScheduler, DDPMScheduler, DiffusionInferer, LatentDiffusionInferer
    from medical_image_generation_amd.unet import DiffusionModelUNet
    ae = AutoencoderKL(**cases.AEKL_CASES["aekl_c3a"]["kwargs"])
    ae.load_state_dict(synth.state_dict({k: tuple(v.shape) for k, v in ae.state_dict().items()}, S))
    ae = ae.cuda().eval()
    kw = dict(spatial_dims=3, in_channels=8, out_channels=8, num_res_blocks=1, num_channels=(32, 64), attention_levels=(False, True),
              num_head_channels=(0, 32), norm_num_groups=16, strides=[[1] * 3, [2] * 3], kernel_sizes=[[3] * 3] * 2, paddings=[[1] * 3] * 2)
    net = DiffusionModelUNet(**kw)
    net.load_state_dict(synth.state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, S))
    net = net.cuda().eval()
    sch = DDIMScheduler(1000, **GENTLE)
    sch.set_timesteps(4)
    z = synth.tensor(S, "latent_noise", (1, 8, 8, 8, 8)).cuda()
    zs = [synth.tensor(S, f"latent_z{i}", (1, 8, 8, 8, 8)).cuda() for i in range(4)]
    scale = 0.7
    plain, latent = DiffusionInferer(sch), LatentDiffusionInferer(sch, scale_factor=scale)
    for eta in (0.0, 0.5):
        lat = plain.sample(z, net, sch, verbose=False, noises=zs, eta=eta)
        img = latent.sample(z, ae, net, sch, verbose=False, noises=zs, eta=eta)
        with torch.no_grad():
            want = ae.decode_stage_2_outputs(lat / scale)
        assert img.shape == (1, 1, 32, 32, 32) and torch.isfinite(img).all() and torch.equal(img, want)
    image = synth.tensor(S, "invert_image", (1, 1, 32, 32, 32)).clamp(-1, 1).cuda()
    torch.manual_seed(S)  # encode_stage_2_inputs draws the latent's eps
    with torch.no_grad():
        enc = ae.encode_stage_2_inputs(image) * scale
    want = plain.invert(enc, net)
    torch.manual_seed(S)
    got = latent.invert(image, ae, net)
    assert got.shape == (1, 8, 8, 8, 8) and got.dtype == torch.float32 and torch.isfinite(got).all() and torch.equal(got, want)
    with pytest.raises(TypeError, match="DDIMScheduler"):
        latent.invert(image, ae, net, scheduler=DDPMScheduler())
    with pytest.raises(TypeError, match="DDIMScheduler"):
        DiffusionInferer(DDPMScheduler()).invert(enc, net)
