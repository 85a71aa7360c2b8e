"""The fp64 restatement of tiled diffusion sampling (tests/tiled_sampling_ref.py) against what it must reduce to, and the window-plan
facts the GPU tests (tests/test_tiled_sampling_gpu.py) rely on.  No GPU."""

import pytest
import torch

from oracle import cases, step
from tests import abi_header, ddim_ref
from tests import sliding_ref as R
from tests import tiled_sampling_ref as T

S = cases.SEED


def _dyadic(name, shape, scale=16):
    return torch.randint(-32, 33, shape, generator=torch.Generator().manual_seed(S + len(name))).float() / scale


def _smooth_model(inp, t, n, null):
    """Any deterministic model: depends on the input, the timestep, the image and the branch."""
    c = inp.shape[1]
    return torch.tanh(inp[:, :1] * 0.5 + inp[:, c - 1:] * 0.25) + 1e-3 * t + 0.1 * n - (0.2 if null else 0.0)


def _ddim_update(rows, prediction_type="epsilon"):
    return lambda i, t, x, m, z: ddim_ref.update(rows[i], x, m, z, prediction_type, True)[0]


def _ddpm_update(sch):
    return lambda i, t, x, m, z: sch.step(m, t, x, z.double() if z is not None else None, clip_sample=True)[0]


@pytest.mark.parametrize("kind", ["ddim", "ddim_eta", "ddpm"])
def test_one_window_is_the_plain_loop(kind):
    """One window equal to the case, mode="constant": acc = 1 * p, wsum = 1, m = p exactly, so the restatement is the plain loop."""
    shape = (2, 1, 6, 10)
    x0 = _dyadic("x0", shape)
    steps = 4
    ts = ddim_ref.timesteps(1000, steps)
    zs = [_dyadic(f"z{i}", shape) for i in range(steps)]
    if kind == "ddpm":
        update = _ddpm_update(step.DDPMSchedule())
    else:
        acp, _ = ddim_ref.alphas_cumprod()
        update = _ddim_update(ddim_ref.rows(acp, steps, 0.5 if kind == "ddim_eta" else 0.0))
    noises = None if kind == "ddim" else zs
    got = T.sample(x0, _smooth_model, ts, update, (6, 10), 0.5, "constant", noises=noises)
    x = x0.double()
    for i, t in enumerate(ts):
        m = torch.cat([_smooth_model(x[n:n + 1].float(), t, n, False) for n in range(2)]).double()
        x = update(i, t, x, m, None if noises is None else noises[i]).double()
    assert torch.equal(got, x)
    # guided: the combination of guidance_ref, per window
    got = T.sample(x0, _smooth_model, ts[:1], update, (6, 10), 0.5, "constant", w=2.0, noises=noises)
    x = x0.double()
    mc = torch.cat([_smooth_model(x[n:n + 1].float(), ts[0], n, False) for n in range(2)]).double()
    mu = torch.cat([_smooth_model(x[n:n + 1].float(), ts[0], n, True) for n in range(2)]).double()
    assert torch.equal(got, update(0, ts[0], x, mu + 2.0 * (mc - mu), None if noises is None else noises[0]).double())


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_two_windows_by_hand(mode):
    """A window-varying model p = tile * r + s (dyadic: the windows disagree on the voxels they share) on a 2-D case (8, 12) under
    windows (8, 8) at overlap 0.5: origins (0, 0) and (0, 4).  The condition varies along W, and the null branch drops it."""
    g = torch.Generator().manual_seed(S)
    r, s = torch.randint(-8, 9, (8, 8), generator=g).float() / 8, torch.randint(-8, 9, (8, 8), generator=g).float() / 4
    x, cond = _dyadic("x", (1, 1, 8, 12)), _dyadic("cond", (1, 1, 8, 12), 8)

    def model(inp, t, n, null):
        return inp[:, :1] * r + s + inp[:, 1:] * 0.5

    roi, wins = T.windows((8, 12), 8, 0.5)
    assert roi == (8, 8) and wins == [(0, 0), (0, 4)]
    imp = R.importance((8, 8), mode).float().double()
    for w in (None, 3.0):
        m, bound = T.blended_prediction(x, model, 500, 8, 0.5, mode, cond=cond, w=w)
        acc, wsum = torch.zeros(1, 1, 8, 12, dtype=torch.float64), torch.zeros(8, 12, dtype=torch.float64)
        for o in (0, 4):
            tile, c = x[..., o:o + 8], cond[..., o:o + 8]
            p = (tile * r + s + c * 0.5).double()
            if w is not None:
                pu = (tile * r + s).double()
                p = pu + w * (p - pu)
            acc[..., o:o + 8] += imp * p
            wsum[:, o:o + 8] += imp
        assert torch.equal(m, acc / wsum)
        assert bool((bound >= 0).all()) and bound.shape == m.shape
    acp, _ = ddim_ref.alphas_cumprod()
    rows = ddim_ref.rows(acp, 2)
    got = T.sample(x, model, ddim_ref.timesteps(1000, 2)[:1], _ddim_update(rows), 8, 0.5, mode, cond=cond)
    m, _ = T.blended_prediction(x, model, ddim_ref.timesteps(1000, 2)[0], 8, 0.5, mode, cond=cond)
    assert torch.equal(got, ddim_ref.update(rows[0], x, m, None)[0])


def test_a_case_smaller_than_the_window_is_refused():
    with pytest.raises(ValueError, match="smaller"):
        T.windows((8, 12), (8, 16), 0.5)


def test_plan_facts_of_the_gpu_tests():
    from medical_image_generation_amd.sliding import WindowPlan
    # several windows against the oracle: 4 windows per image; batch 3 -> 3 calls, the second mixes both images, the last ends in one filler
    plan = WindowPlan((16, 24, 24), 16, 0.5)
    assert plan.starts == [[0], [0, 8], [0, 8]] and plan.num_windows == 4 and plan.padded == (16, 24, 24)
    assert T.windows((16, 24, 24), 16, 0.5) == ((16, 16, 16), plan.windows)
    rows = plan.rows(2, 3)
    assert rows.shape == (3, 3, 4)
    assert rows[:, :, 0].tolist() == [[0, 0, 0], [0, 1, 1], [1, 1, -1]]
    # one window: the plain sampler
    assert WindowPlan((16, 16, 16), 16, 0.25).windows == [(0, 0, 0)]
    assert WindowPlan((16, 16), 16, 0.25).windows == [(0, 0)]
    # concat conditioning: 2 windows along W
    assert WindowPlan((8, 8, 12), 8, 0.5).windows == [(0, 0, 0), (0, 0, 4)]
    # 2-D with labels: 2 windows per image, batch 3: the first call mixes the images
    plan = WindowPlan((16, 24), 16, 0.5)
    assert plan.windows == [(0, 0), (0, 8)]
    assert plan.rows(2, 3)[:, :, 0].tolist() == [[0, 0, 1], [1, -1, -1]]
    # the latent pair: 8^3 latent under 4^3 windows
    assert WindowPlan((8, 8, 8), 4, 0.5).num_windows == 27
    # kernel shapes: both access paths
    assert WindowPlan((6, 9, 16), (4, 5, 8), 0.5).padded == (6, 9, 16) and WindowPlan((6, 9, 23), (4, 5, 7), 0.5).padded == (6, 9, 23)


def test_binding_and_header_agree_on_the_new_entry_points():
    import ctypes

    from medical_image_generation_amd import _lib
    lib = _lib.load()
    for name in ("mi_sw_gather_cl", "mi_sw_accumulate_cl", "mi_sw_diffusion_step"):
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
        assert len(abi_header.params(name)) == len(_lib.signature(name)[1]), name
    assert _lib.signature("mi_sw_accumulate_cl")[1][1] is ctypes.c_void_p  # the guidance scale is a device pointer


def test_public_surface_takes_the_keyword():
    import inspect

    from medical_image_generation_amd.inferer import DiffusionInferer, LatentDiffusionInferer
    for cls in (DiffusionInferer, LatentDiffusionInferer):
        for name in ("sample", "invert"):
            assert inspect.signature(getattr(cls, name)).parameters["window_inferer"].default is None, (cls, name)
    for name in ("img2img", "inpaint"):
        assert inspect.signature(getattr(DiffusionInferer, name)).parameters["window_inferer"].default is None, name
