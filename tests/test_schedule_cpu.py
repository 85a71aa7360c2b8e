"""Training (trainer.DDPMSchedule) and sampling (inferer.DDPMScheduler) take their betas from ONE function, inferer.betas: the two
classes agree bit for bit on the CPU and with the oracle's own restatement (oracle/step.py)."""
import pytest
import torch

from oracle import step

ARGS = dict(num_train_timesteps=250, beta_start=0.0005, beta_end=0.0195)  # none of them a default of either class (train_ddpm.py:381)


@pytest.mark.parametrize("schedule", ["scaled_linear_beta", "linear_beta"])
def test_train_and_sampling_schedules_are_one(schedule):
    """Bit equality is asserted on what DDPMSchedule keeps, sqrt(alphas_cumprod) and sqrt(1 - alphas_cumprod): torch.sqrt is correctly
    rounded, so equal alphas_cumprod give equal roots, while squaring the stored root does not return fp32 alphas_cumprod (it misses
    about half of the 250 entries by one ulp, for either class's own values)."""
    from medical_image_generation_amd.inferer import DDPMScheduler, betas
    from medical_image_generation_amd.trainer import DDPMSchedule
    train = DDPMSchedule(schedule=schedule, device="cpu", **ARGS)
    sample = DDPMScheduler(schedule=schedule, **ARGS)
    assert torch.equal(sample.betas, betas(schedule, **ARGS))
    assert torch.equal(train.sqrt_acp, sample.alphas_cumprod.sqrt())
    assert torch.equal(train.sqrt_1macp, (1.0 - sample.alphas_cumprod).sqrt())
    ref = step.DDPMSchedule(schedule=schedule, **ARGS)
    assert torch.allclose(sample.alphas_cumprod, ref.alphas_cumprod, rtol=1e-6, atol=1e-7)
    assert torch.allclose(train.sqrt_acp ** 2, ref.alphas_cumprod, rtol=1e-6, atol=1e-7)
    assert torch.allclose(sample._coef, ref.step_coefficients(), rtol=1e-6, atol=1e-7)  # (tests/test_inferer_gpu.py's check and bound)


def test_unknown_schedule_is_refused_by_both():
    from medical_image_generation_amd.inferer import DDPMScheduler
    from medical_image_generation_amd.trainer import DDPMSchedule
    with pytest.raises(ValueError, match="unknown schedule cosine"):
        DDPMSchedule(schedule="cosine", device="cpu")
    with pytest.raises(ValueError, match="unknown schedule cosine"):
        DDPMScheduler(schedule="cosine")
    # each class raises its errors in its own order: the trainer's names the schedule first, the sampler's the prediction type
    with pytest.raises(ValueError, match="unknown schedule"):
        DDPMSchedule(schedule="cosine", prediction_type="sample", device="cpu")
    with pytest.raises(ValueError, match="unknown prediction_type"):
        DDPMScheduler(schedule="cosine", prediction_type="sample")
