"""Host side of the validation passes (trainer.ValidationMeter / kl_weight_from_mean / validate): the meter's global mean over a
2-rank gloo group, the decade rule of adapt_kl_loss_weight (train_autoencoder.py:319-327) and the no-CPU-fallback error."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import cases


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


_RANK_LOSSES = {0: [0.5, 0.25, 1.0], 1: [2.0]}  # different sums AND different counts


def _worker(rank, world, port, out):
    from medical_image_generation_amd.trainer import ValidationMeter
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = ValidationMeter("cpu")
        for v in _RANK_LOSSES[rank]:
            m.add(v)
        first = m.mean()
        second = m.mean()  # the all-reduce works on a copy: asking twice does not double the sums
        m.reset()
        if rank == 0:
            m.add(3.0)  # rank 1 stays empty: the global mean is still defined
        out[rank] = (first, second, float(m.last), m.mean())
    finally:
        dist.destroy_process_group()


def test_meter_mean_is_global_over_two_gloo_ranks():
    world, port = 2, _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    want = sum(sum(v) for v in _RANK_LOSSES.values()) / sum(len(v) for v in _RANK_LOSSES.values())
    for rank in range(world):
        first, second, last, after = out[rank]
        assert first == pytest.approx(want, rel=1e-12) and second == first
        assert after == 3.0
    assert out[0][2] == 3.0 and out[1][2] == 0.0
    assert out[0][0] != sum(_RANK_LOSSES[0]) / len(_RANK_LOSSES[0])  # not the local mean


def test_meter_single_process():
    from medical_image_generation_amd.trainer import ValidationMeter
    m = ValidationMeter("cpu")
    with pytest.raises(ValueError):
        m.mean()
    m.add(1.5), m.add(torch.tensor(2.5))
    assert m.mean() == 2.0 and float(m.last) == 2.5
    m.reset()
    assert float(m.acc.abs().sum()) == 0.0
    with pytest.raises(ValueError):
        m.mean()


def test_kl_weight_from_mean_decade_rule():
    """Worked from train_autoencoder.py:319-327: exponent = floor(log10(kl)); kl_weight = 0.001 / 10 ** exponent."""
    from medical_image_generation_amd.trainer import kl_weight_from_mean
    assert kl_weight_from_mean(3.7e3) == pytest.approx(1e-6, rel=1e-12)
    assert kl_weight_from_mean(0.42) == pytest.approx(1e-2, rel=1e-12)
    assert kl_weight_from_mean(1.0) == pytest.approx(1e-3, rel=1e-12)
    assert kl_weight_from_mean(9.99) == pytest.approx(1e-3, rel=1e-12) and kl_weight_from_mean(10.0) == pytest.approx(1e-4, rel=1e-12)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            kl_weight_from_mean(bad)


def test_validate_has_no_cpu_fallback():
    """CPU inputs are refused by validate() with the error step() gives them: there is no CPU path to fall back to."""
    from medical_image_generation_amd.autoencoderkl import AutoencoderKL
    from medical_image_generation_amd.trainer import AETrainer, DDPMTrainer
    from medical_image_generation_amd.unet import DiffusionModelUNet
    c = cases.UNET_CASES["unet3d"]
    tr = DDPMTrainer(DiffusionModelUNet(**c["kwargs"]), device="cpu")
    x, t = torch.zeros(c["shape"]), torch.zeros(c["shape"][0], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="must live on the GPU") as e_step:
        tr.step(x, x, t)
    with pytest.raises(RuntimeError, match="must live on the GPU") as e_val:
        tr.validate(x, x, t)
    assert str(e_val.value) == str(e_step.value)
    with pytest.raises(RuntimeError, match="capture_validate"):
        tr.validate_graph()
    ca = cases.AEKL_CASES["aekl_attn"]
    ta = AETrainer(AutoencoderKL(**ca["kwargs"]), device="cpu")
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ta.validate(torch.zeros(ca["shape"]), torch.zeros(2, 4, 8, 8, 4))
