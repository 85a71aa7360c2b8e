"""Averaged weights, the part that needs no GPU: the two entry points are declared, bound and exported under ABI 15, refuse bad
arguments before any launch, and FusedAdam carries the decay and the warm-up flag in the last two slots of its device block."""
import ctypes

import pytest
import torch

from oracle import cases
from tests import abi_header

BAD_ARG = 10001
NEW = ("mi_adam_ema_step_dev", "mi_swap_f32")


def test_library_exports_the_new_entry_points():
    from medical_image_generation_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 15 and lib.mi_abi_version() == _lib.ABI_VERSION
    for name in NEW:
        assert hasattr(lib, name), name
        assert len(abi_header.params(name)) == len(_lib.signature(name)[1]), name
    # the shadow entry point takes mi_adam_step_dev's arguments with `ema` behind the moments
    old, new = _lib.signature("mi_adam_step_dev")[1], _lib.signature("mi_adam_ema_step_dev")[1]
    assert new == old[:4] + [ctypes.c_void_p] + old[4:]


def _adam_args(**over):
    """Non-null 16-byte aligned host addresses: every refusal below returns before a launch, so nothing is dereferenced."""
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += -a % 16
    args = dict(param=a, grad=a, exp_avg=a, exp_avg_sq=a, ema=a, n=16, hparams=a, decoupled=1, sumsq=None, grad_scale=1.0, step=a)
    args.update(over)
    return buf, tuple(args.values()) + (None,)


@pytest.mark.parametrize("over", [dict(n=0), dict(n=-4), dict(ema=None), dict(grad_scale=0.0), dict(grad_scale=-1.0)],
                         ids=["n0", "n_negative", "null_ema", "zero_grad_scale", "negative_grad_scale"])
def test_adam_ema_refuses_bad_arguments_before_a_launch(over):
    from medical_image_generation_amd import _lib
    keep, args = _adam_args(**over)
    assert _lib.load().mi_adam_ema_step_dev(*args) == BAD_ARG


def test_swap_refuses_bad_arguments_before_a_launch():
    from medical_image_generation_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += -a % 16
    b = a + 64
    assert lib.mi_swap_f32(a, b, 0, None) == BAD_ARG
    assert lib.mi_swap_f32(a, None, 8, None) == BAD_ARG
    assert lib.mi_swap_f32(None, b, 8, None) == BAD_ARG
    assert lib.mi_swap_f32(a + 4, b, 8, None) == BAD_ARG  # one float off the 16-byte grid
    assert lib.mi_swap_f32(a, b + 4, 8, None) == BAD_ARG


def _trainer(**kw):
    from medical_image_generation_amd.trainer import DDPMSchedule, DDPMTrainer
    from medical_image_generation_amd.unet import DiffusionModelUNet
    net = DiffusionModelUNet(**cases.UNET_CASES["unet3d"]["kwargs"])
    return DDPMTrainer(net, lr=1e-3, device="cpu", schedule=DDPMSchedule(device="cpu"), **kw)


def test_block_carries_decay_and_warmup_and_follows_changes():
    tr = _trainer(ema_decay=0.75, ema_warmup=True)
    opt = tr.optimizer
    assert opt.ema is tr.ema and tr.ema.shape == (tr.arena.n_trainable,) and tr.ema.dtype == torch.float32
    assert torch.equal(tr.ema, tr.arena.data[:tr.arena.n_trainable]) and tr.ema.data_ptr() != tr.arena.data.data_ptr()
    opt.push()
    assert opt.hparams.tolist()[6:] == [0.75, 1.0]
    tr.ema_decay, tr.ema_warmup = 0.5, False
    assert opt.ema_decay == 0.5 and tr.ema_decay == 0.5
    opt.push()
    assert opt.hparams.tolist()[6:] == [0.5, 0.0]
    with pytest.raises(ValueError):
        tr.ema_decay = 1.5
    with pytest.raises(ValueError):
        _trainer(ema_decay=-0.1)


def test_default_trainer_keeps_no_shadow():
    tr = _trainer()
    assert tr.ema is None and tr.optimizer.ema is None and tr.ema_decay is None
    tr.optimizer.push()
    assert tr.optimizer.hparams.tolist()[6:] == [0.0, 0.0]
    for fn in (tr.ema_state_dict, tr.reset_ema, lambda: tr.ema_weights().__enter__()):
        with pytest.raises(RuntimeError, match="ema_decay"):
            fn()
    with pytest.raises(RuntimeError):
        tr.ema_decay = 0.9


def test_ema_state_dict_has_the_networks_names_and_takes_trainable_tensors_from_the_shadow():
    tr = _trainer(ema_decay=0.9)
    tr.ema.add_(1.0)
    sd, net_sd = tr.ema_state_dict(), tr.model.state_dict()
    assert list(sd) == list(net_sd) and all(sd[k].shape == net_sd[k].shape and sd[k].device.type == "cpu" for k in sd)
    trainable = {n for n, _, t in tr.model._entries if t}
    assert 0 < len(trainable) < len(sd)  # proj_attn.* never receives a gradient: it is read from the network
    for k in sd:
        assert torch.equal(sd[k], net_sd[k] + 1.0 if k in trainable else net_sd[k]), k
    tr.reset_ema()
    assert torch.equal(tr.ema, tr.arena.data[:tr.arena.n_trainable])
    tr.load_ema_state_dict(sd)
    assert torch.equal(tr.arena.view(next(iter(trainable)), tr.ema), sd[next(iter(trainable))])
