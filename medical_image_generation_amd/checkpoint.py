"""Checkpoints in the reference's `.pth` layout (train_ldm.py:466-505, train_ddpm.py / train_autoencoder.py alike):

    {'epoch', 'network_state_dict', 'optimizer_state_dict', 'validation_loss'[, 'scheduler_state_dict']}

`network_state_dict` is the module's `state_dict()` (reference names and shapes); `optimizer_state_dict` is written in
the layout `torch.optim.Adam[W].state_dict()` has -- per-parameter `step` / `exp_avg` / `exp_avg_sq` keyed by the index of the
parameter in `model.parameters()` order (the order of the reference's modules: tests/test_abi_cpu.py), no entry for parameters that
never receive a gradient (`proj_attn.*`), one param group -- although the fused optimizer of this package keeps its moments in two
flat buffers over the parameter arena.  A checkpoint written by the reference's trainers therefore resumes here and the other way
round.  Files are written with torch.save and read with torch.load(weights_only=True): tensors, numbers, lists and dicts only.

GAN trainers (a `.D` discriminator with its own optimizer, `d_optimizer`) also write the keys train_autoencoder.py:533-553 writes:
'discriminator_state_dict' (BatchNorm running buffers included), 'disc_optimizer_state_dict' (torch.optim.Adam layout over the
discriminator's parameters) and, when a discriminator scheduler is given, 'disc_scheduler_state_dict'; load_model restores each one that
is present (train_autoencoder.py:566-588).  Keys a scheduler adds to the parameter group ('initial_lr', ...) are carried both ways.

A trainer that keeps averaged weights (`ema_decay=`) adds 'ema_state_dict' (the names and shapes of 'network_state_dict', trainable
tensors from the shadow) and 'ema_decay'; without one the key set is unchanged.  The reference's loaders index the keys they know and
ignore the rest, so they still read these files.
"""
from __future__ import annotations

import os

import torch


def _load(path):
    """torch.load(weights_only=True) with numpy scalars admitted: the reference's trainers store `validation_loss` as whatever their
    validation loop returned, which is a numpy float when it came out of np.mean (tensors, numbers, containers and these only)."""
    import numpy as np
    allow = [np.dtype, np.float64, np.float32, np.int64] + [type(np.dtype(t)) for t in (np.float64, np.float32, np.int64)]
    try:
        allow.append(np._core.multiarray.scalar)
    except AttributeError:  # numpy < 2
        allow.append(np.core.multiarray.scalar)
    with torch.serialization.safe_globals(allow):
        return torch.load(path, map_location="cpu", weights_only=True)


_GROUP_KEYS = {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused",
               "decoupled_weight_decay", "params"}


def _group(trainer):
    """The torch parameter group behind `trainer` (a FusedAdam, or a trainer holding one as .optimizer), or None."""
    opt = trainer if isinstance(trainer, torch.optim.Optimizer) else getattr(trainer, "optimizer", None)
    return opt.param_groups[0] if isinstance(opt, torch.optim.Optimizer) else None


def optimizer_state_dict(trainer) -> dict:
    """torch.optim.Adam / AdamW state of the trainer's fused optimizer (CPU tensors, like a torch checkpoint after map_location='cpu').
    `trainer`: a trainer or a FusedAdam (anything with model, arena, exp_avg, exp_avg_sq, step_count and the hyperparameters)."""
    a, model = trainer.arena, trainer.model
    trainable = {n for n, _, t in model._entries if t}
    step = trainer.step_count.detach().cpu().reshape(()).clone()
    m, v = trainer.exp_avg.detach().cpu(), trainer.exp_avg_sq.detach().cpu()
    state, names = {}, [n for n, _ in model.named_parameters()]
    if float(step) > 0:  # torch creates a parameter's state at its first update
        for i, n in enumerate(names):
            if n in trainable:
                state[i] = {"step": step.clone(), "exp_avg": a.view(n, m).clone(), "exp_avg_sq": a.view(n, v).clone()}
    group = {"lr": trainer.lr, "betas": tuple(trainer.betas), "eps": trainer.eps, "weight_decay": trainer.weight_decay, "amsgrad": False,
             "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "decoupled_weight_decay": bool(trainer.decoupled), "params": list(range(len(names)))}
    live = _group(trainer)
    if live is not None:  # what a scheduler added (initial_lr: needed to resume it with last_epoch >= 0)
        group.update({k: v for k, v in live.items() if k not in _GROUP_KEYS})
    return {"state": state, "param_groups": [group]}


def load_optimizer_state_dict(trainer, sd: dict) -> None:
    a, model = trainer.arena, trainer.model
    names = [n for n, _ in model.named_parameters()]
    groups = sd["param_groups"]
    if sum(len(g["params"]) for g in groups) != len(names):
        raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")  # torch's message
    g0 = groups[0]
    trainer.lr, trainer.betas, trainer.eps, trainer.weight_decay = float(g0["lr"]), tuple(g0["betas"]), float(g0["eps"]), float(g0["weight_decay"])
    live = _group(trainer)
    if live is not None:
        live.update({k: v for k, v in g0.items() if k not in _GROUP_KEYS})
    ids = [i for g in groups for i in g["params"]]  # saved id of the k-th parameter
    m, v = torch.zeros_like(trainer.exp_avg, device="cpu"), torch.zeros_like(trainer.exp_avg_sq, device="cpu")
    trainable = {n for n, _, t in model._entries if t}
    steps = set()
    for k, n in enumerate(names):
        st = sd["state"].get(ids[k])
        if st is None:
            continue
        if n not in trainable:
            raise ValueError(f"optimizer state for {n}, which never receives a gradient in this network")
        a.view(n, m).copy_(st["exp_avg"].to(torch.float32))
        a.view(n, v).copy_(st["exp_avg_sq"].to(torch.float32))
        steps.add(float(st["step"]))
    if len(steps) > 1:
        raise ValueError(f"parameters at different step counts {sorted(steps)}: the fused optimizer keeps one")
    trainer.exp_avg.copy_(m)  # in place: a captured optimizer graph reads these buffers
    trainer.exp_avg_sq.copy_(v)
    trainer.step_count.fill_(steps.pop() if steps else 0.0)


def save_model(trainer, results_path, epoch, validation_loss, scheduler=None, disc_scheduler=None) -> str:
    """train_ldm.py:466-490 / train_autoencoder.py:533-563: checkpoints/last_model.pth always, checkpoints/best_model.pth when the
    validation loss improved.  A GAN trainer's discriminator, its optimizer and (given) its scheduler go in as well."""
    save_path = os.path.join(results_path, "checkpoints")
    os.makedirs(save_path, exist_ok=True)
    checkpoint = {"epoch": epoch, "network_state_dict": {k: v.detach().cpu() for k, v in trainer.model.state_dict().items()},
                  "optimizer_state_dict": optimizer_state_dict(trainer), "validation_loss": validation_loss}
    if scheduler:
        checkpoint["scheduler_state_dict"] = scheduler.state_dict()
    if getattr(trainer, "ema", None) is not None:
        checkpoint["ema_state_dict"] = trainer.ema_state_dict()
        checkpoint["ema_decay"] = float(trainer.ema_decay)
    if getattr(trainer, "D", None) is not None:
        checkpoint["discriminator_state_dict"] = {k: v.detach().cpu() for k, v in trainer.D.state_dict().items()}
        checkpoint["disc_optimizer_state_dict"] = optimizer_state_dict(trainer.d_optimizer)
        if disc_scheduler:
            checkpoint["disc_scheduler_state_dict"] = disc_scheduler.state_dict()
    last = os.path.join(save_path, "last_model.pth")
    torch.save(checkpoint, last)
    best = os.path.join(save_path, "best_model.pth")
    if os.path.isfile(best):
        best_loss = _load(best).get("validation_loss", float("inf"))
        if validation_loss < best_loss:
            torch.save(checkpoint, best)
    else:
        torch.save(checkpoint, best)
    return last


def load_model(trainer, load_model_path, load_optimizer=True, lr_scheduler=None, for_training=False, disc_scheduler=None):
    """train_ldm.py:492-505 / train_autoencoder.py:566-591: every part present in the file is restored (the discriminator's only on a
    GAN trainer).  Parameters, moments and step counts are written in place and the hyperparameters reach the device block before the
    next step, so this also holds for a trainer that was already captured.  Returns the epoch to resume at when for_training.
    A trainer with averaged weights restores them from 'ema_state_dict' (in place), or restarts the average at the loaded parameters
    when the file has none; the file's 'ema_decay' is informative, the trainer keeps its own.  Without a shadow the key is ignored."""
    if getattr(trainer, "_ema_swapped", False):
        raise RuntimeError("load_model inside ema_weights(): the arena holds the averaged weights; leave the context first")
    checkpoint = _load(load_model_path)
    trainer.model.load_state_dict(checkpoint["network_state_dict"])
    if getattr(trainer, "ema", None) is not None:
        if "ema_state_dict" in checkpoint:
            trainer.load_ema_state_dict(checkpoint["ema_state_dict"])
        else:
            trainer.reset_ema()
    if load_optimizer:
        load_optimizer_state_dict(trainer, checkpoint["optimizer_state_dict"])
    if lr_scheduler and "scheduler_state_dict" in checkpoint:
        lr_scheduler.load_state_dict(checkpoint["scheduler_state_dict"])
    if getattr(trainer, "D", None) is not None:
        if "discriminator_state_dict" in checkpoint:
            trainer.D.load_state_dict(checkpoint["discriminator_state_dict"])
        if load_optimizer and "disc_optimizer_state_dict" in checkpoint:
            load_optimizer_state_dict(trainer.d_optimizer, checkpoint["disc_optimizer_state_dict"])
        if disc_scheduler and "disc_scheduler_state_dict" in checkpoint:
            disc_scheduler.load_state_dict(checkpoint["disc_scheduler_state_dict"])
    if for_training:
        return checkpoint["epoch"] + 1
