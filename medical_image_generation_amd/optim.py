"""`FusedAdam`: the torch.optim.Optimizer face of a trainer's fused Adam / AdamW, so that torch LR schedulers drive it
(train_ldm.py:124-130, 551-553; train_autoencoder.py:478-486, 632-638) -- also through a captured hipGraph.

The optimizer state itself stays where the kernels read it: the flat parameter arena, two flat moment buffers and a device step count.
One parameter group holds the module's parameters in `parameters()` order, with plain Python floats for lr / betas / eps / weight_decay
(so state_dict() and get_last_lr() look like torch's).  The kernel (mi_adam_step_dev) reads its hyperparameters from a small device
block {lr, beta1, beta2, eps, weight_decay, max_norm}; before every launch or graph replay the group is compared with the values last
pushed and the block is rewritten when they differ -- one host-to-device copy on the current stream, never inside a capture.  That is
how a replayed optimizer graph follows `scheduler.step()`, a changed `trainer.lr` or a loaded checkpoint.

With `ema=` (fp32 [arena.n_trainable]) the update also moves an exponential moving average of the parameters in the same launch
(mi_adam_ema_step_dev).  Whether a shadow exists is fixed when a graph is captured; `ema_decay` and `ema_warmup` are the last two slots
of the device block and travel through push() like lr.
"""
from __future__ import annotations

import torch

from ._lib import call, ptr

F32 = torch.float32


class FusedAdam(torch.optim.Optimizer):
    """Adam / AdamW (torch.optim defaults, + clip_grad_norm_ with `max_grad_norm`) over one module's arena.

    model / arena: a HipModule and its ParamArena; exp_avg, exp_avg_sq: fp32 [arena.n_trainable]; step_count: fp32 [1] on the device.
    grad_scale: 1 / world (the gradient buffer holds the SUM over data-parallel ranks).  step() launches the update eagerly;
    step(replay=graph) replays a captured graph that holds launch() instead.  Both push changed hyperparameters first.
    ema: fp32 [arena.n_trainable] or None -- the shadow e += (1 - d) * (p - e) the update kernel moves along; d = ema_decay, or
    min(ema_decay, (1 + step) / (10 + step)) with ema_warmup."""

    def __init__(self, model, arena, exp_avg, exp_avg_sq, step_count, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 decoupled=False, max_grad_norm=None, grad_scale=1.0, ema=None, ema_decay=0.0, ema_warmup=False):
        self.model, self.arena = model, arena
        self.exp_avg, self.exp_avg_sq, self.step_count = exp_avg, exp_avg_sq, step_count
        if ema is not None and (ema.dtype != F32 or ema.shape != exp_avg.shape or ema.device != exp_avg.device or not ema.is_contiguous()):
            raise ValueError("ema must be a contiguous fp32 [arena.n_trainable] tensor on the moments' device")
        self.ema, self.ema_decay, self.ema_warmup = ema, ema_decay, bool(ema_warmup)
        self.decoupled = bool(decoupled)
        self.max_grad_norm = max_grad_norm
        self.grad_scale = float(grad_scale)
        defaults = {"lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps), "weight_decay": float(weight_decay),
                    "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                    "decoupled_weight_decay": self.decoupled}
        self._ready = False
        super().__init__(list(model.parameters()), defaults)
        self._ready = True
        self.hparams = torch.zeros(8, dtype=F32, device=exp_avg.device)  # {lr, beta1, beta2, eps, weight_decay, max_norm, ema decay, ema warm-up}
        self.sumsq = torch.zeros(1, dtype=F32, device=exp_avg.device)
        self.sumsq_partials = None  # fixed_order_norm(): fp64 [MI_VQ_PARTIALS] scratch of mi_sumsq_det_f32
        self._pushed = None

    def fixed_order_norm(self):
        """Compute the clip norm with mi_sumsq_det_f32 (workgroup partials folded in a fixed order) instead of mi_sumsq_f32 (float atomics
        in arrival order): a captured step then equals the eager one bit for bit (VQAETrainer).  Call before capture()."""
        from ._lib import constants
        self.sumsq_partials = torch.empty(constants()["MI_VQ_PARTIALS"], dtype=torch.float64, device=self.exp_avg.device)

    def add_param_group(self, param_group):
        if self._ready:
            raise ValueError("FusedAdam keeps one parameter group: its hyperparameter block covers the whole parameter arena")
        super().add_param_group(param_group)

    # ---- hyperparameters (the trainer's lr / betas / eps / weight_decay properties read and write these)
    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, v):
        self.param_groups[0]["lr"] = float(v)

    @property
    def betas(self):
        return self.param_groups[0]["betas"]

    @betas.setter
    def betas(self, v):
        self.param_groups[0]["betas"] = (float(v[0]), float(v[1]))

    @property
    def eps(self):
        return self.param_groups[0]["eps"]

    @eps.setter
    def eps(self, v):
        self.param_groups[0]["eps"] = float(v)

    @property
    def weight_decay(self):
        return self.param_groups[0]["weight_decay"]

    @weight_decay.setter
    def weight_decay(self, v):
        self.param_groups[0]["weight_decay"] = float(v)

    @property
    def ema_decay(self):
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, v):
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"ema_decay must lie in [0, 1], got {v}")
        self._ema_decay = float(v)

    @property
    def clip(self) -> bool:
        return self.max_grad_norm is not None and self.max_grad_norm > 0

    def _values(self):
        g = self.param_groups[0]
        if isinstance(g["lr"], torch.Tensor):
            raise TypeError("FusedAdam takes a float lr (its kernel reads the value from its own device block)")
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                float(self.max_grad_norm) if self.clip else 0.0, float(self.ema_decay), 1.0 if self.ema_warmup else 0.0)

    def push(self):
        """Write the device hyperparameter block if the group changed since the last push (current stream, outside any capture)."""
        vals = self._values()
        if vals == self._pushed:
            return
        if self.hparams.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdam.push() inside a graph capture: push before capturing")
        self.hparams.copy_(torch.tensor(vals, dtype=F32))
        self._pushed = vals

    def launch(self):
        """The kernels of one update on the current stream (capturable): squared gradient norm when clipping, then Adam[W] reading the
        device block (and moving the shadow when there is one).  Does not push."""
        a = self.arena
        n = a.n_trainable
        if self.clip and self.sumsq_partials is not None:
            call("mi_sumsq_det_f32", ptr(a.grad), n, ptr(self.sumsq), ptr(self.sumsq_partials))
        elif self.clip:
            call("mi_sumsq_f32", ptr(a.grad), n, ptr(self.sumsq), 0)
        tail = (n, ptr(self.hparams), int(self.decoupled), ptr(self.sumsq) if self.clip else None, self.grad_scale, ptr(self.step_count))
        if self.ema is None:
            call("mi_adam_step_dev", ptr(a.data), ptr(a.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), *tail)
        else:
            call("mi_adam_ema_step_dev", ptr(a.data), ptr(a.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self.ema), *tail)

    @torch.no_grad()
    def step(self, closure=None, replay=None):
        """One update from the gradients in arena.grad: eager launch, or `replay` (a captured graph holding launch()) when given."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.push()
        if replay is None:
            self.launch()
        else:
            replay.replay()
        return loss

    def zero_grad(self, set_to_none=True):
        """The trainers write fresh gradients into the arena every step; nothing to clear."""

    # ---- checkpoints: torch.optim.Adam[W] layout (checkpoint.optimizer_state_dict)
    def state_dict(self):
        from .checkpoint import optimizer_state_dict
        return optimizer_state_dict(self)

    def load_state_dict(self, state_dict):
        """Moments and step count are copied in place and the hyperparameters go through the device block: takes effect on the next
        step or replay, captured or not."""
        from .checkpoint import load_optimizer_state_dict
        load_optimizer_state_dict(self, state_dict)
